"""Preview surfaces on the device: ffgpu_preview_bgr_dev / _nv12_dev on synthetic frames and surfaces, and behind a forward and a draw on the real net,
against tests/preview/previewref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  Sources, destination surfaces and 64 guard bytes
around each lie in one arena of seeded random bytes; the WHOLE arena is compared byte for byte, so every byte the contract leaves alone -- the
sources, the gaps of a wall, row padding, kept bars, the guards -- must have stayed; the call is then repeated from the same bytes and must give the
same.  The seeded cases are built on the CPU once (tests/preview/fuzzcases.py) and shared by the tests; tests/test_preview_abi.py holds the
conditions that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from overlay import drawref
from preview import fuzzcases, previewref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
GUARD = fuzzcases.GUARD


def differ(what, got, want, regions=()):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return
    for name, lo, nb in regions:
        hit = bad[(bad >= lo - GUARD) & (bad < lo + nb + GUARD)]
        if len(hit):
            pytest.fail("%s: %s: %d bytes differ, first at region offset %d (region of %d bytes): got %d, want %d"
                        % (what, name, len(hit), int(hit[0]) - lo, nb, got[hit[0]], want[hit[0]]), pytrace=False)
    pytest.fail("%s: %d bytes differ, first at %d: got %d, want %d" % (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]]), pytrace=False)


def descs(c, which, base, a=0, b=None):
    """the case's sources or destinations a .. b - 1 as the wrappers take them"""
    out = []
    for d in which[a:b]:
        if d is None:
            out.append(None)
        elif c.fmt == "bgr":
            out.append((base + d[0], d[1], d[2], d[3]))
        else:
            out.append((base + d[0], base + d[1], d[2], d[3], d[4], d[5]))
    return out


def c_spec(F, c):
    return F.preview_spec(c.fit, c.fill, c.keep)


def c_panes(F, c, a=0, b=None):
    return [F.preview_pane(p[:4], p[4:]) for p in c.panes[a:b]]


def run(F, c, splits=None):
    """the case on the device, as one call or split into several at the given pane numbers; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    fn = F.preview_bgr_dev if c.fmt == "bgr" else F.preview_nv12_dev
    cuts = [0] + list(splits or []) + [c.n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a != b:
            fn(descs(c, c.srcs, base, a, b), descs(c, c.dsts, base, a, b), c_panes(F, c, a, b), c_spec(F, c))
    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("fmt,name", fuzzcases.PARAMS)
def test_preview(F, fmt, name):
    """one call: the whole arena against previewref; the same call again from the same bytes: the same bytes"""
    c = fuzzcases.get(fmt, name)
    got = run(F, c)
    differ(c.what, got, c.want, c.regions())
    assert run(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_split_calls_leave_the_same_bytes(F, fmt):
    """130 panes in one call and in calls of 1, 63, 3 and 63 panes"""
    c = fuzzcases.cases(fmt)["launch table"]
    assert c.n == 130
    differ("%s split" % c.what, run(F, c, [1, 64, 67]), c.want, c.regions())


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_rejections(F, fmt):
    """one call per reason, the message matched, with the pane's index where there is one; nothing is launched: the arena stays; a working call
    afterwards"""
    import torch
    c = fuzzcases.cases(fmt)["wall"]
    dev = torch.from_numpy(c.start.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    nv12 = fmt == "nv12"
    fn = L.ffgpu_preview_nv12_dev if nv12 else L.ffgpu_preview_bgr_dev
    table = F.nv12_frame_table if nv12 else F.bgr_frame_table
    n = c.n
    gs, gd = descs(c, c.srcs, base), descs(c, c.dsts, base)

    def tab(which, k=None, **kw):
        t = table(which)
        for name_, v in kw.items():
            setattr(t[k], name_, v)
        return t

    def panes(k=None, **kw):
        arr = (F.PreviewPane * n)(*c_panes(F, c))
        for name_, v in kw.items():
            setattr(arr[k], name_, v)
        return arr

    def sp(**kw):
        s = c_spec(F, c)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(srcs=tab(gs), dsts=tab(gd), pn=panes(), np_=n, spec=sp()):
        return fn(srcs, dsts, pn, np_, spec, None)
    fill3 = sp()
    fill3.fill[3] = 1
    addr = "y" if nv12 else "bgr"
    p1 = c.panes[1]
    cases = [(dict(srcs=None), "NULL srcs"), (dict(dsts=None), "NULL dsts"), (dict(pn=None), "NULL panes"), (dict(spec=None), "NULL spec"),
             (dict(np_=0), "0 panes (1..4096)"), (dict(np_=4097), "4097 panes (1..4096)"), (dict(spec=sp(fit=2)), "fit 2 is neither FFGPU_PREVIEW_STRETCH nor FFGPU_PREVIEW_FIT"),
             (dict(spec=sp(flags=2)), "unknown flags 0x2"), (dict(spec=fill3), "fill[3] must be 0"), (dict(spec=sp(reserved=1)), "spec: reserved must be 0"),
             (dict(srcs=tab(gs, 1, w=0)), "source 1: bad size 0 x 48"), (dict(dsts=tab(gd, 3, h=0)), "destination 3: bad size 97 x 0"),
             (dict(srcs=tab(gs, 0, reserved=1)), "source 0: reserved must be 0"), (dict(dsts=tab(gd, 2, reserved=1)), "destination 2: reserved must be 0"),
             (dict(pn=panes(1, sw=5)), "pane 1: a source region of 5 x 0 (both 0 for the whole frame, or neither)"),
             (dict(pn=panes(3, dh=0)), "pane 3: a pane of %d x 0 (both 0 for the whole surface, or neither)" % c.panes[3][6]),
             (dict(pn=panes(0, sx=2)), "pane 0: the whole frame as the source region wants sx = sy = 0, not (2, 0)"),
             (dict(pn=panes(1, sx=40, sy=0, sw=30, sh=10)), "pane 1: the source region 30 x 10 at (40, 0) is outside the frame of 64 x 48"),
             (dict(pn=panes(5, dy=50)), "pane 5: the pane %d x %d at (%d, 50) is outside the surface of 97 x 61" % (c.panes[5][6], c.panes[5][7], c.panes[5][4])),
             (dict(pn=panes(2, dw=8194)), "pane 2: a pane of 8194 x %d (1..8192 each)" % c.panes[2][7]),
             (dict(srcs=tab(gs, 3, **{addr: gd[3][0]})), "pane 3: the source and the destination are the same pixels"),
             (dict(pn=panes(3, dx=p1[4], dy=p1[5] + 2)), "panes 1 and 3 overlap in one destination surface")]
    if nv12:
        cases += [(dict(srcs=tab(gs, 0, pitch_y=10)), "source 0: pitch_y 10 is below w = 31"), (dict(dsts=tab(gd, 1, matrix=4)), "destination 1: matrix 4"),
                  (dict(srcs=tab(gs, 3, uv=gs[3][1] + 1)), "is odd (U V pairs are read"), (dict(dsts=tab(gd, 0, uv=gd[0][1] + 1)), "is odd (U V pairs are written"),
                  (dict(pn=panes(1, sx=1, sy=0, sw=30, sh=10)), "pane 1: NV12 wants even sx, sy, dx, dy, not (1, 0)"),
                  (dict(pn=panes(0, dy=3)), "pane 0: NV12 wants even sx, sy, dx, dy, not (0, 0) and (2, 3)")]
    else:
        cases += [(dict(srcs=tab(gs, 0, pitch=50)), "source 0: pitch 50 is below 3 w = 93"), (dict(dsts=tab(gd, 0, pitch=100)), "destination 0: pitch 100 is below 3 w = 291")]
    for kw, msg in cases:
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == c.start.tobytes()                            # nothing was launched
    differ("after the rejections", run(F, c), c.want, c.regions())


# ---------------------------------------------------------------------------------------------------------------- behind the real net
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_forward_draw_preview(F, net, picture, fmt):
    """data/test.bmp through a forward on the real net, its boxes drawn into the frame with thickness 4, then the frame's 320 x 320 middle scaled to an
    80 x 80 pane of a small surface: the pane equals previewref applied to drawref's frame; frame, padding and the rest of the surface stay"""
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    rng = np.random.default_rng(9300)
    h, w = picture.shape[:2]
    region, pane = (160, 52, 320, 320), (8, 4, 80, 80)
    if fmt == "bgr":
        pitch, dp = 3 * w + 4, 3 * 100 + 3
        o_dst = GUARD + h * pitch + GUARD + 1
        arena = rng.integers(0, 256, o_dst + 90 * dp + GUARD, dtype=np.uint8)
        previewref.view(arena, GUARD, h, 3 * w, pitch)[...] = picture.reshape(h, 3 * w)
        src, dst = (GUARD, w, h, pitch), (o_dst, 100, 90, dp)
    else:
        Y, UV = bgr_to_nv12(picture)
        o_uv = GUARD + h * w + GUARD
        o_dy = o_uv + UV.size + GUARD + 1
        o_duv = (o_dy + 90 * 100 + GUARD + 1) & ~1
        arena = rng.integers(0, 256, o_duv + 45 * 100 + GUARD, dtype=np.uint8)
        arena[GUARD:GUARD + h * w] = Y.reshape(-1)
        arena[o_uv:o_uv + UV.size] = UV.reshape(-1)
        src, dst = (GUARD, o_uv, w, h, w, UV.shape[1]), (o_dy, o_duv, 100, 90, 100, 100)
    dev = torch.from_numpy(arena.copy()).cuda()
    base = dev.data_ptr()

    def at(d):
        return (base + d[0],) + tuple(d[1:]) if fmt == "bgr" else (base + d[0], base + d[1]) + tuple(d[2:])
    with net.executor(1) as ex:
        if fmt == "bgr":
            ex.forward_bgr_frames_dev([at(src)])
            boxes = ex.read_boxes(0)
            ex.draw_bgr([at(src)], F.DRAW_ENTRIES, color=(0, 255, 0), thickness=4)
            F.preview_bgr_dev([at(src)], [at(dst)], [F.preview_pane(region, pane)], F.preview_spec())
        else:
            ex.forward_nv12_frames_dev([at(src)])
            boxes = ex.read_boxes(0)
            ex.draw_nv12([at(src)], F.DRAW_ENTRIES, color=(81, 90, 240), thickness=4)
            F.preview_nv12_dev([at(src)], [at(dst)], [F.preview_pane(region, pane)], F.preview_spec())
        torch.cuda.synchronize()
    assert len(boxes) > 0
    want = arena.copy()
    if fmt == "bgr":
        drawref.draw_bgr(want, src[0], w, h, src[3], boxes, drawref.colours_of(boxes, (0, 255, 0)), 4)
    else:
        drawref.draw_nv12(want, src[0], src[1], w, h, src[4], src[5], boxes, drawref.colours_of(boxes, (81, 90, 240)), 4)
    drawn = want.copy()
    previewref.preview(want, fmt, [src], [dst], [region + pane])
    assert (drawn != arena).sum() > 500 and (want != drawn).sum() > 80 * 80 // 2
    # the outlines reach the pane: it differs from the preview of the frame nobody drew into
    plain = previewref.preview(arena.copy(), fmt, [src], [dst], [region + pane])
    assert (plain[dst[0]:] != want[dst[0]:]).sum() > 20
    differ("%s forward, draw, preview" % fmt, dev.cpu().numpy(), want)
