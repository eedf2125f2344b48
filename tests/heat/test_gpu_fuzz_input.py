"""Heat maps on the device: ffgpu_heat_boxes_dev / ffgpu_heat_reset_dev and ffgpu_heat_blend_bgr_dev / _nv12_dev (the operators, on synthetic records,
lists, states and targets) and ffgpu_exec_heat (behind forwards and a merge on the real net, its state blended into the frames under the draw and the
captions), against tests/heat/heatref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  State, rows and targets lie in one arena of
seeded random bytes with 64 guard bytes around each; the WHOLE arena is compared byte for byte (every word of the family is an integer), so every
byte the contract leaves alone must have stayed.  The seeded cases are built on the CPU once (tests/heat/fuzzcases.py) and shared by the tests;
tests/test_heat_abi.py holds the conditions that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from captions import textref
from captions.fuzzcases import names_rows
from heat import fuzzcases, heatref
from overlay import drawref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX, DETS, GUARD = heatref.BOX_DTYPE, heatref.DETS_DTYPE, fuzzcases.GUARD
NAN = float("nan")
BLEND_PARAMS = [(fmt, name) for fmt in fuzzcases.FORMATS for name in fuzzcases.BLEND_NAMES]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def c_spec(F, sp):
    return F.heat_spec(sp.gw, sp.gh, sp.cell_log2, sp.mode, sp.anchor, sp.spread, sp.gain, sp.decay_shift, float(sp.min_score), sp.classes)


def c_blend(F, bs):
    return F.heat_blend_spec(bs.gw, bs.gh, bs.cell_log2, bs.full_scale, bs.floor, bs.opacity, bs.smooth, bs.ramp_alpha, bs.palette)


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


# ---------------------------------------------------------------------------------------------------------------- accumulate
def run_acc(F, c, splits=None):
    """the case on the device, as one call or split into several at the given record numbers; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    d_recs = to_dev(c.recs)
    d_flat = None if c.flat is None else to_dev(c.flat)
    cs = c_spec(F, c.spec)
    cuts = [0] + list(splits or []) + [c.n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == b:
            continue
        lists = None if d_flat is None else d_flat.data_ptr() + (0 if c.first is not None else 24 * a * c.stride)
        F.heat_boxes_dev(d_recs.data_ptr() + DETS.itemsize * a, lists, c.stride if d_flat is not None else 0, c.streams[a:b], cs, base + c.state_off, c.nstreams,
                         base + c.row_off + 4 * heatref.ROW * a, list_first=None if c.first is None else c.first[a:b])
    torch.cuda.synchronize()
    assert d_recs.cpu().numpy().tobytes() == c.recs.tobytes() and (d_flat is None or d_flat.cpu().numpy().tobytes() == c.flat.view(np.uint8).tobytes())
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.ACC_NAMES)
def test_accumulate(F, name):
    """one call from the case's first state: the whole arena against heatref; the same call again from the same state: the same bytes"""
    c = fuzzcases.acc_cases()[name]
    got = run_acc(F, c)
    differ(c.what, got, c.want, c.regions())
    assert run_acc(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("name", ["grid 3x2 box", "grid 17x5 anchor", "records 65", "records 130", "junk state", "saturate"])
def test_split_calls_leave_the_same_bytes(F, name):
    """the sequence cut into several calls (the state carries the streams across) leaves what one call leaves; short ones are cut at every record"""
    c = fuzzcases.acc_cases()[name]
    rng = np.random.default_rng(7700)
    for cuts in ([c.n // 2], sorted(int(v) for v in rng.integers(0, c.n + 1, 3)), list(range(1, c.n)) if c.n <= 12 else [1, 64, c.n - 1]):
        differ("%s split at %s" % (c.what, cuts), run_acc(F, c, cuts), c.want, c.regions())


def test_reset(F):
    """ffgpu_heat_reset_dev zeroes one stream or all and nothing else"""
    import torch
    c = fuzzcases.acc_cases()["grid 3x2 box"]
    got = run_acc(F, c)
    nb, one = heatref.state_nbytes(3, 3, 2), heatref.stream_nbytes(3, 2)
    assert all(got[c.state_off + s * one:c.state_off + (s + 1) * one].any() for s in range(3))
    dev = torch.from_numpy(got.copy()).cuda()
    F.heat_reset_dev(dev.data_ptr() + c.state_off, 3, 3, 2, 1)
    torch.cuda.synchronize()
    want = got.copy()
    want[c.state_off + one:c.state_off + 2 * one] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    F.heat_reset_dev(dev.data_ptr() + c.state_off, 3, 3, 2)
    torch.cuda.synchronize()
    want[c.state_off:c.state_off + nb] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    p = dev.data_ptr()
    for args, msg in (((None, 3, 3, 2, -1), "NULL state"), ((p + 8, 3, 3, 2, -1), "16-byte aligned"), ((p, 0, 3, 2, -1), "0 streams"), ((p, 3, 129, 2, -1), "129 x 2 cells"),
                      ((p, 3, 3, 0, -1), "3 x 0 cells"), ((p, 3, 3, 2, 3), "stream 3"), ((p, 3, 3, 2, -2), "stream -2")):
        assert F.lib().ffgpu_heat_reset_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())


def test_accumulate_rejections(F):
    """every rejected argument with its message, the entry's index where there is one; the state (and everything else) stays as it was"""
    import torch
    c = fuzzcases.acc_cases()["grid 17x5 anchor"]
    before = run_acc(F, c)
    dev = torch.from_numpy(before.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    d_recs, d_flat = to_dev(c.recs), to_dev(c.flat)
    r, fl, st, rw, n = d_recs.data_ptr(), d_flat.data_ptr(), base + c.state_off, base + c.row_off, c.n
    streams = (C.c_int * n)(*c.streams)
    cls = (C.c_ubyte * 4)(1, 1, 0, 1)

    def sp(**kw):
        s = c_spec(F, c.spec)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(recs=r, lists=fl, stride=c.stride, first=None, strm=streams, nt=n, spec=sp(), state=st, ns=3, rows=rw):
        return L.ffgpu_heat_boxes_dev(recs, lists, stride, first, strm, nt, spec, state, ns, rows, None)
    bad_stream = (C.c_int * n)(*c.streams)
    bad_stream[4] = 3
    low_stream = (C.c_int * n)(*c.streams)
    low_stream[2] = -2
    neg_first = (C.c_int * n)(*([0] * n))
    neg_first[5] = -1
    for kw, msg in ((dict(recs=None), "NULL records"), (dict(strm=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(state=None), "NULL state"),
                    (dict(rows=None), "NULL rows"), (dict(nt=0), "0 targets"), (dict(nt=-1), "-1 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"),
                    (dict(strm=bad_stream), "target 4: stream 3 is outside -1 .. 2"), (dict(strm=low_stream), "target 2: stream -2"),
                    (dict(spec=sp(gw=0)), "a grid of 0 x 5 cells (1..128 each)"), (dict(spec=sp(gw=129)), "a grid of 129 x 5 cells"), (dict(spec=sp(gh=0)), "a grid of 17 x 0 cells"),
                    (dict(spec=sp(gh=129)), "a grid of 17 x 129 cells"), (dict(spec=sp(cell_log2=0)), "cell_log2 0 is outside 1..8"), (dict(spec=sp(cell_log2=9)), "cell_log2 9 is outside 1..8"),
                    (dict(spec=sp(mode=2)), "mode 2 is neither FFGPU_HEAT_ANCHOR nor FFGPU_HEAT_BOX"), (dict(spec=sp(mode=-1)), "mode -1"),
                    (dict(spec=sp(flags=1)), "unknown flags 0x1"), (dict(spec=sp(flags=-1)), "unknown flags"), (dict(spec=sp(anchor=2)), "anchor 2 is neither 0 nor 1"),
                    (dict(spec=sp(spread=-1)), "spread -1 is outside 0..4"), (dict(spec=sp(spread=5)), "spread 5 is outside 0..4"),
                    (dict(spec=sp(mode=1)), "spread 1 with FFGPU_HEAT_BOX (0 then)"), (dict(spec=sp(gain=0)), "gain 0 is outside 1..65536"),
                    (dict(spec=sp(gain=65537)), "gain 65537 is outside 1..65536"), (dict(spec=sp(decay_shift=-1)), "decay_shift -1 is outside 0..16"),
                    (dict(spec=sp(decay_shift=17)), "decay_shift 17 is outside 0..16"), (dict(spec=sp(nclasses=3)), "nclasses 3 (0 with NULL classes, else 1..256)"),
                    (dict(spec=sp(classes=C.addressof(cls))), "nclasses 0"), (dict(spec=sp(classes=C.addressof(cls), nclasses=257)), "nclasses 257"),
                    (dict(spec=sp(reserved=1)), "reserved must be 0"), (dict(state=st + 8), "the state must be 16-byte aligned"),
                    (dict(stride=0), "bad list_stride 0"), (dict(stride=2 ** 24 + 1), "bad list_stride"), (dict(first=neg_first), "target 5: negative list start -1")):
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == before.tobytes()                            # nothing was launched: the state, too, is as it was
    differ("after the rejections", run_acc(F, c), c.want, c.regions())                # and the next valid call is right


# ---------------------------------------------------------------------------------------------------------------- blend
def descs(c, base):
    """the case's targets as the wrappers take them"""
    out = []
    for d in c.desc:
        if d is None:
            out.append(None)
        elif c.fmt == "bgr":
            out.append((base + d[0], d[1], d[2], d[3]))
        else:
            out.append((base + d[0], base + d[1], d[2], d[3], d[4], d[5]))
    return out


def run_blend(F, c, times=1):
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    fn = F.heat_blend_bgr_dev if c.fmt == "bgr" else F.heat_blend_nv12_dev
    for _ in range(times):
        fn(base + c.state_off, c.nstreams, c.streams, descs(c, base), c_blend(F, c.bspec))
    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("fmt,name", BLEND_PARAMS)
def test_blend(F, fmt, name):
    """one call: the whole arena against heatref -- every byte that is not written stayed, the state among them"""
    c = fuzzcases.blend_cases(fmt)[name]
    differ(c.what, run_blend(F, c), c.want, c.regions())


@pytest.mark.parametrize("fmt,name", [("bgr", "edges smooth"), ("nv12", "edges smooth"), ("bgr", "big cell"), ("nv12", "cold blocks ramp")])
def test_the_same_blend_twice(F, fmt, name):
    """the same call twice against the reference applied twice: the second blend reads what the first wrote"""
    c = fuzzcases.blend_cases(fmt)[name]
    want = c.want.copy()
    c.apply(want)
    assert (want != c.want).any()
    differ("%s twice" % c.what, run_blend(F, c, 2), want, c.regions())


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_blend_rejections(F, fmt):
    """every rejected argument with its message and the target's index; nothing is written, and a working call afterwards"""
    import torch
    c = fuzzcases.blend_cases(fmt)["big cell"]
    dev = torch.from_numpy(c.start.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    nv12 = fmt == "nv12"
    fn = L.ffgpu_heat_blend_nv12_dev if nv12 else L.ffgpu_heat_blend_bgr_dev
    table = F.nv12_frame_table if nv12 else F.bgr_frame_table
    good, n = descs(c, base), len(c.desc)
    streams = (C.c_int * n)(*c.streams)

    def sp(**kw):
        s = c_blend(F, c.bspec)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def tab(k=None, **kw):
        t = table(good)
        for name_, v in kw.items():
            setattr(t[k], name_, v)
        return t

    def call(state=base + c.state_off, ns=c.nstreams, strm=streams, targets=tab(), nt=n, spec=sp()):
        return fn(state, ns, strm, targets, nt, spec, None)
    high, low = (C.c_int * n)(*c.streams), (C.c_int * n)(*c.streams)
    high[1], low[0] = 2, -2
    cases = [(dict(state=None), "NULL state"), (dict(strm=None), "NULL streams"), (dict(targets=None), "NULL targets"), (dict(spec=None), "NULL spec"),
             (dict(nt=0), "0 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"), (dict(state=base + c.state_off + 4), "the state must be 16-byte aligned"),
             (dict(strm=high), "target 1: stream 2 is outside -1 .. 1"), (dict(strm=low), "target 0: stream -2"),
             (dict(spec=sp(gw=0)), "a grid of 0 x 1 cells (1..128 each)"), (dict(spec=sp(gh=129)), "a grid of 2 x 129 cells"), (dict(spec=sp(cell_log2=0)), "cell_log2 0 is outside 1..8"),
             (dict(spec=sp(cell_log2=9)), "cell_log2 9 is outside 1..8"), (dict(spec=sp(full_scale=-1)), "negative full_scale -1"), (dict(spec=sp(floor=-1)), "floor -1 is outside 0..255"),
             (dict(spec=sp(floor=256)), "floor 256 is outside 0..255"), (dict(spec=sp(opacity=0)), "opacity 0 is outside 1..255"), (dict(spec=sp(opacity=256)), "opacity 256 is outside 1..255"),
             (dict(spec=sp(sampling=2)), "sampling 2 is neither FFGPU_HEAT_NEAREST nor FFGPU_HEAT_SMOOTH"), (dict(spec=sp(flags=2)), "unknown flags 0x2"),
             (dict(spec=sp(reserved=(C.c_int * 2)(0, 1))), "reserved must be 0"),
             (dict(targets=tab(1, w=0)), "target 1: bad size 0 x 66"), (dict(targets=tab(0, h=-1)), "target 0: bad size 129 x -1"), (dict(targets=tab(1, reserved=1)), "target 1: reserved must be 0")]
    if nv12:
        cases += [(dict(targets=tab(0, pitch_y=10)), "target 0: pitch_y 10 is below w = 129"), (dict(targets=tab(1, pitch_uv=65)), "target 1: pitch_uv 65 is odd"),
                  (dict(targets=tab(1, uv=good[1][1] + 1)), "is odd (U V pairs are written"), (dict(targets=tab(0, matrix=4)), "target 0: matrix 4")]
    else:
        cases += [(dict(targets=tab(0, pitch=100)), "target 0: pitch 100 is below 3 w = 387")]
    for kw, msg in cases:
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == c.start.tobytes()                            # nothing was written
    differ("after the rejections", run_blend(F, c), c.want, c.regions())


# ---------------------------------------------------------------------------------------------------------------- behind the real net
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


def flat_of(boxes, S):
    flat = np.zeros((len(boxes), S), BOX)
    for t, b in enumerate(boxes):
        flat[t, :len(b)] = b
    return flat.reshape(-1)


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_heat_then_blend_draw_caption_bgr(F, net, picture, flags):
    """data/test.bmp in 2 entries as two video streams over two forwards (flags 32: FFGPU_SPLIT2), the second shifted: forward, ffgpu_exec_heat
    (ENTRIES); state and rows equal heatref on the boxes read back, the executor's records, lists and graph stay.  Then the order of the contract:
    heat blend, draw, caption into the frames, against heatref, drawref and textref composed.  Rejected calls leave the state and the executor usable."""
    import torch
    h, w = picture.shape[:2]
    pitch = 3 * w + 4
    hs = heatref.Spec(40, 27, 4, heatref.ANCHOR, 1, 2, 200, 1, 0.25)
    bs = heatref.BlendSpec(40, 27, 4, 0, 4, 160, True, True)
    names = names_rows([b"class %d" % k for k in range(80)])
    d_names = to_dev(names)
    ts = textref.Spec(textref.NAME | textref.SCORE | textref.CAPTION_OPAQUE, 0.25, textref.NONE, 1, (255, 255, 255), palette=[(0, 0, 255), (0, 160, 0)], names=names)
    state = heatref.State(2, 40, 27)
    with net.executor(2, flags) as ex:
        S = ex.cand_capacity
        d_state = torch.zeros(heatref.state_nbytes(2, 40, 27), dtype=torch.uint8, device="cuda")
        d_rows = torch.full((4 * 2 * heatref.ROW,), 0xA5, dtype=torch.uint8, device="cuda")
        for k in range(2):
            buf = np.zeros((2, h, pitch), np.uint8)
            buf[0, :, :3 * w] = np.roll(picture, 10 * k, axis=1).reshape(h, 3 * w)
            buf[1, :, :3 * w] = np.roll(picture, -10 * k, axis=0).reshape(h, 3 * w)
            dev = torch.from_numpy(buf).cuda()
            frames = [(dev.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)]
            ex.forward_bgr_frames_dev(frames)
            dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(2)], ex.graph_captures
            ex.heat([1, 0], c_spec(F, hs), d_state.data_ptr(), 2, d_rows.data_ptr())
            torch.cuda.synchronize()
            assert all(len(b) >= 2 for b in boxes)
            rows = heatref.accumulate(dets, flat_of(boxes, S), S, None, [1, 0], hs, state)
            assert d_rows.cpu().numpy().tobytes() == rows.tobytes(), "rows of forward %d" % k
            assert d_state.cpu().numpy().tobytes() == state.tobytes(), "state after forward %d" % k
            assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(2))
        assert state.hdr[:, 0].tolist() == [2, 2] and int(state.hdr[:, 1].min()) >= 200 and int(rows[:, 0].min()) >= 2
        stride = 8
        d_items = torch.full((2 * stride * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        F.heat_blend_bgr_dev(d_state.data_ptr(), 2, [1, 0], frames, c_blend(F, bs))
        ex.draw_bgr(frames, F.DRAW_ENTRIES, color=(0, 255, 0), thickness=2)
        ex.caption_bgr(frames, F.caption_spec(True, True, False, True, 0.25, F.ZONES_NONE, 1, ts.fg, ts.color, ts.palette, d_names.data_ptr(), len(names)), d_items.data_ptr(), stride)
        torch.cuda.synchronize()
        want, font = buf.copy().reshape(-1), F.font_builtin()
        items = textref.caption_boxes(dets, flat_of(boxes, S), S, None, ts, None, stride)
        for t in range(2):
            heatref.blend_bgr(want, t * h * pitch, w, h, pitch, state.hdr[1 - t], state.cells[1 - t], bs)
        heat_only = want.copy()
        for t in range(2):
            drawref.draw_bgr(want, t * h * pitch, w, h, pitch, boxes[t], drawref.colours_of(boxes[t], (0, 255, 0)), 2)
            textref.draw_bgr(want, t * h * pitch, w, h, pitch, items[t], font)
        assert (heat_only != buf.reshape(-1)).sum() > 1000 and (want != heat_only).sum() > 1000      # the map shows, and the overlays lie on top of it
        differ("frames", dev.cpu().numpy().reshape(-1), want)
        # rejected: the executor and the state stay usable
        L, cs = F.lib(), c_spec(F, hs)
        two = (C.c_int * 2)(0, 1)
        p = (d_state.data_ptr(), 2, d_rows.data_ptr())
        before = d_state.cpu().numpy().tobytes()
        for call, msg in ((lambda: L.ffgpu_exec_heat(ex.h, 2, two, 2, cs, *p, None), "which = 2"),
                          (lambda: L.ffgpu_exec_heat(ex.h, 1, two, 2, cs, *p, None), "no ffgpu_exec_merge_tiles has run"),
                          (lambda: L.ffgpu_exec_heat(ex.h, 0, two, 1, cs, *p, None), "1 targets for an executor of batch 2"),
                          (lambda: L.ffgpu_exec_heat(ex.h, 0, two, 2, cs, *p, torch.cuda.Stream().cuda_stream), "stream of the forward"),
                          (lambda: L.ffgpu_exec_heat(ex.h, 0, None, 2, cs, *p, None), "NULL streams"),
                          (lambda: L.ffgpu_exec_heat(ex.h, 0, two, 2, cs, p[0], p[1], None, None), "NULL rows"),
                          (lambda: L.ffgpu_exec_heat(ex.h, 0, (C.c_int * 2)(0, 2), 2, cs, *p, None), "target 1: stream 2 is outside")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert d_state.cpu().numpy().tobytes() == before and d_rows.cpu().numpy().tobytes() == rows.tobytes()


def test_exec_heat_nv12(F, net, picture):
    """the same pass behind an NV12 forward, FFGPU_HEAT_BOX, and the map blended into the NV12 frames"""
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    h, w = picture.shape[:2]
    Y, UV = bgr_to_nv12(picture)
    py, puv = w + 3, 2 * ((w + 1) // 2) + 4
    oy, ouv = 1, (1 + py * h + 1) & ~1
    start = np.random.default_rng(7800).integers(0, 256, ouv + puv * ((h + 1) // 2) + 64, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(start[oy:], shape=(h, w), strides=(py, 1), writeable=True)[...] = Y
    np.lib.stride_tricks.as_strided(start[ouv:], shape=UV.shape, strides=(puv, 1), writeable=True)[...] = UV
    dev = torch.from_numpy(start.copy()).cuda()
    assert dev.data_ptr() % 2 == 0
    frame = (dev.data_ptr() + oy, dev.data_ptr() + ouv, w, h, py, puv)
    hs = heatref.Spec(20, 14, 5, heatref.BOX, 0, 0, 3, 0, 0.25)
    bs = heatref.BlendSpec(20, 14, 5, 6, 1, 200, False, False)
    with net.executor(1) as ex:
        ex.forward_nv12_frames_dev([frame])
        dets, boxes = ex.read_dets(), [ex.read_boxes(0)]
        S = ex.cand_capacity
        d_state = torch.zeros(heatref.state_nbytes(1, 20, 14), dtype=torch.uint8, device="cuda")
        d_rows = torch.full((4 * heatref.ROW,), 0xA5, dtype=torch.uint8, device="cuda")
        ex.heat([0], c_spec(F, hs), d_state.data_ptr(), 1, d_rows.data_ptr())
        ex.heat([0], c_spec(F, hs), d_state.data_ptr(), 1, d_rows.data_ptr())
        F.heat_blend_nv12_dev(d_state.data_ptr(), 1, [0], [frame], c_blend(F, bs))
        torch.cuda.synchronize()
        state = heatref.State(1, 20, 14)
        for _ in range(2):
            rows = heatref.accumulate(dets, flat_of(boxes, S), S, None, [0], hs, state)
        assert len(boxes[0]) >= 2 and int(rows[0, 0]) >= 2 and int(rows[0, 3]) == 1 and int(rows[0, 4]) >= 6
        assert d_rows.cpu().numpy().tobytes() == rows.tobytes() and d_state.cpu().numpy().tobytes() == state.tobytes()
        want = start.copy()
        heatref.blend_nv12(want, oy, ouv, w, h, py, puv, state.hdr[0], state.cells[0], bs)
        assert (want != start).sum() > 1000
        differ("nv12 frame", dev.cpu().numpy(), want)
        assert ex.read_dets().tobytes() == dets.tobytes() and ex.read_boxes(0).tobytes() == boxes[0].tobytes()


def test_exec_heat_merged(F, net, picture):
    """2 pictures x 2 tiles: forward, merge, ffgpu_exec_heat (MERGED) on the merged lists, one stream per picture; records and lists are what they were"""
    import torch
    h, w = picture.shape[:2]
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    pics = np.stack([wide, np.ascontiguousarray(wide[::-1])])
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    dev = torch.from_numpy(pics).cuda()
    p = 3 * 1280
    frames, tiles = [], []
    for g in range(2):
        for x0, y0, tw, th in plan:
            frames.append((dev.data_ptr() + g * h * p + y0 * p + 3 * x0, tw, th, p))
            tiles.append((g, x0, y0))
    hs = heatref.Spec(80, 27, 4, heatref.ANCHOR, 0, 1, 65536, 4, 0.25)
    with net.executor(4) as ex:
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 2)
        merged, lists = ex.read_merged(2), [ex.read_merged_boxes(g) for g in range(2)]
        assert all(len(b) >= 2 for b in lists)
        S = 2 * ex.cand_capacity                                                      # a picture's merged list has room for its tiles' boxes
        d_state = torch.zeros(heatref.state_nbytes(2, 80, 27), dtype=torch.uint8, device="cuda")
        d_rows = torch.full((4 * 2 * heatref.ROW,), 0xA5, dtype=torch.uint8, device="cuda")
        ex.heat([0, 1], c_spec(F, hs), d_state.data_ptr(), 2, d_rows.data_ptr(), which=F.HEAT_MERGED)
        torch.cuda.synchronize()
        state = heatref.State(2, 80, 27)
        rows = heatref.accumulate(merged, flat_of(lists, S), S, None, [0, 1], hs, state)
        assert int(rows[:, 0].min()) >= 2 and d_rows.cpu().numpy().tobytes() == rows.tobytes() and d_state.cpu().numpy().tobytes() == state.tobytes()
        assert ex.read_merged(2).tobytes() == merged.tobytes() and all(ex.read_merged_boxes(g).tobytes() == lists[g].tobytes() for g in range(2)) and ex.graph_captures == 1
