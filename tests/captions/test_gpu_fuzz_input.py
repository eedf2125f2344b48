"""Captions on the device: ffgpu_draw_text_bgr_dev / _nv12_dev (the rasteriser, on seeded items and surfaces), ffgpu_caption_boxes_dev and
ffgpu_caption_scene_dev (the composers, on synthetic records, lists, ids, scenes, state and events) and ffgpu_exec_caption_bgr / _nv12 (behind a
forward and the tracker on the real net), against tests/captions/textref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  Surfaces and
items lie in arenas of seeded random bytes with 64 guard bytes around each; the WHOLE arena is compared byte for byte, so every byte that is not to be
written must have stayed: row padding, unwritten pixels, the memory in front of and behind a surface.  The seeded cases are built on the CPU once
(tests/captions/fuzzcases.py) and shared by the tests; tests/test_captions_abi.py holds the conditions that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from captions import fuzzcases, textref
from tracks import trackref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX, DETS, ITEM, GUARD = textref.BOX_DTYPE, textref.DETS_DTYPE, textref.ITEM_DTYPE, fuzzcases.GUARD
NAN, INF = float("nan"), float("inf")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def c_spec(F, sp, d_names=None):
    return F.caption_spec(bool(sp.flags & 1), bool(sp.flags & 2), bool(sp.flags & 4), bool(sp.flags & 8), float(sp.min_score), sp.identity, sp.scale, sp.fg,
                          sp.color, sp.palette, None if sp.names is None else d_names, 0 if sp.names is None else len(sp.names))


def differ(what, got, want):
    bad = np.nonzero(got != want)[0]
    if len(bad):
        pytest.fail("%s: %d bytes differ, first at %d: got %d, want %d" % (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]]), pytrace=False)


# ---------------------------------------------------------------------------------------------------------------- the rasteriser
def run_text(F, c):
    """the case on the device; the font, when the case has one, at an odd address; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    d_items = to_dev(c.items)
    d_font = None if c.font is None else to_dev(np.concatenate([np.zeros(1, np.uint8), c.font.reshape(-1)]))
    fn = F.draw_text_nv12_dev if c.nv12 else F.draw_text_bgr_dev
    fn(d_items.data_ptr(), c.stride, c.descs(base), None if d_font is None else d_font.data_ptr() + 1)
    torch.cuda.synchronize()
    assert d_items.cpu().numpy().tobytes() == c.items.tobytes()                        # the items are only read
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.TEXT_NAMES)
@pytest.mark.parametrize("nv12", [False, True], ids=["bgr", "nv12"])
def test_draw_text(F, nv12, name):
    """one call: the whole arena against textref; the same call again from the same bytes: the same bytes"""
    c = fuzzcases.text_cases(nv12)[name]
    want = c.want(F.font_builtin())
    got = run_text(F, c)
    differ("%s %s" % ("nv12" if nv12 else "bgr", name), got, want)
    assert run_text(F, c).tobytes() == got.tobytes(), "two runs differ"


def test_draw_text_rejections(F):
    """every rejected argument with its message, the target's index where there is one; nothing is written"""
    import torch
    c, nv = fuzzcases.text_cases(False)["overlap"], fuzzcases.text_cases(True)["overlap"]
    arena = np.zeros(max(len(c.start), len(nv.start)), np.uint8)                       # (room for either case's surfaces)
    arena[:len(c.start)] = c.start
    dev = torch.from_numpy(arena.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    d_items = to_dev(c.items)
    it = d_items.data_ptr()
    good, n = F.bgr_frame_table(c.descs(base)), c.n
    good_nv = F.nv12_frame_table(nv.descs(base))

    def table(k, **kw):
        arr = F.bgr_frame_table(c.descs(base))
        for f, v in kw.items():
            setattr(arr[k], f, v)
        return arr

    def table_nv(k, **kw):
        arr = F.nv12_frame_table(nv.descs(base))
        for f, v in kw.items():
            setattr(arr[k], f, v)
        return arr
    for args, msg in (((None, c.stride, None, good, n), "NULL items"), ((it, c.stride, None, None, n), "NULL targets"), ((it + 2, c.stride, None, good, n), "4-byte aligned"),
                      ((it, c.stride, None, good, 0), "0 targets"), ((it, c.stride, None, good, -3), "-3 targets"), ((it, 0, None, good, n), "items_stride 0 is outside 1..256"),
                      ((it, 257, None, good, n), "items_stride 257 is outside 1..256"), ((it, c.stride, None, table(2, w=0), n), "target 2: bad size"),
                      ((it, c.stride, None, table(3, reserved=1), n), "target 3: reserved"), ((it, c.stride, None, table(1, pitch=5), n), "target 1: pitch 5 is below")):
        assert L.ffgpu_draw_text_bgr_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())
    for args, msg in (((None, nv.stride, None, good_nv, n), "NULL items"), ((it, nv.stride, None, table_nv(4, pitch_uv=3), n), "target 4: pitch_uv 3"),
                      ((it, nv.stride, None, table_nv(0, matrix=9), n), "target 0: matrix 9"), ((it, nv.stride, None, table_nv(5, uv=base + 1), n), "target 5: the uv plane's address")):
        assert L.ffgpu_draw_text_nv12_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == arena.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the composers
def run_boxes(F, c):
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    d_recs = to_dev(c.recs)
    d_flat = None if c.flat is None else to_dev(c.flat)
    d_ids = None if c.ids is None else to_dev(c.ids)
    d_names = None if c.spec.names is None else to_dev(c.spec.names)
    F.caption_boxes_dev(d_recs.data_ptr(), None if d_flat is None else d_flat.data_ptr(), c.stride, c.n, c_spec(F, c.spec, None if d_names is None else d_names.data_ptr()),
                        base + c.items_off, c.items_stride, None if d_ids is None else d_ids.data_ptr(), list_first=c.first)
    torch.cuda.synchronize()
    assert d_recs.cpu().numpy().tobytes() == c.recs.tobytes()                          # the inputs are only read
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.BOX_NAMES)
def test_caption_boxes(F, name):
    """the items of every target against textref, every byte of them written and the guard bytes kept; twice: the same bytes"""
    c = fuzzcases.box_cases()[name]
    got = run_boxes(F, c)
    differ(name, got, c.want)
    assert run_boxes(F, c).tobytes() == got.tobytes(), "two runs differ"


def run_scene(F, c):
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    d_scenes, d_state, d_events = to_dev(c.scenes), to_dev(c.state), to_dev(c.events)
    F.caption_scene_dev(d_scenes.data_ptr(), d_state.data_ptr(), c.nstreams, c.capacity, d_events.data_ptr(), c.events_stride, c.streams, c_spec(F, c.spec),
                        base + c.items_off, c.items_stride)
    torch.cuda.synchronize()
    assert d_state.cpu().numpy().tobytes() == c.state.tobytes() and d_events.cpu().numpy().tobytes() == c.events.tobytes()
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.SCENE_NAMES)
def test_caption_scene(F, name):
    c = fuzzcases.scene_cases()[name]
    got = run_scene(F, c)
    differ(name, got, c.want)
    assert run_scene(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("nv12", [False, True], ids=["bgr", "nv12"])
def test_composed_items_drawn_where_they_lie(F, nv12):
    """compose, then draw the device's own items with the built-in font, no host in between: the frames equal textref's drawing of textref's items"""
    import torch
    c = fuzzcases.box_cases()["lists"]
    w, h = 199, 121
    rng = np.random.default_rng(5950)
    if nv12:
        pitch_y, pitch_uv = w + 2, 2 * ((w + 1) // 2) + 2
        uv = (GUARD + pitch_y * h + GUARD + 1) & ~1                                    # (the U V plane's address is even)
        one = (uv + pitch_uv * ((h + 1) // 2) + GUARD + 1) & ~1
    else:
        pitch = 3 * w + 1
        one = GUARD + pitch * h + GUARD
    start = rng.integers(0, 256, one * c.n, dtype=np.uint8)
    dev, d_items = torch.from_numpy(start.copy()).cuda(), to_dev(c.start)
    base, items = dev.data_ptr(), d_items.data_ptr() + c.items_off
    d_recs, d_flat, d_ids, d_names = to_dev(c.recs), to_dev(c.flat), to_dev(c.ids), to_dev(c.spec.names)
    F.caption_boxes_dev(d_recs.data_ptr(), d_flat.data_ptr(), c.stride, c.n, c_spec(F, c.spec, d_names.data_ptr()), items, c.items_stride, d_ids.data_ptr())
    want, font = start.copy(), F.font_builtin()
    if nv12:
        F.draw_text_nv12_dev(items, c.items_stride, [(base + t * one + GUARD, base + t * one + uv, w, h, pitch_y, pitch_uv) for t in range(c.n)])
        for t in range(c.n):
            textref.draw_nv12(want, t * one + GUARD, t * one + uv, w, h, pitch_y, pitch_uv, c.want_items[t], font)
    else:
        F.draw_text_bgr_dev(items, c.items_stride, [(base + t * one + GUARD, w, h, pitch) for t in range(c.n)])
        for t in range(c.n):
            textref.draw_bgr(want, t * one + GUARD, w, h, pitch, c.want_items[t], font)
    torch.cuda.synchronize()
    assert (want != start).mean() > 0.02
    differ("frames", dev.cpu().numpy(), want)
    differ("items", d_items.cpu().numpy(), c.want)


def test_composer_rejections(F):
    """every rejected argument with its message; the items stay as they were"""
    import torch
    c = fuzzcases.box_cases()["lists"]
    dev = torch.from_numpy(c.start.copy()).cuda()
    items, L = dev.data_ptr() + c.items_off, F.lib()
    d_recs, d_flat, d_ids, d_names = to_dev(c.recs), to_dev(c.flat), to_dev(c.ids), to_dev(c.spec.names)
    r, fl, idp_, nm = d_recs.data_ptr(), d_flat.data_ptr(), d_ids.data_ptr(), d_names.data_ptr()

    def sp(**kw):
        s = c_spec(F, c.spec, nm)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(recs=r, lists=fl, stride=c.stride, first=None, nt=c.n, spec=sp(), idp=idp_, itp=items, ist=c.items_stride):
        return L.ffgpu_caption_boxes_dev(recs, lists, stride, first, nt, spec, idp, itp, ist, None)
    neg_first = (C.c_int * c.n)(*([0] * c.n))
    neg_first[5] = -1
    for kw, msg in ((dict(recs=None), "NULL records"), (dict(spec=None), "NULL spec"), (dict(itp=None), "NULL items"), (dict(itp=items + 2), "items must be 4-byte aligned"),
                    (dict(nt=0), "0 targets"), (dict(nt=-1), "-1 targets"), (dict(ist=0), "items_stride 0 is outside 1..256"), (dict(ist=257), "items_stride 257"),
                    (dict(stride=0), "bad list_stride 0"), (dict(stride=2 ** 24 + 1), "bad list_stride"), (dict(first=neg_first), "target 5: negative list start -1"),
                    (dict(spec=sp(min_score=NAN)), "min_score"), (dict(spec=sp(min_score=INF)), "min_score"), (dict(spec=sp(min_score=-0.5)), "min_score"),
                    (dict(spec=sp(min_score=1.5)), "min_score"), (dict(spec=sp(flags=8)), "name no part"), (dict(spec=sp(flags=0)), "name no part"),
                    (dict(spec=sp(flags=16 | 1)), "unknown flags 0x11"), (dict(spec=sp(flags=-1)), "unknown flags"), (dict(spec=sp(identity=3)), "identity 3"),
                    (dict(spec=sp(identity=-1)), "identity -1"), (dict(spec=sp(scale=0)), "scale 0 is outside 1..4"), (dict(spec=sp(scale=5)), "scale 5 is outside 1..4"),
                    (dict(spec=sp(npalette=0)), "npalette 0"), (dict(spec=sp(npalette=257)), "npalette 257"), (dict(spec=sp(palette=None)), "npalette 7"),
                    (dict(spec=sp(nnames=-1)), "nnames -1"), (dict(spec=sp(nnames=0)), "nnames 0"), (dict(spec=sp(d_names=None)), "nnames 80"),
                    (dict(idp=None), "NULL ids with identity FFGPU_ZONES_IDS"), (dict(spec=sp(identity=textref.NONE)), "ids given without identity FFGPU_ZONES_IDS"),
                    (dict(spec=sp(identity=textref.TYPE)), "ids given without identity FFGPU_ZONES_IDS")):
        assert call(**kw) < 0, kw
        assert re.search(msg, F.last_error()), (msg, F.last_error())
    s = fuzzcases.scene_cases()["six streams"]
    d_scenes, d_state, d_events = to_dev(s.scenes), to_dev(s.state), to_dev(s.events)
    streams = (C.c_int * s.n)(*s.streams)
    low = (C.c_int * s.n)(*s.streams)
    low[2] = -2

    def scall(scenes=d_scenes.data_ptr(), state=d_state.data_ptr(), ns=s.nstreams, cap=s.capacity, evp=d_events.data_ptr(), es=s.events_stride, strm=streams, nt=s.n,
              spec=c_spec(F, s.spec), itp=items, ist=16):
        return L.ffgpu_caption_scene_dev(scenes, state, ns, cap, evp, es, strm, nt, spec, itp, ist, None)
    bad_scale = c_spec(F, s.spec)
    bad_scale.scale = 7
    for kw, msg in ((dict(scenes=None), "NULL scenes"), (dict(state=None), "NULL state"), (dict(evp=None), "NULL events"), (dict(strm=None), "NULL streams"),
                    (dict(spec=None), "NULL spec"), (dict(itp=None), "NULL items"), (dict(ist=15), "items_stride 15 is outside 16..256"), (dict(ist=257), "items_stride 257"),
                    (dict(nt=0), "0 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"), (dict(cap=0), "capacity 0"), (dict(cap=129), "capacity 129"),
                    (dict(es=63), "events_stride 63 is below FFGPU_ZONES_ROW = 64"), (dict(ns=2), r"target \d+: stream \d is outside -1 .. 1"),
                    (dict(strm=low), "target 2: stream -2"), (dict(spec=bad_scale), "scale 7"), (dict(state=d_state.data_ptr() + 2), "4-byte aligned")):
        assert scall(**kw) < 0, kw
        assert re.search(msg, F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == c.start.tobytes()                            # nothing was launched
    differ("after the rejections", run_boxes(F, c), c.want)                            # and the next valid call is right


# ---------------------------------------------------------------------------------------------------------------- on an executor
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_caption_behind_the_tracker(F, net, picture, flags):
    """data/test.bmp in 2 entries as one video stream (flags 32: FFGPU_SPLIT2): forward, ffgpu_exec_track (min_hits 2: pending ids in entry 0, positive
    ones in entry 1), ffgpu_exec_caption_bgr with the tracker's ids, names and a palette.  The items equal textref on the boxes and ids read back and
    the frames textref's drawing of them with the built-in font; the same records captioned into NV12 surfaces; the executor's records, lists and
    graph stay; rejected calls leave the executor usable."""
    import torch
    h, w = picture.shape[:2]
    pitch = 3 * w + 4
    buf = np.zeros((2, h, pitch), np.uint8)
    buf[:, :, :3 * w] = picture.reshape(h, 3 * w)
    dev = torch.from_numpy(buf).cuda()
    frames = [(dev.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)]
    names = fuzzcases.names_rows([b"class %d" % k for k in range(80)])
    d_names = to_dev(names)
    pal = [(0, 0, 255), (0, 160, 0), (255, 0, 0)]
    spec = textref.Spec(textref.NAME | textref.SCORE | textref.ID | textref.CAPTION_OPAQUE, 0.25, textref.IDS, 2, (255, 255, 255), palette=pal, names=names)
    with net.executor(2, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(2)], ex.graph_captures
        S = ex.cand_capacity
        assert len(boxes[0]) == 3 and boxes[1].tobytes() == boxes[0].tobytes()
        t_state = torch.zeros(trackref.state_nbytes(1, 16), dtype=torch.uint8, device="cuda")
        t_ids = torch.full((4 * 2 * (8 + S),), 0xA5, dtype=torch.uint8, device="cuda")
        ex.track([0, 0], F.track_spec(16, 0, 2, 0.3), t_state.data_ptr(), 1, t_ids.data_ptr())
        stride = 8
        d_items = torch.full((2 * stride * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        cs = c_spec(F, spec, d_names.data_ptr())
        ex.caption_bgr(frames, cs, d_items.data_ptr(), stride, t_ids.data_ptr())
        torch.cuda.synchronize()
        ids = t_ids.cpu().numpy().view("<i4").reshape(2, 8 + S)
        assert [int(v) for v in ids[0, 8:11]] == [-1, -2, -3] and [int(v) for v in ids[1, 8:11]] == [1, 2, 3]
        flat = np.zeros((2, S), BOX)
        for t in range(2):
            flat[t, :3] = boxes[t]
        items = textref.caption_boxes(dets, flat.reshape(-1), S, None, spec, ids, stride)
        assert d_items.cpu().numpy().tobytes() == items.tobytes(), "items"
        texts = [[bytes(it["text"][:int(it["len"])]) for it in items[t, :3]] for t in range(2)]
        assert all(re.fullmatch(rb"[a-z0-9 ]+ \d+% #" + b"%d" % (k + 1) + rb"\?", tx) for k, tx in enumerate(texts[0])), texts
        assert all(re.fullmatch(rb"[a-z0-9 ]+ \d+% #" + b"%d" % (k + 1), tx) for k, tx in enumerate(texts[1])), texts
        assert not items[:, 3:].view(np.uint8).any()
        want, font = buf.copy().reshape(-1), F.font_builtin()
        for t in range(2):
            textref.draw_bgr(want, t * h * pitch, w, h, pitch, items[t], font)
        assert (want != buf.reshape(-1)).sum() > 3000
        differ("frames", dev.cpu().numpy().reshape(-1), want)
        # the same records into NV12 surfaces of another size: the tags are clipped at their edges
        nw, nh = 333, 201
        rng = np.random.default_rng(5960)
        uv_off = (nw * nh + 1) & ~1                                                   # (the U V plane's address is even)
        one = uv_off + 2 * ((nw + 1) // 2) * ((nh + 1) // 2)
        start = rng.integers(0, 256, 2 * one, dtype=np.uint8)
        nv = torch.from_numpy(start.copy()).cuda()
        ex.caption_nv12([(nv.data_ptr() + t * one, nv.data_ptr() + t * one + uv_off, nw, nh) for t in range(2)], cs, d_items.data_ptr(), stride, t_ids.data_ptr())
        torch.cuda.synchronize()
        want = start.copy()
        for t in range(2):
            textref.draw_nv12(want, t * one, t * one + uv_off, nw, nh, nw, 2 * ((nw + 1) // 2), items[t], font)
        assert (want != start).any()
        differ("nv12 frames", nv.cpu().numpy(), want)
        assert d_items.cpu().numpy().tobytes() == items.tobytes()
        # the executor's own: untouched
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(2))
        # rejected: the executor stays usable
        L = F.lib()
        tab = F.bgr_frame_table(frames)
        bad = F.bgr_frame_table(frames)
        bad[1].w = 0
        p = (t_ids.data_ptr(), d_items.data_ptr(), stride, None)
        no_ids = c_spec(F, spec, d_names.data_ptr())
        no_ids.identity = textref.NONE
        before = dev.cpu().numpy().tobytes()
        for call, msg in ((lambda: L.ffgpu_exec_caption_bgr(ex.h, 2, tab, 2, cs, *p, None), "which = 2"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 1, tab, 2, cs, *p, None), "no ffgpu_exec_merge_tiles has run"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 1, cs, *p, None), "1 targets for an executor of batch 2"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 2, cs, *p, torch.cuda.Stream().cuda_stream), "stream of the forward"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, None, 2, cs, *p, None), "NULL targets"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 2, None, *p, None), "NULL spec"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 2, cs, None, *p[1:], None), "NULL ids"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 2, no_ids, *p, None), "ids given without identity"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 2, cs, p[0], None, stride, None, None), "NULL items"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, tab, 2, cs, p[0], p[1], 0, None, None), "items_stride 0"),
                          (lambda: L.ffgpu_exec_caption_bgr(ex.h, 0, bad, 2, cs, *p, None), "target 1: bad size")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert dev.cpu().numpy().tobytes() == before and d_items.cpu().numpy().tobytes() == items.tobytes()
        clean = torch.from_numpy(buf).cuda()                                           # (the captioned frames are another picture)
        ex.forward_bgr_frames_dev([(clean.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)])
        assert ex.read_dets()["count"].tolist() == dets["count"].tolist() and ex.read_boxes(1).tobytes() == boxes[1].tobytes()
