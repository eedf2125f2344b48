"""Outlines on the device: ffgpu_draw_segments_bgr_dev / _nv12_dev (the segment primitive, on seeded items and surfaces), ffgpu_outline_scene_dev (the
composer, on the zones fuzz's scenes with random state and events) and the chain forward -> ffgpu_exec_track -> ffgpu_exec_zones ->
ffgpu_outline_scene_dev -> ffgpu_draw_segments_*_dev on the real net, against tests/outlines/lineref.py, the numpy restatement of the contract in
include/ffcnn_hip.h.  Surfaces and items lie in arenas of seeded random bytes with 64 guard bytes around each; the WHOLE arena is compared byte for
byte, so every byte that is not to be written must have stayed: row padding, unwritten pixels, the items, the memory in front of and behind a surface.
The seeded cases are built on the CPU once (tests/outlines/fuzzcases.py) and shared by the tests; tests/test_outlines_abi.py holds the conditions that
keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from outlines import fuzzcases, lineref
from tracks import trackref
from zones import zoneref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ITEM, GUARD = lineref.ITEM_DTYPE, fuzzcases.GUARD
BOX, DETS = zoneref.BOX_DTYPE, zoneref.DETS_DTYPE


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def c_spec(F, sp):
    f = sp.flags
    return F.outline_spec(bool(f & 1), bool(f & 2), bool(f & 4), bool(f & 8), bool(f & 16), sp.thickness, sp.line_dash, sp.marker, sp.color, sp.alarm, sp.palette)


def differ(what, got, want):
    bad = np.nonzero(got != want)[0]
    if len(bad):
        pytest.fail("%s: %d bytes differ, first at %d: got %d, want %d" % (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]]), pytrace=False)


# ---------------------------------------------------------------------------------------------------------------- the primitive
def run_segments(F, c):
    """the case on the device, the items where they lie in the arena; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    fn = F.draw_segments_nv12_dev if c.nv12 else F.draw_segments_bgr_dev
    fn(base + c.items_off, c.stride, c.descs(base))
    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.SEG_NAMES)
@pytest.mark.parametrize("nv12", [False, True], ids=["bgr", "nv12"])
def test_draw_segments(F, nv12, name):
    """one call: the whole arena against lineref; the same call again from the same bytes: the same bytes"""
    c = fuzzcases.seg_cases(nv12)[name]
    got = run_segments(F, c)
    differ("%s %s" % ("nv12" if nv12 else "bgr", name), got, c.want())
    assert run_segments(F, c).tobytes() == got.tobytes(), "two runs differ"


def test_draw_segments_rejections(F):
    """every rejected argument with its message, the target's index where there is one; nothing is written"""
    import torch
    c, nv = fuzzcases.seg_cases(False)["overlap"], fuzzcases.seg_cases(True)["overlap"]
    arena = np.zeros(max(len(c.start), len(nv.start)), np.uint8)                       # (room for either case's surfaces)
    arena[:len(c.start)] = c.start
    dev = torch.from_numpy(arena.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    it = base + c.items_off
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
    for args, msg in (((None, c.stride, good, n), "NULL items"), ((it, c.stride, None, n), "NULL targets"), ((it + 2, c.stride, good, n), "4-byte aligned"),
                      ((it, c.stride, good, 0), "0 targets"), ((it, c.stride, good, -3), "-3 targets"), ((it, 0, good, n), "items_stride 0 is outside 1..512"),
                      ((it, 513, good, n), "items_stride 513 is outside 1..512"), ((it, c.stride, table(2, w=0), n), "target 2: bad size"),
                      ((it, c.stride, table(3, reserved=1), n), "target 3: reserved"), ((it, c.stride, table(1, pitch=5), n), "target 1: pitch 5 is below")):
        assert L.ffgpu_draw_segments_bgr_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())
    for args, msg in (((None, nv.stride, good_nv, n), "NULL items"), ((it, nv.stride, table_nv(4, pitch_uv=3), n), "target 4: pitch_uv 3"),
                      ((it, nv.stride, table_nv(0, matrix=9), n), "target 0: matrix 9"), ((it, nv.stride, table_nv(5, uv=base + 1), n), "target 5: the uv plane's address")):
        assert L.ffgpu_draw_segments_nv12_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == arena.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the composer
def run_scene(F, c):
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    d_scenes, d_state, d_events = to_dev(c.scenes), to_dev(c.state), to_dev(c.events)
    F.outline_scene_dev(d_scenes.data_ptr(), d_state.data_ptr(), c.nstreams, c.capacity, d_events.data_ptr(), c.events_stride, c.streams, c_spec(F, c.spec),
                        base + c.items_off, c.items_stride)
    torch.cuda.synchronize()
    assert d_state.cpu().numpy().tobytes() == c.state.tobytes() and d_events.cpu().numpy().tobytes() == c.events.tobytes()       # the inputs are only read
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.SCENE_NAMES)
def test_outline_scene(F, name):
    """the items of every target against lineref, every byte of them written and the guard bytes kept; twice: the same bytes"""
    c = fuzzcases.scene_cases()[name]
    got = run_scene(F, c)
    differ(name, got, c.want)
    assert run_scene(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("nv12", [False, True], ids=["bgr", "nv12"])
def test_composed_items_drawn_where_they_lie(F, nv12):
    """compose, then draw the device's own items, no host in between: the frames equal lineref's drawing of lineref's items (the zones fuzz's scenes lie
    in a picture of 48 x 48)"""
    import torch
    c = fuzzcases.scene_cases()["six streams"]
    w, h = 63, 47
    rng = np.random.default_rng(6250)
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
    d_scenes, d_state, d_events = to_dev(c.scenes), to_dev(c.state), to_dev(c.events)
    F.outline_scene_dev(d_scenes.data_ptr(), d_state.data_ptr(), c.nstreams, c.capacity, d_events.data_ptr(), c.events_stride, c.streams, c_spec(F, c.spec), items,
                        c.items_stride)
    want = start.copy()
    if nv12:
        F.draw_segments_nv12_dev(items, c.items_stride, [(base + t * one + GUARD, base + t * one + uv, w, h, pitch_y, pitch_uv) for t in range(c.n)])
        for t in range(c.n):
            lineref.draw_nv12(want, t * one + GUARD, t * one + uv, w, h, pitch_y, pitch_uv, c.want_items[t])
    else:
        F.draw_segments_bgr_dev(items, c.items_stride, [(base + t * one + GUARD, w, h, pitch) for t in range(c.n)])
        for t in range(c.n):
            lineref.draw_bgr(want, t * one + GUARD, w, h, pitch, c.want_items[t])
    torch.cuda.synchronize()
    assert (want != start).mean() > 0.02
    differ("frames", dev.cpu().numpy(), want)
    differ("items", d_items.cpu().numpy(), c.want)


def test_composer_rejections(F):
    """every rejected argument with its message; the items stay as they were"""
    import torch
    s = fuzzcases.scene_cases()["six streams"]
    dev = torch.from_numpy(s.start.copy()).cuda()
    items, L = dev.data_ptr() + s.items_off, F.lib()
    d_scenes, d_state, d_events = to_dev(s.scenes), to_dev(s.state), to_dev(s.events)
    streams = (C.c_int * s.n)(*s.streams)
    low = (C.c_int * s.n)(*s.streams)
    low[2] = -2

    def sp(**kw):
        p = c_spec(F, s.spec)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def scall(scenes=d_scenes.data_ptr(), state=d_state.data_ptr(), ns=s.nstreams, cap=s.capacity, evp=d_events.data_ptr(), es=s.events_stride, strm=streams, nt=s.n,
              spec=sp(), itp=items, ist=80):
        return L.ffgpu_outline_scene_dev(scenes, state, ns, cap, evp, es, strm, nt, spec, itp, ist, None)
    for kw, msg in ((dict(scenes=None), "NULL scenes"), (dict(state=None), "NULL state"), (dict(evp=None), "NULL events"), (dict(strm=None), "NULL streams"),
                    (dict(spec=None), "NULL spec"), (dict(itp=None), "NULL items"), (dict(itp=items + 2), "items must be 4-byte aligned"),
                    (dict(ist=79), "items_stride 79 is outside 80..512"), (dict(ist=513), "items_stride 513 is outside 80..512"),
                    (dict(nt=0), "0 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"), (dict(cap=0), "capacity 0"), (dict(cap=129), "capacity 129"),
                    (dict(es=63), "events_stride 63 is below FFGPU_ZONES_ROW = 64"), (dict(ns=2), r"target \d+: stream \d is outside -1 .. 1"),
                    (dict(strm=low), "target 2: stream -2"), (dict(state=d_state.data_ptr() + 2), "4-byte aligned"),
                    (dict(spec=sp(flags=0)), "name no part"), (dict(spec=sp(flags=4)), "name no part"), (dict(spec=sp(flags=32 | 1)), "unknown flags 0x21"),
                    (dict(spec=sp(flags=1 | 4)), "FFGPU_OUTLINE_TICKS without FFGPU_OUTLINE_LINES"), (dict(spec=sp(flags=2 | 16)), "FFGPU_OUTLINE_ALARM without FFGPU_OUTLINE_ZONES"),
                    (dict(spec=sp(thickness=0)), "thickness 0 is outside 1..8"), (dict(spec=sp(thickness=9)), "thickness 9 is outside 1..8"),
                    (dict(spec=sp(line_dash=-1)), "line_dash -1 is outside 0..6"), (dict(spec=sp(line_dash=7)), "line_dash 7 is outside 0..6"),
                    (dict(spec=sp(marker=-1)), "marker -1 is outside 0..32"), (dict(spec=sp(marker=33)), "marker 33 is outside 0..32"),
                    (dict(spec=sp(marker=0)), "marker 0 with FFGPU_OUTLINE_MARKERS"), (dict(spec=sp(npalette=0)), "npalette 0"), (dict(spec=sp(npalette=257)), "npalette 257"),
                    (dict(spec=sp(palette=None)), "npalette 5"), (dict(spec=sp(reserved=1)), "reserved must be 0")):
        assert scall(**kw) < 0, kw
        assert re.search(msg, F.last_error()), (msg, F.last_error())
        assert L.ffgpu_outline_spec_check(kw["spec"]) < 0 if kw.get("spec") is not None else True
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == s.start.tobytes()                            # nothing was launched
    differ("after the rejections", run_scene(F, s), s.want)                            # and the next valid call is right


# ---------------------------------------------------------------------------------------------------------------- on the real net
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


def test_outlines_behind_the_tracker_and_the_zones(F, net, picture):
    """data/test.bmp in 2 entries as one video stream: forward, ffgpu_exec_track, ffgpu_exec_zones with a scene laid round the boxes (an octagon round
    the first box's anchor, a zone over the whole picture with a dwell of one frame, which loiters in entry 1; a line through the picture and one
    running off it), then ffgpu_outline_scene_dev on the events and the state where they lie and ffgpu_draw_segments_bgr_dev into the frames and
    _nv12_dev into NV12 surfaces of another size.  The items equal lineref on what zoneref makes of the boxes and ids read back, the frames lineref's
    drawing of them; the executor's records, lists and graph stay."""
    import torch
    h, w = picture.shape[:2]
    pitch = 3 * w + 4
    buf = np.zeros((2, h, pitch), np.uint8)
    buf[:, :, :3 * w] = picture.reshape(h, 3 * w)
    dev = torch.from_numpy(buf).cuda()
    frames = [(dev.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)]
    with net.executor(2) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(2)], ex.graph_captures
        S = ex.cand_capacity
        assert len(boxes[0]) == 3 and boxes[1].tobytes() == boxes[0].tobytes()
        b0 = boxes[0][0]
        cx, cy = int((b0["x1"] + b0["x2"]) / 2), int((b0["y1"] + b0["y2"]) / 2)
        octagon = [(cx + dx, cy + dy) for dx, dy in ((-20, -48), (20, -48), (48, -20), (48, 20), (20, 48), (-20, 48), (-48, 20), (-48, -20))]
        zones_ = [(octagon,), ([(0, 0), (w, 0), (w, h), (0, h)], 1)]
        lines_ = [((-10, cy + 3), (w + 10, cy + 3)), ((cx + 31, 17), (cx - 120, h + 99))]
        scene = zoneref.make_scene(zones_, lines_)
        t_state = torch.zeros(trackref.state_nbytes(1, 16), dtype=torch.uint8, device="cuda")
        t_ids = torch.full((4 * 2 * (8 + S),), 0xA5, dtype=torch.uint8, device="cuda")
        ex.track([0, 0], F.track_spec(16, 0, 1, 1.0), t_state.data_ptr(), 1, t_ids.data_ptr())
        z_state = torch.zeros(zoneref.state_nbytes(1, 16), dtype=torch.uint8, device="cuda")
        z_ev = torch.full((4 * 2 * (zoneref.ROW + 2 * S),), 0xA5, dtype=torch.uint8, device="cuda")
        d_scene = to_dev(scene)
        spec = zoneref.Spec(16, max_missed=0, identity=zoneref.IDS)
        ex.zones([0, 0], F.zones_spec(16, 0, F.ZONES_IDS), d_scene.data_ptr(), z_state.data_ptr(), 1, z_ev.data_ptr(), t_ids.data_ptr())
        stride = 96
        ospec = lineref.Spec(fuzzcases.ALL, 2, 2, 5, alarm=(0, 0, 255), palette=[(255, 0, 0), (0, 255, 0), (0, 160, 255), (255, 255, 0)])
        d_items = torch.full((2 * stride * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        F.outline_scene_dev(d_scene.data_ptr(), z_state.data_ptr(), 1, 16, z_ev.data_ptr(), zoneref.ROW + 2 * S, [0, 0], c_spec(F, ospec), d_items.data_ptr(), stride)
        F.draw_segments_bgr_dev(d_items.data_ptr(), stride, frames)
        nw, nh = 333, 201                                                               # the same items into NV12 surfaces of another size: clipped at their edges
        rng = np.random.default_rng(6260)
        uv_off = (nw * nh + 1) & ~1                                                   # (the U V plane's address is even)
        one = uv_off + 2 * ((nw + 1) // 2) * ((nh + 1) // 2)
        start = rng.integers(0, 256, 2 * one, dtype=np.uint8)
        nv = torch.from_numpy(start.copy()).cuda()
        F.draw_segments_nv12_dev(d_items.data_ptr(), stride, [(nv.data_ptr() + t * one, nv.data_ptr() + t * one + uv_off, nw, nh) for t in range(2)])
        torch.cuda.synchronize()
        ids = t_ids.cpu().numpy().view("<i4").reshape(2, 8 + S)
        flat = np.zeros((2, S), BOX)
        for t in range(2):
            flat[t, :3] = boxes[t]
        state = zoneref.State(1, 16)
        events, _, _ = zoneref.zones(dets, flat.reshape(-1), S, None, [0, 0], spec, np.array([scene], zoneref.SCENE_DTYPE), state, ids)
        assert z_ev.cpu().numpy().tobytes() == events.tobytes() and z_state.cpu().numpy().tobytes() == state.tobytes()
        items = lineref.outline_scene(np.array([scene], zoneref.SCENE_DTYPE), np.frombuffer(state.tobytes(), np.uint8), 1, 16, events, zoneref.ROW + 2 * S, [0, 0], ospec,
                                      stride)
        assert d_items.cpu().numpy().tobytes() == items.tobytes(), "items"
        used = items["thickness"] > 0
        assert used[:, :8].all() and used[:, 8:12].all() and not used[:, 12:64].any() and used[:, 64:68].all() and not used[:, 68:80].any()
        assert used[:, 80:86].all() and not used[:, 86:].any()                        # three anchors: the state is the one after entry 1 for both targets
        assert [list(it["color"]) for it in items[:, 8]] == [[0, 255, 0, 0], [0, 0, 255, 0]]       # the whole-picture zone: loitered in entry 1: the alarm colour
        want = buf.copy().reshape(-1)
        for t in range(2):
            lineref.draw_bgr(want, t * h * pitch, w, h, pitch, items[t])
        assert (want != buf.reshape(-1)).sum() > 3000
        differ("frames", dev.cpu().numpy().reshape(-1), want)
        want = start.copy()
        for t in range(2):
            lineref.draw_nv12(want, t * one, t * one + uv_off, nw, nh, nw, 2 * ((nw + 1) // 2), items[t])
        assert (want != start).any()
        differ("nv12 frames", nv.cpu().numpy(), want)
        # the executor's own: untouched
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(2))
