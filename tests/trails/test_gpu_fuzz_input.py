"""Track trails on the device: ffgpu_trails_boxes_dev / ffgpu_trails_reset_dev (the operator, on synthetic records, lists and ids) and
ffgpu_exec_trails (behind forwards and the tracker on the real net, its items drawn by ffgpu_draw_segments_*_dev), against tests/trails/trailref.py,
the numpy restatement of the contract in include/ffcnn_hip.h.  State, rows and items lie in one arena of seeded random bytes with 64 guard bytes around
each; the WHOLE arena is compared byte for byte (every word of the family is an integer), so every byte outside the written item slots must have
stayed.  The seeded cases are built on the CPU once (tests/trails/fuzzcases.py) and shared by the tests; tests/test_trails_abi.py holds the conditions
that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from outlines import lineref
from tracks import trackref
from trails import fuzzcases, trailref
from zones import zoneref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX, DETS, GUARD = trailref.BOX_DTYPE, trailref.DETS_DTYPE, fuzzcases.GUARD
NAN, INF = float("nan"), float("inf")
PARAMS = [(cap, name) for cap in fuzzcases.CAPACITIES for name in fuzzcases.NAMES]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def c_spec(F, sp):
    return F.trails_spec(sp.capacity, sp.max_missed, sp.identity, float(sp.min_score), sp.anchor, sp.points, sp.min_move, sp.thickness, sp.coast, sp.taper,
                         sp.coast_dash, sp.color, sp.palette)


def run(F, c, splits=None):
    """the case on the device, as one call or split into several at the given record numbers; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    d_recs, d_flat = to_dev(c.recs), to_dev(c.flat)
    d_ids = None if c.ids is None else to_dev(c.ids)
    cs = c_spec(F, c.spec)
    cuts = [0] + list(splits or []) + [c.n]
    rowb = 4 * (trailref.ROW + 4 * c.stride)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == b:
            continue
        F.trails_boxes_dev(d_recs.data_ptr() + DETS.itemsize * a, d_flat.data_ptr() + (0 if c.first is not None else 24 * a * c.stride), c.stride, c.streams[a:b], cs,
                           base + c.state_off, c.nstreams, base + c.row_off + rowb * a,
                           None if d_ids is None else d_ids.data_ptr() + 4 * (8 + c.stride) * a,
                           None if c.items_off is None else base + c.items_off + 32 * c.items_stride * a, c.items_stride, c.first_item, c.nitems,
                           list_first=None if c.first is None else c.first[a:b])
    torch.cuda.synchronize()
    assert d_recs.cpu().numpy().tobytes() == c.recs.tobytes() and d_flat.cpu().numpy().tobytes() == c.flat.view(np.uint8).tobytes()      # the inputs are only read
    return dev.cpu().numpy()


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


def check(c, got, what=""):
    differ("%s %s" % (c.what, what), got, c.want, c.regions())


@pytest.mark.parametrize("cap,name", PARAMS)
def test_operator(F, cap, name):
    """one call from the case's first state: the whole arena against trailref; the same call again from the same state: the same bytes"""
    c = fuzzcases.fuzz_cases(cap)[name]
    got = run(F, c)
    check(c, got)
    assert run(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("cap,name", [(1, "ring"), (128, "ring"), (2, "streams"), (128, "records 65"), (128, "long lists"), (2, "junk state")])
def test_split_calls_leave_the_same_bytes(F, cap, name):
    """the sequence cut into several calls (the state carries the streams across) leaves what one call leaves"""
    c = fuzzcases.fuzz_cases(cap)[name]
    rng = np.random.default_rng(5760)
    for cuts in ([c.n // 2], sorted(int(v) for v in rng.integers(0, c.n + 1, 3)), list(range(1, c.n)) if c.n <= 12 else [1, c.n - 1]):
        check(c, run(F, c, cuts), "split at %s" % cuts)


def test_reset(F):
    """ffgpu_trails_reset_dev zeroes one stream or all and nothing else"""
    import torch
    c = fuzzcases.fuzz_cases(2)["streams"]
    got = run(F, c)
    nb, one = trailref.state_nbytes(6, 2), trailref.state_nbytes(1, 2)
    assert all(got[c.state_off + s * one:c.state_off + (s + 1) * one].any() for s in range(6))
    dev = torch.from_numpy(got.copy()).cuda()
    F.trails_reset_dev(dev.data_ptr() + c.state_off, 6, 2, 4)
    torch.cuda.synchronize()
    want = got.copy()
    want[c.state_off + 4 * one:c.state_off + 5 * one] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    F.trails_reset_dev(dev.data_ptr() + c.state_off, 6, 2)
    torch.cuda.synchronize()
    want[c.state_off:c.state_off + nb] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    for args, msg in (((None, 6, 2, -1), "NULL state"), ((dev.data_ptr() + 8, 6, 2, -1), "16-byte aligned"), ((dev.data_ptr(), 0, 2, -1), "0 streams"),
                      ((dev.data_ptr(), 6, 129, -1), "129 slots"), ((dev.data_ptr(), 6, 2, 6), "stream 6"), ((dev.data_ptr(), 6, 2, -2), "stream -2")):
        assert F.lib().ffgpu_trails_reset_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())


def test_operator_rejections(F):
    """every rejected argument with its message, the entry's index where there is one; the state (and everything else) stays as it was"""
    import torch
    c = fuzzcases.fuzz_cases(2)["ring"]
    before = run(F, c)
    dev = torch.from_numpy(before.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    d_recs, d_flat, d_ids = to_dev(c.recs), to_dev(c.flat), to_dev(c.ids)
    r, fl, idp_ = d_recs.data_ptr(), d_flat.data_ptr(), d_ids.data_ptr()
    st, rw, it = base + c.state_off, base + c.row_off, base + c.items_off
    n = c.n
    streams = (C.c_int * n)(*c.streams)

    def sp(**kw):
        s = c_spec(F, c.spec)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(recs=r, lists=fl, stride=c.stride, first=None, strm=streams, nt=n, spec=sp(), state=st, ns=1, idp=idp_, rows=rw, items=it, ist=c.items_stride,
             fi=c.first_item, ni=c.nitems):
        return L.ffgpu_trails_boxes_dev(recs, lists, stride, first, strm, nt, spec, state, ns, idp, rows, items, ist, fi, ni, None)
    bad_stream = (C.c_int * n)(*c.streams)
    bad_stream[4] = 1
    low_stream = (C.c_int * n)(*c.streams)
    low_stream[2] = -2
    neg_first = (C.c_int * n)(*([0] * n))
    neg_first[5] = -1
    for kw, msg in ((dict(recs=None), "NULL records"), (dict(strm=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(state=None), "NULL state"),
                    (dict(rows=None), "NULL rows"), (dict(idp=None), "NULL ids with identity FFGPU_ZONES_IDS"),
                    (dict(spec=sp(identity=trailref.TYPE)), "ids given without identity FFGPU_ZONES_IDS"),
                    (dict(spec=sp(identity=trailref.NONE), idp=None), "identity 0 is neither FFGPU_ZONES_TYPE nor _IDS"),
                    (dict(nt=0), "0 targets"), (dict(nt=-1), "-1 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"),
                    (dict(strm=bad_stream), "target 4: stream 1 is outside -1 .. 0"), (dict(strm=low_stream), "target 2: stream -2"),
                    (dict(spec=sp(capacity=0)), "capacity 0"), (dict(spec=sp(capacity=129)), "capacity 129"), (dict(spec=sp(max_missed=-1)), "max_missed -1"),
                    (dict(spec=sp(max_missed=2 ** 20 + 1)), "max_missed"), (dict(spec=sp(identity=3)), "identity 3"), (dict(spec=sp(identity=-1)), "identity -1"),
                    (dict(spec=sp(flags=4)), "unknown flags 0x4"), (dict(spec=sp(flags=-1)), "unknown flags"),
                    (dict(spec=sp(min_score=NAN)), "min_score"), (dict(spec=sp(min_score=INF)), "min_score"), (dict(spec=sp(min_score=-1.0)), "min_score"),
                    (dict(spec=sp(anchor=2)), "anchor 2 is neither 0 nor 1"), (dict(spec=sp(points=1)), "points 1 is outside 2..32"),
                    (dict(spec=sp(points=33)), "points 33 is outside 2..32"), (dict(spec=sp(min_move=-1)), "min_move -1"), (dict(spec=sp(min_move=2 ** 20 + 1)), "min_move"),
                    (dict(spec=sp(thickness=0)), "thickness 0 is outside 1..8"), (dict(spec=sp(thickness=9)), "thickness 9 is outside 1..8"),
                    (dict(spec=sp(coast_dash=-1)), "coast_dash -1"), (dict(spec=sp(coast_dash=7)), "coast_dash 7 is outside 0..6"),
                    (dict(spec=sp(npalette=0)), "npalette 0"), (dict(spec=sp(npalette=257)), "npalette 257"), (dict(spec=sp(palette=None)), "npalette 5"),
                    (dict(spec=sp(reserved=1)), "reserved must be 0"), (dict(spec=sp(reserved0=1)), "reserved must be 0"),
                    (dict(state=st + 8), "the state must be 16-byte aligned"),
                    (dict(stride=0), "bad list_stride 0"), (dict(stride=2 ** 24 + 1), "bad list_stride"), (dict(first=neg_first), "target 5: negative list start -1"),
                    (dict(items=None), "NULL items with items_stride %d, first_item 2, nitems 64" % c.items_stride),
                    (dict(items=None, ist=0, fi=0, ni=1), "NULL items with items_stride 0, first_item 0, nitems 1"),
                    (dict(items=it + 2), "the items must be 4-byte aligned"), (dict(ist=0), "items_stride 0 is outside 1..512"),
                    (dict(ist=513), "items_stride 513 is outside 1..512"), (dict(fi=-1), "negative first_item -1"), (dict(ni=0), "nitems 0"),
                    (dict(ni=c.items_stride - 1), "lie outside a row of items_stride %d" % c.items_stride)):
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == before.tobytes()                            # nothing was launched: the state, too, is as it was
    check(c, run(F, c), "after the rejections")                                       # and the next valid call is right


# ---------------------------------------------------------------------------------------------------------------- on the real net
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


@pytest.mark.parametrize("behind_outline", [False, True])
def test_trails_behind_the_tracker_drawn_into_the_frames(F, net, picture, behind_outline):
    """data/test.bmp in 2 entries as two video streams over three forwards, the picture shifted by 6 pixels per forward (to the right in stream 0, to
    the left in stream 1): forward, ffgpu_exec_track (min_hits 1: positive ids at once), ffgpu_exec_trails with the tracker's ids, and after the third
    forward ffgpu_draw_segments_bgr_dev of the device's own items into the frames and _nv12_dev into NV12 surfaces of odd sizes.  State, rows and
    items equal trailref on the boxes and ids read back after every forward, the frames lineref's drawing of trailref's items; the executor's records,
    lists and graph stay.  behind_outline: ffgpu_exec_zones and ffgpu_outline_scene_dev write the item rows first (markers of 16 slots), the trails
    the slots behind them."""
    import torch
    h, w = picture.shape[:2]
    pitch = 3 * w + 4
    CAP, P = 16, 4
    stride, first_item = (160, 80 + 2 * CAP) if behind_outline else (40, 0)
    nitems = stride - first_item - (8 if behind_outline else 3)                        # (slots behind the range stay, too)
    tspec = trailref.Spec(CAP, max_missed=1, identity=trailref.IDS, anchor=1, points=P, min_move=2, thickness=3, taper=True,
                          palette=[(255, 0, 0), (0, 255, 0), (0, 160, 255), (255, 255, 0)])
    with net.executor(2) as ex:
        S = ex.cand_capacity
        t_state = torch.zeros(trackref.state_nbytes(2, 16), dtype=torch.uint8, device="cuda")
        t_ids = torch.full((4 * 2 * (8 + S),), 0xA5, dtype=torch.uint8, device="cuda")
        r_state = torch.zeros(trailref.state_nbytes(2, CAP), dtype=torch.uint8, device="cuda")
        r_rows = torch.full((4 * 2 * (trailref.ROW + 4 * S),), 0xA5, dtype=torch.uint8, device="cuda")
        d_items = torch.full((2 * stride * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        want_items = np.frombuffer(d_items.cpu().numpy().tobytes(), trailref.ITEM_DTYPE).reshape(2, stride).copy()
        state = trailref.State(2, CAP)
        if behind_outline:
            scene = zoneref.make_scene([([(40, 40), (600, 40), (600, 380), (40, 380)], 1)], [((-10, 200), (w + 10, 200))])
            scenes = np.array([scene, scene], zoneref.SCENE_DTYPE)
            d_scene = to_dev(scenes)
            z_state = torch.zeros(zoneref.state_nbytes(2, CAP), dtype=torch.uint8, device="cuda")
            z_ev = torch.full((4 * 2 * (zoneref.ROW + 2 * S),), 0xA5, dtype=torch.uint8, device="cuda")
            zstate, zspec = zoneref.State(2, CAP), zoneref.Spec(CAP, max_missed=1, identity=zoneref.IDS)
            ospec = lineref.Spec(lineref.ZONES | lineref.LINES | lineref.MARKERS, 2, 2, 5, palette=[(9, 9, 250), (250, 9, 9)])
        longest = 0
        for k in range(3):
            buf = np.zeros((2, h, pitch), np.uint8)
            buf[0, :, :3 * w] = np.roll(picture, 6 * k, axis=1).reshape(h, 3 * w)
            buf[1, :, :3 * w] = np.roll(picture, -6 * k, axis=1).reshape(h, 3 * w)
            dev = torch.from_numpy(buf).cuda()
            frames = [(dev.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)]
            ex.forward_bgr_frames_dev(frames)
            dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(2)], ex.graph_captures
            ex.track([0, 1], F.track_spec(16, 1, 1, 0.2), t_state.data_ptr(), 2, t_ids.data_ptr())
            if behind_outline:
                ex.zones([0, 1], F.zones_spec(CAP, 1, F.ZONES_IDS), d_scene.data_ptr(), z_state.data_ptr(), 2, z_ev.data_ptr(), t_ids.data_ptr())
                F.outline_scene_dev(d_scene.data_ptr(), z_state.data_ptr(), 2, CAP, z_ev.data_ptr(), zoneref.ROW + 2 * S, [0, 1],
                                    F.outline_spec(True, True, False, True, False, 2, 2, 5, palette=ospec.palette), d_items.data_ptr(), stride)
            ex.trails([0, 1], c_spec(F, tspec), r_state.data_ptr(), 2, r_rows.data_ptr(), t_ids.data_ptr(), d_items.data_ptr(), stride, first_item, nitems)
            torch.cuda.synchronize()
            ids = t_ids.cpu().numpy().view("<i4").reshape(2, 8 + S)
            flat = np.zeros((2, S), BOX)
            for t in range(2):
                assert len(boxes[t]) >= 2
                flat[t, :len(boxes[t])] = boxes[t]
            rows, items = trailref.trails(dets, flat.reshape(-1), S, None, [0, 1], tspec, state, ids, nitems)
            if behind_outline:
                events, _, _ = zoneref.zones(dets, flat.reshape(-1), S, None, [0, 1], zspec, scenes, zstate, ids)
                want_items[:] = lineref.outline_scene(scenes, np.frombuffer(zstate.tobytes(), np.uint8), 2, CAP, events, zoneref.ROW + 2 * S, [0, 1], ospec, stride)
            want_items[:, first_item:first_item + nitems] = items
            assert r_rows.cpu().numpy().tobytes() == rows.tobytes(), "rows of forward %d" % k
            assert r_state.cpu().numpy().tobytes() == state.tobytes(), "state after forward %d" % k
            differ("items of forward %d" % k, d_items.cpu().numpy(), want_items.view(np.uint8).reshape(-1))
            longest = max(longest, int(rows[:, trailref.ROW::4].max()))
            # the executor's own: untouched
            assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(2))
        assert longest == 3 and int(rows[:, 11].min()) >= 2                           # somebody was followed through all three forwards; both streams draw trails
        F.draw_segments_bgr_dev(d_items.data_ptr(), stride, frames)
        nw, nh = 639, 423                                                               # the same items into NV12 surfaces of odd sizes
        rng = np.random.default_rng(5770)
        uv_off = (nw * nh + 1) & ~1                                                   # (the U V plane's address is even)
        one = uv_off + 2 * ((nw + 1) // 2) * ((nh + 1) // 2)
        start = rng.integers(0, 256, 2 * one, dtype=np.uint8)
        nv = torch.from_numpy(start.copy()).cuda()
        F.draw_segments_nv12_dev(d_items.data_ptr(), stride, [(nv.data_ptr() + t * one, nv.data_ptr() + t * one + uv_off, nw, nh) for t in range(2)])
        torch.cuda.synchronize()
        want = buf.copy().reshape(-1)
        trail_only = buf.copy().reshape(-1)
        for t in range(2):
            lineref.draw_bgr(want, t * h * pitch, w, h, pitch, want_items[t])
            lineref.draw_bgr(trail_only, t * h * pitch, w, h, pitch, want_items[t, first_item:first_item + nitems])
        assert (trail_only != buf.reshape(-1)).sum() > 100                            # the trails themselves show
        differ("frames", dev.cpu().numpy().reshape(-1), want)
        want = start.copy()
        for t in range(2):
            lineref.draw_nv12(want, t * one, t * one + uv_off, nw, nh, nw, 2 * ((nw + 1) // 2), want_items[t])
        assert (want != start).any()
        differ("nv12 frames", nv.cpu().numpy(), want)
        # rejected: the executor and the state stay usable
        L, cs = F.lib(), c_spec(F, tspec)
        two = (C.c_int * 2)(0, 1)
        p = (r_state.data_ptr(), 2, t_ids.data_ptr(), r_rows.data_ptr(), d_items.data_ptr(), stride, first_item, nitems)
        before = r_state.cpu().numpy().tobytes()
        for call, msg in ((lambda: L.ffgpu_exec_trails(ex.h, 2, two, 2, cs, *p, None), "which = 2"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 1, two, 2, cs, *p, None), "no ffgpu_exec_merge_tiles has run"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 0, two, 1, cs, *p, None), "1 targets for an executor of batch 2"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 0, two, 2, cs, *p, torch.cuda.Stream().cuda_stream), "stream of the forward"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 0, None, 2, cs, *p, None), "NULL streams"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 0, two, 2, cs, p[0], p[1], None, *p[3:], None), "NULL ids"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 0, two, 2, cs, *p[:7], stride + 1 - first_item, None), "lie outside a row"),
                          (lambda: L.ffgpu_exec_trails(ex.h, 0, (C.c_int * 2)(0, 2), 2, cs, *p, None), "target 1: stream 2 is outside")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert r_state.cpu().numpy().tobytes() == before and r_rows.cpu().numpy().tobytes() == rows.tobytes()
