"""Zones and lines on the device: ffgpu_zones_boxes_dev / ffgpu_zones_reset_dev (the operator, on synthetic records, lists, ids and scenes) and
ffgpu_exec_zones (behind a forward and the tracker on the real net), against tests/zones/zoneref.py, the numpy restatement of the contract in
include/ffcnn_hip.h.  State, events, gated records and gated lists lie in one arena of seeded random bytes with 64 guard bytes around each; the WHOLE
arena is compared byte for byte -- the fp32 words a NaN can reach (a slot's px, py; the gated boxes) as a NaN pattern, as tests/tracks does -- and every
other byte must have stayed.  The seeded cases are built on the CPU once (tests/zones/fuzzcases.py) and shared by the tests; tests/test_zones_abi.py
holds the conditions that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from redact import redactref
from tracks import trackref
from zones import fuzzcases, zoneref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX, DETS, GUARD = zoneref.BOX_DTYPE, zoneref.DETS_DTYPE, fuzzcases.GUARD
F32 = np.float32
NAN, INF = float("nan"), float("inf")
PARAMS = [(cap, name) for cap in fuzzcases.CAPACITIES for name in fuzzcases.NAMES]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def c_spec(F, sp):
    return F.zones_spec(sp.capacity, sp.max_missed, sp.identity, float(sp.min_score), sp.gate_zone, sp.gate_line, sp.invert)


def run(F, c, splits=None):
    """the case on the device, as one call or split into several at the given record numbers; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    d_recs, d_scenes = to_dev(c.recs), to_dev(c.scenes)
    d_flat = None if c.flat is None else to_dev(c.flat)
    d_ids = None if c.ids is None else to_dev(c.ids)
    cs = c_spec(F, c.spec)
    cuts = [0] + list(splits or []) + [c.n]
    rowb = 4 * (zoneref.ROW + 2 * c.stride)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == b:
            continue
        lists_ptr = None if d_flat is None else d_flat.data_ptr() + (0 if c.first is not None else 24 * a * c.stride)
        F.zones_boxes_dev(d_recs.data_ptr() + DETS.itemsize * a, lists_ptr, 0 if d_flat is None else c.stride, c.streams[a:b], cs, d_scenes.data_ptr(),
                          base + c.state_off, c.nstreams, base + c.ev_off + rowb * a,
                          None if d_ids is None else d_ids.data_ptr() + 4 * (8 + c.stride) * a,
                          None if c.rec_off is None else base + c.rec_off + DETS.itemsize * a,
                          None if c.list_off is None else base + c.list_off + 24 * a * c.stride,
                          list_first=None if c.first is None else c.first[a:b])
    torch.cuda.synchronize()
    assert d_recs.cpu().numpy().tobytes() == c.recs.tobytes() and d_scenes.cpu().numpy().tobytes() == c.scenes.tobytes()      # the inputs are only read
    return dev.cpu().numpy()


def check(c, got, what=""):
    bad = got != c.want
    fw = c.float_words()                                                               # NaN as NaN, not by payload
    n4 = len(got) // 4 * 4
    both = np.zeros(len(got), bool)
    both[:n4] = np.repeat(np.isnan(got[:n4].view(F32)) & np.isnan(c.want[:n4].view(F32)), 4)
    bad &= ~(both & fw)
    if not bad.any():
        return
    idx = np.nonzero(bad)[0]
    for name, lo, nb in c.regions():
        hit = idx[(idx >= lo - GUARD) & (idx < lo + nb + GUARD)]
        if len(hit):
            pytest.fail("%s %s: %s: %d bytes differ, first at region offset %d (region of %d bytes): got %d, want %d"
                        % (c.what, what, name, len(hit), int(hit[0]) - lo, nb, got[hit[0]], c.want[hit[0]]), pytrace=False)
    pytest.fail("%s %s: %d bytes differ outside every region, first at %d" % (c.what, what, len(idx), int(idx[0])), pytrace=False)


def test_arena_offsets_are_word_aligned():
    """check() reads the arena as fp32 words from its start: every region starts on a word"""
    for cap in fuzzcases.CAPACITIES:
        for c in fuzzcases.fuzz_cases(cap).values():
            assert all(lo % 4 == 0 and nb % 4 == 0 for _, lo, nb in c.regions())


@pytest.mark.parametrize("cap,name", PARAMS)
def test_operator(F, cap, name):
    """one call from the empty state: the whole arena against zoneref; the same call again from the same state: the same bytes"""
    c = fuzzcases.fuzz_cases(cap)[name]
    got = run(F, c)
    check(c, got)
    assert run(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("cap,name", [(1, "frames"), (128, "frames"), (2, "streams"), (128, "records 131"), (2, "own boxes"), (128, "clamped lists")])
def test_split_calls_leave_the_same_bytes(F, cap, name):
    """the sequence cut into several calls (the state carries the streams across) leaves what one call leaves"""
    c = fuzzcases.fuzz_cases(cap)[name]
    rng = np.random.default_rng(5660)
    for cuts in ([c.n // 2], sorted(int(v) for v in rng.integers(0, c.n + 1, 3)), list(range(1, c.n)) if c.n <= 12 else [1, c.n - 1]):
        check(c, run(F, c, cuts), "split at %s" % cuts)


def test_reset(F):
    """ffgpu_zones_reset_dev zeroes one stream or all and nothing else"""
    import torch
    c = fuzzcases.fuzz_cases(2)["records 131"]
    got = run(F, c)
    nb, one = zoneref.state_nbytes(3, 2), zoneref.state_nbytes(1, 2)
    assert got[c.state_off:c.state_off + nb].any()
    dev = torch.from_numpy(got.copy()).cuda()
    F.zones_reset_dev(dev.data_ptr() + c.state_off, 3, 2, 1)
    torch.cuda.synchronize()
    want = got.copy()
    want[c.state_off + one:c.state_off + 2 * one] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    F.zones_reset_dev(dev.data_ptr() + c.state_off, 3, 2)
    torch.cuda.synchronize()
    want[c.state_off:c.state_off + nb] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    for args, msg in (((None, 3, 2, -1), "NULL state"), ((dev.data_ptr() + 8, 3, 2, -1), "16-byte aligned"), ((dev.data_ptr(), 0, 2, -1), "0 streams"),
                      ((dev.data_ptr(), 3, 129, -1), "129 slots"), ((dev.data_ptr(), 3, 2, 3), "stream 3"), ((dev.data_ptr(), 3, 2, -2), "stream -2")):
        assert F.lib().ffgpu_zones_reset_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())


def test_operator_rejections(F):
    """every rejected argument with its message, the entry's index where there is one; the state (and everything else) stays as it was"""
    import torch
    c = fuzzcases.fuzz_cases(2)["records 131"]
    before = run(F, c)
    dev = torch.from_numpy(before.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    d_recs, d_flat, d_ids, d_scenes = to_dev(c.recs), to_dev(c.flat), to_dev(c.ids), to_dev(c.scenes)
    r, fl, idp_, scp = d_recs.data_ptr(), d_flat.data_ptr(), d_ids.data_ptr(), d_scenes.data_ptr()
    st, ev, orec, ol = base + c.state_off, base + c.ev_off, base + c.rec_off, base + c.list_off
    n = c.n
    streams = (C.c_int * n)(*c.streams)

    def sp(**kw):
        s = c_spec(F, c.spec)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(recs=r, lists=fl, stride=c.stride, first=None, strm=streams, nt=n, spec=sp(), scenes=scp, state=st, ns=3, idp=idp_, evp=ev, orp=orec, olp=ol):
        return L.ffgpu_zones_boxes_dev(recs, lists, stride, first, strm, nt, spec, scenes, state, ns, idp, evp, orp, olp, None)
    bad_stream = (C.c_int * n)(*c.streams)
    bad_stream[4] = 3
    low_stream = (C.c_int * n)(*c.streams)
    low_stream[2] = -2
    neg_first = (C.c_int * n)(*([0] * n))
    neg_first[5] = -1
    for kw, msg in ((dict(recs=None), "NULL records"), (dict(strm=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(scenes=None), "NULL scenes"),
                    (dict(state=None), "NULL state"), (dict(evp=None), "NULL events"), (dict(idp=None), "NULL ids with identity FFGPU_ZONES_IDS"),
                    (dict(spec=sp(identity=zoneref.NONE)), "ids given without identity FFGPU_ZONES_IDS"),
                    (dict(spec=sp(identity=zoneref.TYPE)), "ids given without identity FFGPU_ZONES_IDS"),
                    (dict(nt=0), "0 targets"), (dict(nt=-1), "-1 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"),
                    (dict(strm=bad_stream), "target 4: stream 3 is outside -1 .. 2"), (dict(strm=low_stream), "target 2: stream -2"),
                    (dict(ns=2), r"target \d+: stream 2 is outside -1 .. 1"),
                    (dict(spec=sp(capacity=0)), "capacity 0"), (dict(spec=sp(capacity=129)), "capacity 129"), (dict(spec=sp(max_missed=-1)), "max_missed -1"),
                    (dict(spec=sp(max_missed=2 ** 20 + 1)), "max_missed"), (dict(spec=sp(identity=3)), "identity 3"), (dict(spec=sp(identity=-1)), "identity -1"),
                    (dict(spec=sp(flags=2)), "unknown flags 0x2"), (dict(spec=sp(flags=-1)), "unknown flags"),
                    (dict(spec=sp(min_score=NAN)), "min_score"), (dict(spec=sp(min_score=INF)), "min_score"), (dict(spec=sp(min_score=-1.0)), "min_score"),
                    (dict(spec=sp(reserved=1)), "reserved"), (dict(state=st + 8), "16-byte aligned"), (dict(scenes=scp + 2), "4-byte aligned"),
                    (dict(stride=0), "bad list_stride 0"), (dict(stride=2 ** 24 + 1), "bad list_stride"),
                    (dict(first=neg_first), "target 5: negative list start -1"), (dict(orp=None), "d_out_lists without d_out_records")):
        assert call(**kw) < 0, kw
        assert re.search(msg, F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == before.tobytes()                            # nothing was launched: the state, too, is as it was
    check(c, run(F, c), "after the rejections")                                       # and the next valid call is right


# ---------------------------------------------------------------------------------------------------------------- on an executor
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_zones_behind_the_tracker_and_redact_of_the_gated_record(F, net, picture, flags):
    """data/test.bmp in 2 entries as one video stream (flags 32: FFGPU_SPLIT2): forward, ffgpu_exec_track (min_hits 1: positive ids at once),
    ffgpu_exec_zones with the tracker's ids, then the gated record redacted.  A zone is laid round the first box's anchor, a second one over the whole
    picture with a dwell of one frame, and the gate selects the first.  The events equal zoneref on the boxes and ids read back; the executor's
    records, lists and graph stay; the redacted bytes equal redactref on the gated record zoneref predicts."""
    import torch
    h, w = picture.shape[:2]
    pitch = 3 * w + 4
    buf = np.zeros((h, pitch), np.uint8)
    buf[:, :3 * w] = picture.reshape(h, 3 * w)
    dev = torch.from_numpy(buf).cuda()
    frames = [(dev.data_ptr(), w, h, pitch)] * 2
    with net.executor(2, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(2)], ex.graph_captures
        S = ex.cand_capacity
        assert len(boxes[0]) == 3 and boxes[1].tobytes() == boxes[0].tobytes()
        b0 = boxes[0][0]
        cx, cy = int((b0["x1"] + b0["x2"]) / 2), int((b0["y1"] + b0["y2"]) / 2)
        zones_ = [([(cx - 6, cy - 6), (cx + 6, cy - 6), (cx + 6, cy + 6), (cx - 6, cy + 6)],), ([(0, 0), (w, 0), (w, h), (0, h)], 1)]
        lines_ = [((-10, cy + 3), (w + 10, cy + 3))]
        scene = zoneref.make_scene(zones_, lines_)
        cscene = F.scene([tuple(z) for z in zones_], lines_)
        F.scene_check([cscene])
        assert F.scenes_bytes([cscene]) == scene.tobytes()
        t_state = torch.zeros(trackref.state_nbytes(1, 16), dtype=torch.uint8, device="cuda")
        t_ids = torch.full((4 * 2 * (8 + S),), 0xA5, dtype=torch.uint8, device="cuda")
        ex.track([0, 0], F.track_spec(16, 0, 1, 1.0), t_state.data_ptr(), 1, t_ids.data_ptr())
        z_state = torch.zeros(zoneref.state_nbytes(1, 16), dtype=torch.uint8, device="cuda")
        z_ev = torch.full((4 * 2 * (zoneref.ROW + 2 * S),), 0xA5, dtype=torch.uint8, device="cuda")
        z_recs = torch.full((DETS.itemsize * 2,), 0xA5, dtype=torch.uint8, device="cuda")
        z_lists = torch.full((24 * 2 * S,), 0xA5, dtype=torch.uint8, device="cuda")
        d_scene = to_dev(scene)
        spec = zoneref.Spec(16, max_missed=0, identity=zoneref.IDS, gate_zone=1)
        ex.zones([0, 0], c_spec(F, spec), d_scene.data_ptr(), z_state.data_ptr(), 1, z_ev.data_ptr(), t_ids.data_ptr(), z_recs.data_ptr(), z_lists.data_ptr())
        torch.cuda.synchronize()
        ids = t_ids.cpu().numpy().view("<i4").reshape(2, 8 + S)
        assert [int(v) for v in ids[0, 8:11]] == [1, 2, 3] and [int(v) for v in ids[1, 8:11]] == [1, 2, 3]
        flat = np.zeros((2, S), BOX)
        for t in range(2):
            flat[t, :3] = boxes[t]
        state = zoneref.State(1, 16)
        events, orecs, olists = zoneref.zones(dets, flat.reshape(-1), S, None, [0, 0], spec, np.array([scene], zoneref.SCENE_DTYPE), state, ids)
        assert z_ev.cpu().numpy().tobytes() == events.tobytes(), "events"
        assert z_state.cpu().numpy().tobytes() == state.tobytes(), "state"
        assert z_recs.cpu().numpy().tobytes() == orecs.tobytes() and z_lists.cpu().numpy().tobytes() == olists.tobytes(), "gated record"
        # what the scene was laid out for: box 0 inside zone 0 and nobody else; everybody inside zone 1: fresh and entered in entry 0, known and
        # loitering in entry 1; identical frames cross nothing
        assert [int(v) for v in events[0, :10]] == [3, 0, 3, 0, 0, 0, 0, 0, 3, 0] and [int(v) for v in events[1, :10]] == [3, 3, 0, 0, 0, 0, 0, 0, 3, 1]
        assert [int(v) for v in events[0, 16:24]] == [1, 1, 0, 0, 3, 3, 0, 0] and [int(v) for v in events[1, 16:24]] == [1, 0, 0, 0, 3, 0, 0, 3]
        assert not events[:, 48:64].any() and [int(r["nfull"]) for r in orecs] == [1, 1] and orecs[0]["box"][0].tobytes() == boxes[0][0].tobytes()
        # the executor's own: untouched
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(2))
        # the gated record redacted: ffgpu_exec_redact_bgr reads the EXECUTOR's records, so the caller's gated record goes through the operator form
        rng = np.random.default_rng(5670)
        start = rng.integers(0, 256, 2 * pitch * h, dtype=np.uint8)
        out = torch.from_numpy(start.copy()).cuda()
        targets = [(out.data_ptr() + t * pitch * h, w, h, pitch) for t in range(2)]
        F.redact_boxes_bgr_dev(z_recs.data_ptr(), z_lists.data_ptr(), S, targets, F.redact_spec(F.REDACT_MOSAIC, 8, margin=(1, 8)))
        torch.cuda.synchronize()
        want = start.copy()
        rs = redactref.Spec(redactref.MOSAIC, 8, margin=(1, 8))
        for t in range(2):
            redactref.redact_bgr(want, t * pitch * h, w, h, pitch, olists[t][:int(orecs[t]["nfull"])], rs)
        assert (want != start).any() and out.cpu().numpy().tobytes() == want.tobytes()
        # rejected: the executor and the state stay usable
        L, cs = F.lib(), c_spec(F, spec)
        one = (C.c_int * 2)(0, 0)
        p = (d_scene.data_ptr(), z_state.data_ptr(), 1, t_ids.data_ptr(), z_ev.data_ptr(), z_recs.data_ptr(), z_lists.data_ptr())
        before = z_state.cpu().numpy().tobytes()
        for call, msg in ((lambda: L.ffgpu_exec_zones(ex.h, 2, one, 2, cs, *p, None), "which = 2"),
                          (lambda: L.ffgpu_exec_zones(ex.h, 1, one, 2, cs, *p, None), "no ffgpu_exec_merge_tiles has run"),
                          (lambda: L.ffgpu_exec_zones(ex.h, 0, one, 1, cs, *p, None), "1 targets for an executor of batch 2"),
                          (lambda: L.ffgpu_exec_zones(ex.h, 0, one, 2, cs, *p, torch.cuda.Stream().cuda_stream), "stream of the forward"),
                          (lambda: L.ffgpu_exec_zones(ex.h, 0, None, 2, cs, *p, None), "NULL streams"),
                          (lambda: L.ffgpu_exec_zones(ex.h, 0, one, 2, cs, p[0], p[1], 1, None, *p[4:], None), "NULL ids"),
                          (lambda: L.ffgpu_exec_zones(ex.h, 0, (C.c_int * 2)(0, 1), 2, cs, *p, None), "target 1: stream 1 is outside")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert z_state.cpu().numpy().tobytes() == before and z_ev.cpu().numpy().tobytes() == events.tobytes()
