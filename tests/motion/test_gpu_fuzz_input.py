"""Motion maps on the device: ffgpu_motion_update_bgr_dev / _nv12_dev, ffgpu_motion_reset_dev and ffgpu_motion_gate_dev (the operators, on synthetic
frames, states, records and lists) and ffgpu_exec_motion_gate (behind a forward and behind a merge on the real net, its gated record then drawn into
the frames), against tests/motion/motionref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  State, rows, words, gated records
and the frames lie in one arena of seeded random bytes with 64 guard bytes around each; the WHOLE arena is compared byte for byte (every word of the
family is an integer), so every byte the contract leaves alone must have stayed.  The seeded cases are built on the CPU once
(tests/motion/fuzzcases.py) and shared by the tests; tests/test_motion_abi.py holds the conditions that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from motion import fuzzcases, motionref
from overlay import drawref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX, DETS, GUARD = motionref.BOX_DTYPE, motionref.DETS_DTYPE, fuzzcases.GUARD
UPDATE_PARAMS = [(fmt, name) for fmt in fuzzcases.FORMATS for name in fuzzcases.UPDATE_NAMES]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def c_spec(F, sp):
    return F.motion_spec(sp.w, sp.h, sp.cell_log2, sp.threshold, sp.learn_shift, sp.learn_shift_changed, sp.min_pixels, sp.cover, sp.warmup, sp.invert,
                         float(sp.min_score), sp.classes)


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


# ---------------------------------------------------------------------------------------------------------------- update
def descs(c, base, a=0, b=None):
    """the case's targets a .. b - 1 as the wrappers take them"""
    out = []
    for d in c.desc[a:b]:
        if d is None:
            out.append(None)
        elif c.fmt == "bgr":
            out.append((base + d[0], d[1], d[2], d[3]))
        else:
            out.append((base + d[0], base + d[1], d[2], d[3], d[4], d[5]))
    return out


def run_update(F, c, splits=None):
    """the case on the device, as one call or split into several at the given target numbers; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    fn = F.motion_update_bgr_dev if c.fmt == "bgr" else F.motion_update_nv12_dev
    cs = c_spec(F, c.spec)
    cuts = [0] + list(splits or []) + [c.n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a != b:
            fn(descs(c, base, a, b), c.streams[a:b], cs, base + c.state_off, c.nstreams, base + c.row_off + 4 * motionref.ROW * a)
    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("fmt,name", UPDATE_PARAMS)
def test_update(F, fmt, name):
    """one call from the case's first state: the whole arena against motionref -- the frames and every padding byte stayed; the same call again from
    the same state: the same bytes"""
    c = fuzzcases.update_cases(fmt)[name]
    got = run_update(F, c)
    differ(c.what, got, c.want, c.regions())
    assert run_update(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_split_calls_leave_the_same_bytes(F, fmt):
    """3 streams x 4 frames in one call, in 4 calls (a round each) and in 12 (a frame each) leave the same bytes; so do other sequences cut anywhere"""
    c = fuzzcases.update_cases(fmt)["3 streams x 4"]
    assert c.n == 12
    for cuts in ([3, 6, 9], list(range(1, 12)), [5], [2, 7]):
        differ("%s split at %s" % (c.what, cuts), run_update(F, c, cuts), c.want, c.regions())
    for name, cuts in (("skipped", [1, 2, 3, 6]), ("targets 130", [64, 67, 100]), ("learn 1 converges", [1, 9])):
        c = fuzzcases.update_cases(fmt)[name]
        differ("%s split at %s" % (c.what, cuts), run_update(F, c, cuts), c.want, c.regions())


def test_reset(F):
    """ffgpu_motion_reset_dev zeroes one stream or all and nothing else"""
    import torch
    c = fuzzcases.update_cases("bgr")["3 streams x 4"]
    sp = c.spec
    got = run_update(F, c)
    nb, one = motionref.state_nbytes(3, sp.w, sp.h, sp.cell_log2), motionref.stream_nbytes(sp.w, sp.h, sp.cell_log2)
    assert all(got[c.state_off + s * one:c.state_off + (s + 1) * one].any() for s in range(3))
    dev = torch.from_numpy(got.copy()).cuda()
    geo = (3, sp.w, sp.h, sp.cell_log2)
    F.motion_reset_dev(dev.data_ptr() + c.state_off, *geo, 1)
    torch.cuda.synchronize()
    want = got.copy()
    want[c.state_off + one:c.state_off + 2 * one] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    F.motion_reset_dev(dev.data_ptr() + c.state_off, *geo)
    torch.cuda.synchronize()
    want[c.state_off:c.state_off + nb] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    p = dev.data_ptr()
    for args, msg in (((None,) + geo + (-1,), "NULL state"), ((p + 8,) + geo + (-1,), "16-byte aligned"), ((p, 0, sp.w, sp.h, sp.cell_log2, -1), "0 streams"),
                      ((p, 3, 8193, sp.h, sp.cell_log2, -1), "8193 x 13 pixels"), ((p, 3, sp.w, 0, sp.cell_log2, -1), "23 x 0 pixels"), ((p, 3, sp.w, sp.h, 7, -1), "cell_log2 7"),
                      ((p,) + geo + (3,), "stream 3"), ((p,) + geo + (-2,), "stream -2")):
        assert F.lib().ffgpu_motion_reset_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_update_rejections(F, fmt):
    """every rejected argument with its message and the target's index; nothing is enqueued: the state and everything else stay; a working call
    afterwards"""
    import torch
    c = fuzzcases.update_cases(fmt)["skipped"]
    dev = torch.from_numpy(c.start.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    nv12 = fmt == "nv12"
    fn = L.ffgpu_motion_update_nv12_dev if nv12 else L.ffgpu_motion_update_bgr_dev
    table = F.nv12_frame_table if nv12 else F.bgr_frame_table
    good, n = descs(c, base), c.n
    streams = (C.c_int * n)(*c.streams)
    cls = (C.c_ubyte * 4)(1, 1, 0, 1)

    def sp(**kw):
        s = c_spec(F, c.spec)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def tab(k=None, **kw):
        t = table(good)
        for name_, v in kw.items():
            setattr(t[k], name_, v)
        return t

    def call(targets=tab(), nt=n, strm=streams, spec=sp(), state=base + c.state_off, ns=c.nstreams, rows=base + c.row_off):
        return fn(targets, nt, strm, spec, state, ns, rows, None)
    high, low = (C.c_int * n)(*c.streams), (C.c_int * n)(*c.streams)
    high[3], low[0] = 3, -2
    cases = [(dict(targets=None), "NULL targets"), (dict(strm=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(state=None), "NULL state"), (dict(rows=None), "NULL rows"),
             (dict(nt=0), "0 targets"), (dict(nt=-1), "-1 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"),
             (dict(state=base + c.state_off + 8), "the state must be 16-byte aligned"), (dict(strm=high), "target 3: stream 3 is outside -1 .. 2"), (dict(strm=low), "target 0: stream -2"),
             (dict(spec=sp(w=0)), "a model of 0 x 11 pixels (1..8192 each)"), (dict(spec=sp(h=8193)), "a model of 19 x 8193 pixels"), (dict(spec=sp(cell_log2=1)), "cell_log2 1 is outside 2..6"),
             (dict(spec=sp(cell_log2=7)), "cell_log2 7 is outside 2..6"), (dict(spec=sp(threshold=0)), "threshold 0 is outside 1..255"), (dict(spec=sp(threshold=256)), "threshold 256"),
             (dict(spec=sp(learn_shift=-1)), "learn_shift -1 is outside 0..16"), (dict(spec=sp(learn_shift=17)), "learn_shift 17"),
             (dict(spec=sp(learn_shift_changed=17)), "learn_shift_changed 17 is outside 0..16"), (dict(spec=sp(min_pixels=0)), "min_pixels 0 is outside 1..16"),
             (dict(spec=sp(min_pixels=17)), "min_pixels 17 is outside 1..16"), (dict(spec=sp(cover=0)), "cover 0 is outside 1..256"), (dict(spec=sp(cover=257)), "cover 257"),
             (dict(spec=sp(warmup=-1)), "warmup -1 is outside 0..65535"), (dict(spec=sp(warmup=65536)), "warmup 65536"), (dict(spec=sp(flags=2)), "unknown flags 0x2"),
             (dict(spec=sp(nclasses=3)), "nclasses 3 (0 with NULL classes, else 1..256)"), (dict(spec=sp(classes=C.addressof(cls))), "nclasses 0"),
             (dict(spec=sp(reserved=(C.c_int * 2)(0, 1))), "reserved must be 0"),
             (dict(spec=sp(w=20)), "target 0: 19 x 11 pixels, the spec's model is 20 x 11"), (dict(targets=tab(3, h=12)), "target 3: 19 x 12 pixels, the spec's model is 19 x 11"),
             (dict(targets=tab(4, w=0)), "target 4: bad size 0 x 11"), (dict(targets=tab(0, reserved=1)), "target 0: reserved must be 0")]
    if nv12:
        cases += [(dict(targets=tab(0, pitch_y=10)), "target 0: pitch_y 10 is below w = 19"), (dict(targets=tab(3, matrix=4)), "target 3: matrix 4"),
                  (dict(targets=tab(3, uv=good[3][1] + 1)), "is odd (U V pairs are written")]
    else:
        cases += [(dict(targets=tab(0, pitch=50)), "target 0: pitch 50 is below 3 w = 57")]
    for kw, msg in cases:
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == c.start.tobytes()                            # nothing was enqueued
    differ("after the rejections", run_update(F, c), c.want, c.regions())


# ---------------------------------------------------------------------------------------------------------------- gate
def run_gate(F, c, splits=None):
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    d_recs = to_dev(c.recs)
    d_flat = None if c.flat is None else to_dev(c.flat)
    cs = c_spec(F, c.spec)
    S = c.stride
    cuts = [0] + list(splits or []) + [c.n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == b:
            continue
        lists = None if d_flat is None else d_flat.data_ptr() + (0 if c.first is not None else 24 * a * S)
        F.motion_gate_dev(d_recs.data_ptr() + DETS.itemsize * a, lists, S if d_flat is not None else 0, c.streams[a:b], cs, base + c.state_off, c.nstreams,
                          base + c.words_off + 4 * (motionref.WORDS + 2 * S) * a,
                          None if c.recs_off is None else base + c.recs_off + DETS.itemsize * a, None if c.lists_off is None else base + c.lists_off + 24 * S * a,
                          list_first=None if c.first is None else c.first[a:b])
    torch.cuda.synchronize()
    assert d_recs.cpu().numpy().tobytes() == c.recs.tobytes() and (d_flat is None or d_flat.cpu().numpy().tobytes() == c.flat.view(np.uint8).tobytes())
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", fuzzcases.GATE_NAMES)
def test_gate(F, name):
    """one call: the whole arena against motionref -- the state among the bytes that stayed; the same call again: the same bytes"""
    c = fuzzcases.gate_cases()[name]
    got = run_gate(F, c)
    differ(c.what, got, c.want, c.regions())
    assert run_gate(F, c).tobytes() == got.tobytes(), "two runs differ"


def test_gate_split_calls(F):
    """the gate keeps nothing: a call cut into several gives the same bytes"""
    for name, cuts in (("records 130", [1, 64, 129]), ("warmth", [1, 2]), ("list_first", [2])):
        c = fuzzcases.gate_cases()[name]
        differ("%s split at %s" % (c.what, cuts), run_gate(F, c, cuts), c.want, c.regions())


def test_gate_rejections(F):
    """every rejected argument with its message, the entry's index where there is one; nothing is launched; a working call afterwards"""
    import torch
    c = fuzzcases.gate_cases()["list_first"]
    dev = torch.from_numpy(c.start.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    d_recs, d_flat = to_dev(c.recs), to_dev(c.flat)
    r, fl, n = d_recs.data_ptr(), d_flat.data_ptr(), c.n
    streams = (C.c_int * n)(*c.streams)
    first = (C.c_int * n)(*c.first)

    def sp(**kw):
        s = c_spec(F, c.spec)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(recs=r, lists=fl, stride=c.stride, first=first, strm=streams, nt=n, spec=sp(), state=base + c.state_off, ns=c.nstreams, words=base + c.words_off,
             orecs=base + c.recs_off, olists=base + c.lists_off):
        return L.ffgpu_motion_gate_dev(recs, lists, stride, first, strm, nt, spec, state, ns, words, orecs, olists, None)
    high, low, neg = (C.c_int * n)(*c.streams), (C.c_int * n)(*c.streams), (C.c_int * n)(*c.first)
    high[4], low[2], neg[3] = 2, -2, -1
    for kw, msg in ((dict(recs=None), "NULL records"), (dict(strm=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(state=None), "NULL state"),
                    (dict(words=None), "NULL words"), (dict(nt=0), "0 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"),
                    (dict(strm=high), "target 4: stream 2 is outside -1 .. 1"), (dict(strm=low), "target 2: stream -2"), (dict(state=base + c.state_off + 4), "the state must be 16-byte aligned"),
                    (dict(spec=sp(w=8193)), "a model of 8193 x 17 pixels"), (dict(spec=sp(cell_log2=0)), "cell_log2 0 is outside 2..6"), (dict(spec=sp(min_pixels=17)), "min_pixels 17 is outside 1..16"),
                    (dict(spec=sp(cover=0)), "cover 0 is outside 1..256"), (dict(spec=sp(flags=4)), "unknown flags 0x4"), (dict(spec=sp(nclasses=2)), "nclasses 2"),
                    (dict(spec=sp(reserved=(C.c_int * 2)(1, 0))), "reserved must be 0"), (dict(orecs=None), "d_out_lists without d_out_records"),
                    (dict(orecs=r), "the outputs must not overlap the inputs"), (dict(olists=fl), "the outputs must not overlap the inputs"),
                    (dict(stride=0), "bad list_stride 0"), (dict(stride=2 ** 24 + 1), "bad list_stride"), (dict(first=neg), "target 3: negative list start -1")):
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == c.start.tobytes()                            # nothing was launched
    differ("after the rejections", run_gate(F, c), c.want, c.regions())


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


def moved(picture, boxes):
    """the picture with every byte inside every second box moved by 48: those boxes lie on pixels whose luma changed by 48, the others on pixels
    that did not change"""
    out = picture.copy()
    h, w = picture.shape[:2]
    for b in boxes[::2]:
        x0, y0, x1, y1 = (max(0, int(b[c])) for c in ("x1", "y1", "x2", "y2"))
        sub = picture[y0:min(y1, h - 1) + 1, x0:min(x1, w - 1) + 1].astype(np.int64)
        out[y0:min(y1, h - 1) + 1, x0:min(x1, w - 1) + 1] = np.where(sub < 128, sub + 48, sub - 48).astype(np.uint8)
    return out


@pytest.mark.parametrize("flags,invert", [(0, False), (32, True)])
def test_exec_gate_then_draw_bgr(F, net, picture, flags, invert):
    """data/test.bmp as one video stream (flags 32: FFGPU_SPLIT2): the model learns the picture, then sees it with every second box's inside
    inverted: update, forward, ffgpu_exec_motion_gate (ENTRIES), the gated record drawn.  State, rows, words and the gated record and list equal
    motionref on the frames and the boxes read back; the frames equal drawref on the gated boxes; the executor's records, lists and graph stay.
    Rejected calls leave the state and the executor usable."""
    import torch
    h, w = picture.shape[:2]
    pitch = 3 * w + 4
    ms = motionref.Spec(w, h, 4, 24, 2, 6, 32, 96, 0, invert, 0.25)
    cs = c_spec(F, ms)
    state = motionref.State(2, w, h, 4)
    with net.executor(2, flags) as ex:
        S = ex.cand_capacity
        first = np.zeros((2, h, pitch), np.uint8)
        first[:, :, :3 * w] = picture.reshape(h, 3 * w)
        d_first = torch.from_numpy(first).cuda()
        ex.forward_bgr_frames_dev([(d_first.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)])
        boxes0 = ex.read_boxes(0)
        assert len(boxes0) >= 2
        pics = [moved(picture, boxes0), moved(picture, boxes0[1:])]
        buf = np.zeros((2, h, pitch), np.uint8)
        for t in range(2):
            buf[t, :, :3 * w] = pics[t].reshape(h, 3 * w)
        dev = torch.from_numpy(buf).cuda()
        frames = [(dev.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)]
        d_state = torch.zeros(motionref.state_nbytes(2, w, h, 4), dtype=torch.uint8, device="cuda")
        d_rows = torch.full((4 * 4 * motionref.ROW,), 0xA5, dtype=torch.uint8, device="cuda")
        # the model learns the picture (streams 1 and 0), then sees the changed frames
        F.motion_update_bgr_dev([(d_first.data_ptr() + t * h * pitch, w, h, pitch) for t in range(2)] + frames, [1, 0, 1, 0], cs, d_state.data_ptr(), 2, d_rows.data_ptr())
        torch.cuda.synchronize()
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(2)], ex.graph_captures
        d_words = torch.full((4 * 2 * (motionref.WORDS + 2 * S),), 0xA5, dtype=torch.uint8, device="cuda")
        d_orecs = torch.full((2 * DETS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        d_olists = torch.full((2 * S * 24,), 0xA5, dtype=torch.uint8, device="cuda")
        ex.motion_gate([1, 0], cs, d_state.data_ptr(), 2, d_words.data_ptr(), d_orecs.data_ptr(), d_olists.data_ptr())
        torch.cuda.synchronize()
        F.draw_boxes_bgr_dev(d_orecs.data_ptr(), d_olists.data_ptr(), S, frames, F.draw_style((0, 255, 0), None, 2))
        torch.cuda.synchronize()
        lumas = [motionref.luma_bgr(picture)] * 2 + [motionref.luma_bgr(p) for p in pics]
        rows = motionref.update(lumas, [1, 0, 1, 0], ms, state)
        assert d_rows.cpu().numpy().tobytes() == rows.tobytes(), "rows"
        assert d_state.cpu().numpy().tobytes() == state.tobytes(), "state"
        assert rows[2, 1] > 1000 and rows[2, 2] >= 1 and rows[3, 2] >= 1 and rows[2, 7] == 1
        words, orecs, olists = motionref.gate(dets, flat_of(boxes, S), S, None, [1, 0], ms, state)
        assert d_words.cpu().numpy().tobytes() == words.tobytes(), "words"
        assert d_orecs.cpu().numpy().tobytes() == orecs.tobytes() and d_olists.cpu().numpy().tobytes() == olists.tobytes(), "the gated record"
        assert 0 < int(orecs["nfull"].sum()) < int(words[:, 0].sum()), "the gate selects some boxes and rejects some"
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(2))
        want = buf.copy().reshape(-1)
        for t in range(2):
            sel = olists[t, :int(orecs[t]["nfull"])]
            drawref.draw_bgr(want, t * h * pitch, w, h, pitch, sel, drawref.colours_of(sel, (0, 255, 0)), 2)
        assert (want != buf.reshape(-1)).sum() > 500
        differ("frames", dev.cpu().numpy().reshape(-1), want)
        # rejected: the executor and the state stay usable
        L = F.lib()
        two = (C.c_int * 2)(0, 1)
        p = (d_state.data_ptr(), 2, d_words.data_ptr(), d_orecs.data_ptr(), d_olists.data_ptr())
        before = d_words.cpu().numpy().tobytes()
        for call, msg in ((lambda: L.ffgpu_exec_motion_gate(ex.h, 2, two, 2, cs, *p, None), "which = 2"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 1, two, 2, cs, *p, None), "no ffgpu_exec_merge_tiles has run"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 0, two, 1, cs, *p, None), "1 targets for an executor of batch 2"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 0, two, 2, cs, *p, torch.cuda.Stream().cuda_stream), "stream of the forward"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 0, None, 2, cs, *p, None), "NULL streams"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 0, two, 2, cs, p[0], p[1], None, p[3], p[4], None), "NULL words"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 0, two, 2, cs, p[0], p[1], p[2], None, p[4], None), "d_out_lists without d_out_records"),
                          (lambda: L.ffgpu_exec_motion_gate(ex.h, 0, (C.c_int * 2)(0, 2), 2, cs, *p, None), "target 1: stream 2 is outside")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert d_words.cpu().numpy().tobytes() == before and d_state.cpu().numpy().tobytes() == state.tobytes()
        ex.motion_gate([1, 0], cs, d_state.data_ptr(), 2, d_words.data_ptr())          # and a call without gated records still works
        torch.cuda.synchronize()
        assert d_words.cpu().numpy().tobytes() == words.tobytes()


def test_exec_gate_merged_then_draw(F, net, picture):
    """2 pictures x 2 tiles: the model learns the wide pictures, then sees them with boxes' insides inverted; forward, merge,
    ffgpu_exec_motion_gate (MERGED) on the merged lists, one stream per picture, the gated record drawn into the pictures"""
    import torch
    h, w = picture.shape[:2]
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    base = np.stack([wide, np.ascontiguousarray(wide[::-1])])
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    p = 3 * 1280
    ms = motionref.Spec(1280, h, 5, 24, 2, 6, 64, 64, 0, False, 0.25)
    cs = c_spec(F, ms)

    def tiles_of(dev):
        frames, tiles = [], []
        for g in range(2):
            for x0, y0, tw, th in plan:
                frames.append((dev.data_ptr() + g * h * p + y0 * p + 3 * x0, tw, th, p))
                tiles.append((g, x0, y0))
        return frames, tiles

    with net.executor(4) as ex:
        d_base = torch.from_numpy(base).cuda()
        frames, tiles = tiles_of(d_base)
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 2)
        lists0 = [ex.read_merged_boxes(g) for g in range(2)]
        assert all(len(b) >= 2 for b in lists0)
        pics = np.stack([moved(base[g], lists0[g]) for g in range(2)])
        dev = torch.from_numpy(pics).cuda()
        whole = [(dev.data_ptr() + g * h * p, 1280, h, p) for g in range(2)]
        d_state = torch.zeros(motionref.state_nbytes(2, 1280, h, 5), dtype=torch.uint8, device="cuda")
        d_rows = torch.full((4 * 4 * motionref.ROW,), 0xA5, dtype=torch.uint8, device="cuda")
        F.motion_update_bgr_dev([(d_base.data_ptr() + g * h * p, 1280, h, p) for g in range(2)] + whole, [0, 1, 0, 1], cs, d_state.data_ptr(), 2, d_rows.data_ptr())
        torch.cuda.synchronize()
        frames, tiles = tiles_of(dev)
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 2)
        merged, lists = ex.read_merged(2), [ex.read_merged_boxes(g) for g in range(2)]
        S = 2 * ex.cand_capacity                                                      # a picture's merged list has room for its tiles' boxes
        d_words = torch.full((4 * 2 * (motionref.WORDS + 2 * S),), 0xA5, dtype=torch.uint8, device="cuda")
        d_orecs = torch.full((2 * DETS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        d_olists = torch.full((2 * S * 24,), 0xA5, dtype=torch.uint8, device="cuda")
        ex.motion_gate([0, 1], cs, d_state.data_ptr(), 2, d_words.data_ptr(), d_orecs.data_ptr(), d_olists.data_ptr(), which=F.MOTION_MERGED)
        torch.cuda.synchronize()
        F.draw_boxes_bgr_dev(d_orecs.data_ptr(), d_olists.data_ptr(), S, whole, F.draw_style((0, 0, 255), None, 1))
        torch.cuda.synchronize()
        state = motionref.State(2, 1280, h, 5)
        rows = motionref.update([motionref.luma_bgr(base[g]) for g in range(2)] + [motionref.luma_bgr(pics[g]) for g in range(2)], [0, 1, 0, 1], ms, state)
        assert d_rows.cpu().numpy().tobytes() == rows.tobytes() and d_state.cpu().numpy().tobytes() == state.tobytes()
        words, orecs, olists = motionref.gate(merged, flat_of(lists, S), S, None, [0, 1], ms, state)
        assert d_words.cpu().numpy().tobytes() == words.tobytes()
        assert d_orecs.cpu().numpy().tobytes() == orecs.tobytes() and d_olists.cpu().numpy().tobytes() == olists.tobytes()
        assert 0 < int(orecs["nfull"].sum()) < int(words[:, 0].sum()), "the gate selects some boxes and rejects some"
        want = pics.copy().reshape(-1)
        for g in range(2):
            sel = olists[g, :int(orecs[g]["nfull"])]
            drawref.draw_bgr(want, g * h * p, 1280, h, p, sel, drawref.colours_of(sel, (0, 0, 255)), 1)
        differ("pictures", dev.cpu().numpy().reshape(-1), want)
        assert ex.read_merged(2).tobytes() == merged.tobytes() and all(ex.read_merged_boxes(g).tobytes() == lists[g].tobytes() for g in range(2))
