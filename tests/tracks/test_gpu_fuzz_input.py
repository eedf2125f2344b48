"""The detections tracked across frames on the device: ffgpu_track_boxes_dev / ffgpu_track_reset_dev (the operator, on synthetic records and lists)
and ffgpu_exec_track (behind a forward or a merge of the real net), against tests/tracks/trackref.py, the numpy restatement of the contract in
include/ffcnn_hip.h.  State, ids, tracked records and tracked lists lie in one arena of seeded random bytes with 64 guard bytes around each; the
WHOLE arena is compared: the state and the ids byte for byte, the tracked boxes word for word with NaN coordinates as a NaN pattern (as
tests/detect_tail does), every other byte must have stayed.  The seeded cases are built on the CPU once (cases()) and shared by the tests.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from overlay import drawref
from tracks import trackref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX, DETS = trackref.BOX_DTYPE, trackref.DETS_DTYPE
GUARD = 64
F32 = np.float32
NAN, INF = float("nan"), float("inf")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---------------------------------------------------------------------------------------------------------------- seeded streams
def video(rng, nframes, counts, spread=400, weird=0.03):
    """nframes lists of one video stream: objects that persist and move a little (so they match), exact copies of other boxes of the frame (exact
    IoU ties), newcomers, class flips, scores on a grid of eighths (ties with the thresholds), NaN / Inf sprinkled in"""
    out, prev = [], np.zeros(0, BOX)
    for f in range(nframes):
        n = counts[f % len(counts)]
        b = np.zeros(n, BOX)
        for k in range(n):
            kind = rng.random()
            if kind < 0.5 and len(prev):
                b[k] = prev[int(rng.integers(0, len(prev)))]
                if rng.random() < 0.6:
                    for c in ("x1", "y1", "x2", "y2"):
                        b[k][c] += F32(rng.integers(-3, 4))
                if rng.random() < 0.1:
                    b[k]["type"] += 1
            elif kind < 0.65 and k:
                b[k] = b[int(rng.integers(0, k))]
            else:
                x, y = rng.integers(0, spread, 2)
                b[k] = (int(rng.integers(0, 3)), 0, x, y, x + int(rng.integers(2, 40)), y + int(rng.integers(2, 40)))
            b[k]["score"] = F32(rng.integers(0, 9)) / F32(8)
            if rng.random() < weird:
                b[k][("x1", "y1", "x2", "y2", "score")[int(rng.integers(0, 5))]] = (NAN, INF, -INF, 1e30)[int(rng.integers(0, 4))]
        out.append(b)
        prev = b
    return out


class Case:
    """one sequence of records over some video streams, built on the CPU: the arena, the inputs, and what trackref makes of them from the empty state"""

    def __init__(self, seed, nstreams, spec, streams, lists, use_records=False, first_given=False, claimed=None, with_lists_out=True, with_out=True, what=""):
        rng = self.rng = np.random.default_rng(seed)
        self.nstreams, self.spec, self.streams, self.use_records, self.what = nstreams, spec, list(streams), use_records, what
        n = self.n = len(streams)
        self.stride = 128 if use_records else max(1, max(len(b) for b in lists)) + 3
        self.recs = np.zeros(n, DETS)
        for t, b in enumerate(lists):
            r = self.recs[t]
            r["count"], r["nfull"], r["ncand"], r["overflow"] = min(len(b), 128), len(b), len(b) + t, int(rng.integers(0, 8))
            r["box"][:min(len(b), 128)] = b[:128]
        for t, v in (claimed or {}).items():                                      # counts outside their range: the field that is read, and junk in the other
            self.recs[t]["count" if use_records else "nfull"] = v
            self.recs[t]["nfull" if use_records else "count"] = 7
        order = list(rng.permutation(n)) if first_given else list(range(n))      # list t lies in slot order[t] of the lists' memory
        self.first = [int(s) * self.stride + (int(s) % 3 if first_given else 0) for s in order] if first_given else None
        self.flat = None
        if not use_records:
            self.flat = np.zeros(n * self.stride + 3, BOX)
            self.flat.view(np.uint8)[:] = 0x3C                                    # (slots behind a list hold junk: never read ...)
            for t, b in enumerate(lists):
                f0 = self.first[t] if first_given else t * self.stride
                self.flat[f0:f0 + len(b)] = b
                v = (claimed or {}).get(t)
                if v is not None and v > len(b):                                  # (... unless the record claims them: then they are boxes like any other)
                    self.flat[f0 + len(b):f0 + self.stride] = video(rng, 1, [self.stride - len(b)])[0]
        self.ar_size = 0
        self.state_off = self._alloc(trackref.state_nbytes(nstreams, spec.capacity), 16)
        self.ids_off = self._alloc(4 * n * (8 + self.stride), 4)
        self.rec_off = self._alloc(DETS.itemsize * n, 4) if with_out else None
        self.list_off = self._alloc(24 * n * self.stride, 4) if with_out and with_lists_out else None
        self.ar_size += GUARD
        self.start = rng.integers(0, 256, self.ar_size, dtype=np.uint8)
        self.start[self.state_off:self.state_off + trackref.state_nbytes(nstreams, spec.capacity)] = 0        # the empty state
        st = trackref.State(nstreams, spec.capacity)
        self.ids, self.orecs, self.olists = trackref.track(self.recs, self.flat, self.stride, self.first, self.streams, spec, st)
        self.state = st
        self.want = self.start.copy()
        self._put(self.state_off, np.frombuffer(st.tobytes(), np.uint8))
        self._put(self.ids_off, self.ids)
        if self.rec_off is not None:
            self._put(self.rec_off, self.orecs)
        if self.list_off is not None:
            self._put(self.list_off, self.olists)

    def _alloc(self, nbytes, align):
        off = -(-(self.ar_size + GUARD) // align) * align
        self.ar_size = off + nbytes
        return off

    def _put(self, off, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.want[off:off + len(raw)] = raw

    def regions(self):
        r = [("state", self.state_off, trackref.state_nbytes(self.nstreams, self.spec.capacity)), ("ids", self.ids_off, 4 * self.n * (8 + self.stride))]
        if self.rec_off is not None:
            r.append(("tracked records", self.rec_off, DETS.itemsize * self.n))
        if self.list_off is not None:
            r.append(("tracked lists", self.list_off, 24 * self.n * self.stride))
        return r

    def header_sums(self):
        return dict(zip(trackref.HEADER, (int(v) for v in self.ids[:, :8].sum(axis=0))))

    def run(self, F, splits=None):
        """the case on the device, as one call or split into several at the given record numbers; returns the arena's bytes afterwards"""
        import torch
        dev = torch.from_numpy(self.start.copy()).cuda()
        base = dev.data_ptr()
        assert base % 256 == 0
        d_recs = to_dev(self.recs)
        d_flat = None if self.flat is None else to_dev(self.flat)
        sp = self.spec
        cs = F.track_spec(sp.capacity, sp.max_missed, sp.min_hits, float(sp.iou_thresh), float(sp.min_score), float(sp.birth_score), sp.class_aware)
        cuts = [0] + list(splits or []) + [self.n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == b:
                continue
            lists_ptr = None if d_flat is None else d_flat.data_ptr() + (0 if self.first is not None else 24 * a * self.stride)
            F.track_boxes_dev(d_recs.data_ptr() + DETS.itemsize * a, lists_ptr, 0 if d_flat is None else self.stride, self.streams[a:b], cs, base + self.state_off,
                              self.nstreams, base + self.ids_off + 4 * a * (8 + self.stride),
                              None if self.rec_off is None else base + self.rec_off + DETS.itemsize * a,
                              None if self.list_off is None else base + self.list_off + 24 * a * self.stride,
                              list_first=None if self.first is None else self.first[a:b])
        torch.cuda.synchronize()
        assert d_recs.cpu().numpy().tobytes() == self.recs.tobytes()              # the inputs are only read
        return dev.cpu().numpy()

    def check(self, got, what=""):
        bad = got != self.want
        for off in (self.rec_off, self.list_off):                                  # tracked boxes: NaN as NaN, not by payload
            if off is None:
                continue
            nb = dict((r[1], r[2]) for r in self.regions())[off]
            g, w = got[off:off + nb].view(F32), self.want[off:off + nb].view(F32)
            bad[off:off + nb] &= ~np.repeat(np.isnan(g) & np.isnan(w), 4)
        if not bad.any():
            return
        idx = np.nonzero(bad)[0]
        for name, lo, nb in self.regions():
            hit = idx[(idx >= lo - GUARD) & (idx < lo + nb + GUARD)]
            if len(hit):
                pytest.fail("%s %s: %s: %d bytes differ, first at region offset %d (region of %d bytes): got %d, want %d"
                            % (self.what, what, name, len(hit), int(hit[0]) - lo, nb, got[hit[0]], self.want[hit[0]]), pytrace=False)
        pytest.fail("%s %s: %d bytes differ outside every region, first at %d" % (self.what, what, len(idx), int(idx[0])), pytrace=False)


def interleave(rng, per_stream, ignored=0):
    """the streams' frames in one table: each stream's frames in order, the streams interleaved at random, `ignored` entries of stream -1 in between"""
    left = [len(v) for v in per_stream]
    streams, lists = [], []
    pool = [s for s, k in enumerate(left) for _ in range(k)] + [-1] * ignored
    for s in rng.permutation(pool):
        s = int(s)
        streams.append(s)
        if s < 0:
            lists.append(video(rng, 1, [5])[0])
        else:
            lists.append(per_stream[s][len(per_stream[s]) - left[s]])
            left[s] -= 1
    return streams, lists


_CASES = {}


def cases():
    if _CASES:
        return _CASES
    S = trackref.Spec
    c = {}
    # capacities 1, 2, 3, 127, 128 on one stream of 5 frames (more boxes than slots: refusals; max_missed 0 and 1: slots freed and re-used)
    for cap, mm in ((1, 0), (2, 1), (3, 0), (127, 1), (128, 1)):
        rng = np.random.default_rng(5500 + cap)
        nb = [cap + 40, cap + 40, cap // 2, cap + 40, cap] if cap > 3 else [4, 2, 0, 5, 3]
        c["capacity %d" % cap] = Case(5510 + cap, 1, S(cap, max_missed=mm, min_hits=2, iou_thresh=0.25, min_score=0.125, birth_score=0.25), [0] * 5,
                                      video(rng, 5, nb, spread=2000 if cap > 3 else 60), what="capacity %d" % cap)
    # 0, 1, 127, 128, 129 and 200 qualifying boxes (min_score 0: every box but a NaN score qualifies), two frames each so that 128 x 128 is matched
    rng = np.random.default_rng(5520)
    lists = []
    for n in (0, 1, 127, 128, 129, 200):
        v = video(rng, 2, [n], spread=3000, weird=0.0)
        v[1] = v[0].copy() if n != 129 else v[1]
        lists += v
    c["counts"] = Case(5521, 6, S(128, max_missed=1, min_hits=2, iou_thresh=0.5), [s for s in range(6) for _ in range(2)], lists, what="counts 0..200")
    # the worst case: 128 identical tracks x 128 identical boxes -- every pair ties, one match per round
    same = np.zeros(130, BOX)
    same[:] = (1, 0.5, 10, 10, 50, 50)
    c["all ties"] = Case(5522, 1, S(128, iou_thresh=1.0, max_missed=2), [0, 0], [same, same], what="128 x 128 ties")
    # nstreams 1, 3, 65: interleaved, some entries ignored, 1, 2 and 5 frames of a stream inside one call; 65 streams x 2..6 frames cross the 128-entry chunk
    for ns, nframes, ign in ((1, [5], 2), (3, [1, 2, 5], 3), (65, [2 + (s % 5 == 0) + 3 * (s % 7 == 0) for s in range(65)], 9)):
        rng = np.random.default_rng(5530 + ns)
        per = [video(rng, nframes[s], [int(rng.integers(0, 9)) for _ in range(3)], spread=80) for s in range(ns)]
        streams, lists = interleave(rng, per, ign)
        c["nstreams %d" % ns] = Case(5531 + ns, ns, S(6, max_missed=1, min_hits=2, iou_thresh=0.25, birth_score=0.25, class_aware=ns != 3), streams, lists,
                                     what="nstreams %d (%d entries)" % (ns, len(streams)))
    assert len(c["nstreams 65"].streams) > 128
    # list_first with irregular starts; the records' own boxes (no lists); no tracked output at all; records without lists out
    rng = np.random.default_rng(5540)
    per = [video(rng, 4, [7, 3, 9], spread=80) for _ in range(3)]
    streams, lists = interleave(rng, per, 2)
    c["list_first"] = Case(5541, 3, S(8, max_missed=2, min_hits=3, iou_thresh=0.25), streams, lists, first_given=True, what="list_first")
    c["records"] = Case(5542, 3, S(8, max_missed=2, min_hits=1, iou_thresh=0.25, class_aware=0), streams, lists, use_records=True, with_lists_out=False, what="own boxes")
    c["ids only"] = Case(5543, 3, S(8, max_missed=0, min_hits=2, iou_thresh=0.0), streams, lists, with_out=False, what="ids only")
    # counts outside their range are clamped to [0, stride]
    rng = np.random.default_rng(5550)
    lists = video(rng, 6, [20, 18, 22], spread=120)
    claimed = {0: -1, 1: 2 ** 31 - 1, 2: -2 ** 31, 3: 26, 4: 1000}
    c["clamped lists"] = Case(5551, 2, S(16, max_missed=1, iou_thresh=0.25), [0, 0, 1, 0, 1, 1], lists, claimed=claimed, what="clamped nfull")
    lists = video(rng, 4, [128, 100], spread=2000)
    c["clamped records"] = Case(5552, 1, S(128, max_missed=1, iou_thresh=0.25), [0] * 4, lists, use_records=True, claimed={0: 129, 1: -7, 3: 2 ** 31 - 1}, what="clamped count")
    # 131 records of 3 streams, lists of 0 to 5 boxes: two launches (128 records, then 3), ignored entries in both.  The second launch has room for three
    # records: the last frames of streams 2 and 0 with an ignored entry between them, so two streams span the boundary
    rng = np.random.default_rng(5580)
    per = [video(rng, nf, [int(rng.integers(0, 6)) for _ in range(3)], spread=60) for nf in (40, 44, 41)]
    streams, lists = interleave(rng, [per[0][:-1], per[1], per[2][:-1]], 5)
    streams, lists = streams + [2, -1, 0], lists + [per[2][-1], video(rng, 1, [5])[0], per[0][-1]]
    c["records 131"] = Case(5581, 3, S(6, max_missed=1, min_hits=2, iou_thresh=0.25, birth_score=0.25), streams, lists, what="131 records")
    _CASES.update(c)
    return _CASES


NAMES = ["capacity 1", "capacity 2", "capacity 3", "capacity 127", "capacity 128", "counts", "all ties", "nstreams 1", "nstreams 3", "nstreams 65",
         "list_first", "records", "ids only", "clamped lists", "clamped records", "records 131"]


def test_seeded_set_covers_every_path():
    """on the CPU: the cases reach what they are for"""
    cs = cases()
    assert sorted(cs) == sorted(NAMES)
    tot = {k: sum(c.header_sums()[k] for c in cs.values()) for k in trackref.HEADER}
    assert all(tot[k] > 0 for k in ("considered", "matched", "born", "refused", "dropped", "freed", "live")), tot
    counts = cs["counts"].ids[:, :8]
    assert [int(v) for v in counts[::2, 0]] == [0, 1, 127, 128, 128, 128] and [int(v) for v in counts[::2, 4]] == [0, 0, 0, 0, 1, 72]
    assert int(counts[7, 1]) == 128                                                  # 128 tracks matched to 128 boxes
    assert cs["all ties"].header_sums()["matched"] == 128 and (cs["all ties"].ids[1, 8:136] == np.arange(1, 129)).all()
    for cap in (1, 2, 3, 127, 128):
        h = cs["capacity %d" % cap].header_sums()
        assert h["refused"] > 0 and h["freed"] > 0 and h["matched"] > 0, (cap, h)
        assert int(cs["capacity %d" % cap].ids[:, 6].max()) == cap                     # every slot was in use
    assert any((c.ids[:, 8:] < 0).any() and (c.ids[:, 8:] > 0).any() for c in cs.values())
    assert sum(int(np.isnan(c.olists["x1"]).sum() + np.isnan(c.olists["y2"]).sum()) for c in cs.values()) > 0     # NaN boxes reach the tracked lists
    ties = 0
    for name in ("nstreams 3", "list_first"):                                          # exact IoU ties between different pairs
        c = cs[name]
        for t in range(c.n):
            b = c.flat[(c.first[t] if c.first else t * c.stride):][:int(c.recs[t]["nfull"])]
            if len(b) > 1:
                m = trackref.iou_matrix(b, b)
                ties += int(((m[:, :, None] == m[:, None, :]) & (m[:, :, None] > 0)).sum() > (m > 0).sum())
    assert ties > 0
    # "records 131": the first launch holds every stream and an ignored entry; the second (three records: no room for more) an ignored entry and two
    # streams; a track issued before the boundary is matched again behind it (trackref alone: the state after the first 128 records)
    c = cs["records 131"]
    assert c.n == 131 and c.spec.capacity == 6 and {len(c.flat[t * c.stride:][:int(c.recs[t]["nfull"])]) for t in range(c.n)} == set(range(6))
    assert set(c.streams[:128]) == {-1, 0, 1, 2} and c.streams[128:] == [2, -1, 0]
    st = trackref.State(3, 6)
    trackref.track(c.recs[:128], c.flat, c.stride, None, c.streams[:128], c.spec, st)
    assert all(int(st.hdr[s][1]) > 0 for s in range(3))                             # (frames: every stream has a history at the boundary)
    carried = [int(((np.abs(c.ids[t, 8:]) > 0) & (np.abs(c.ids[t, 8:]) <= int(st.hdr[c.streams[t]][0]))).sum()) for t in (128, 130)]
    assert sum(carried) > 0 and not c.ids[129].any(), carried


@pytest.mark.parametrize("name", NAMES)
def test_operator(F, name):
    """one call from the empty state: the whole arena against trackref; the same call again from the same state: the same bytes"""
    c = cases()[name]
    got = c.run(F)
    c.check(got)
    assert c.run(F).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("name", ["capacity 3", "counts", "nstreams 3", "nstreams 65", "list_first", "records", "clamped lists"])
def test_split_calls_leave_the_same_bytes(F, name):
    """the sequence cut into several calls (the state carries the streams across) leaves what one call leaves"""
    c = cases()[name]
    rng = np.random.default_rng(5560)
    for cuts in ([c.n // 2], sorted(int(v) for v in rng.integers(0, c.n + 1, 3)), list(range(1, c.n)) if c.n <= 12 else [1, c.n - 1]):
        c.check(c.run(F, cuts), "split at %s" % cuts)


def test_reset(F):
    """ffgpu_track_reset_dev zeroes one stream or all and nothing else; a zeroed stream starts again at id 1 and frame 0"""
    import torch
    c = cases()["nstreams 3"]
    got = c.run(F)
    nb, one = trackref.state_nbytes(3, c.spec.capacity), trackref.state_nbytes(1, c.spec.capacity)
    assert got[c.state_off:c.state_off + nb].any()
    dev = torch.from_numpy(got.copy()).cuda()
    F.track_reset_dev(dev.data_ptr() + c.state_off, 3, c.spec.capacity, 1)
    torch.cuda.synchronize()
    want = got.copy()
    want[c.state_off + one:c.state_off + 2 * one] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    F.track_reset_dev(dev.data_ptr() + c.state_off, 3, c.spec.capacity)
    torch.cuda.synchronize()
    want[c.state_off:c.state_off + nb] = 0
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    for args, msg in (((None, 3, 6, -1), "NULL state"), ((dev.data_ptr() + 8, 3, 6, -1), "16-byte aligned"), ((dev.data_ptr(), 0, 6, -1), "0 streams"),
                      ((dev.data_ptr(), 3, 129, -1), "129 slots"), ((dev.data_ptr(), 3, 6, 3), "stream 3"), ((dev.data_ptr(), 3, 6, -2), "stream -2")):
        assert F.lib().ffgpu_track_reset_dev(*args, None) < 0 and msg in F.last_error(), (msg, F.last_error())


def test_operator_rejections(F):
    """every rejected argument with its message, the entry's index where there is one; the state (and everything else) stays as it was"""
    import torch
    c = cases()["nstreams 3"]
    before = c.run(F)
    dev = torch.from_numpy(before.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    d_recs, d_flat = to_dev(c.recs), to_dev(c.flat)
    r, fl, st, ids, orec, ol = d_recs.data_ptr(), d_flat.data_ptr(), base + c.state_off, base + c.ids_off, base + c.rec_off, base + c.list_off
    n = c.n
    streams = (C.c_int * n)(*c.streams)

    def sp(**kw):
        s = F.track_spec(6, 1, 2, 0.25, 0.0, 0.25, 0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(recs=r, lists=fl, stride=c.stride, first=None, strm=streams, nt=n, spec=sp(), state=st, ns=3, idp=ids, orp=orec, olp=ol):
        return L.ffgpu_track_boxes_dev(recs, lists, stride, first, strm, nt, spec, state, ns, idp, orp, olp, None)
    bad_stream = (C.c_int * n)(*c.streams)
    bad_stream[4] = 3
    low_stream = (C.c_int * n)(*c.streams)
    low_stream[2] = -2
    neg_first = (C.c_int * n)(*([0] * n))
    neg_first[5] = -1
    for kw, msg in ((dict(recs=None), "NULL records"), (dict(strm=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(state=None), "NULL state"),
                    (dict(idp=None), "NULL ids"), (dict(nt=0), "0 targets"), (dict(nt=-1), "-1 targets"), (dict(ns=0), "nstreams 0"), (dict(ns=65537), "nstreams 65537"),
                    (dict(strm=bad_stream), "target 4: stream 3 is outside -1 .. 2"), (dict(strm=low_stream), "target 2: stream -2"),
                    (dict(ns=2), r"target \d+: stream 2 is outside -1 .. 1"),
                    (dict(spec=sp(capacity=0)), "capacity 0"), (dict(spec=sp(capacity=129)), "capacity 129"), (dict(spec=sp(max_missed=-1)), "max_missed -1"),
                    (dict(spec=sp(max_missed=2 ** 20 + 1)), "max_missed"), (dict(spec=sp(min_hits=0)), "min_hits 0"), (dict(spec=sp(min_hits=2 ** 20 + 1)), "min_hits"),
                    (dict(spec=sp(iou_thresh=NAN)), "iou_thresh"), (dict(spec=sp(iou_thresh=1.5)), "iou_thresh"), (dict(spec=sp(iou_thresh=-0.5)), "iou_thresh"),
                    (dict(spec=sp(min_score=INF)), "min_score"), (dict(spec=sp(min_score=-1.0)), "min_score"), (dict(spec=sp(birth_score=NAN)), "birth_score"),
                    (dict(spec=sp(birth_score=2.0)), "birth_score"), (dict(spec=sp(class_aware=2)), "class_aware 2"), (dict(spec=sp(class_aware=-1)), "class_aware -1"),
                    (dict(spec=sp(reserved=1)), "reserved"), (dict(state=st + 8), "16-byte aligned"), (dict(stride=0), "bad list_stride 0"),
                    (dict(stride=2 ** 24 + 1), "bad list_stride"), (dict(first=neg_first), "target 5: negative list start -1"), (dict(orp=None), "d_out_lists without d_out_records")):
        assert call(**kw) < 0, kw
        assert re.search(msg, F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == before.tobytes()                            # nothing was launched
    dev = torch.from_numpy(c.start.copy()).cuda()                                      # and the next valid call is right
    base = dev.data_ptr()
    F.track_boxes_dev(r, fl, c.stride, c.streams, sp(), base + c.state_off, 3, base + c.ids_off, base + c.rec_off, base + c.list_off)
    torch.cuda.synchronize()
    c.check(dev.cpu().numpy(), "after the rejections")


# ---------------------------------------------------------------------------------------------------------------- on an executor
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


def picture_on_device(picture, pad=4):
    import torch
    h, w = picture.shape[:2]
    buf = np.zeros((h, 3 * w + pad), np.uint8)
    buf[:, :3 * w] = picture.reshape(h, 3 * w)
    return torch.from_numpy(buf).cuda(), 3 * w + pad


class Buffers:
    """state (zero), ids, tracked records and lists for n records of stride S, filled with 0xA5"""

    def __init__(self, n, S, nstreams, capacity):
        import torch
        self.n, self.S, self.nstreams, self.capacity = n, S, nstreams, capacity
        self.state = torch.zeros(trackref.state_nbytes(nstreams, capacity), dtype=torch.uint8, device="cuda")
        self.ids = torch.full((4 * n * (8 + S),), 0xA5, dtype=torch.uint8, device="cuda")
        self.recs = torch.full((DETS.itemsize * n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.lists = torch.full((24 * n * S,), 0xA5, dtype=torch.uint8, device="cuda")

    def read(self):
        import torch
        torch.cuda.synchronize()
        return (self.state.cpu().numpy(), self.ids.cpu().numpy().view("<i4").reshape(self.n, 8 + self.S), self.recs.cpu().numpy().view(DETS),
                self.lists.cpu().numpy().view(BOX).reshape(self.n, self.S))


def against_trackref(bufs, recs, lists, streams, spec, state, what):
    """the buffers after a call against trackref on the boxes read back; `state` (a trackref.State) is advanced"""
    S = bufs.S
    flat = np.zeros((len(recs), S), BOX)
    for t, b in enumerate(lists):
        flat[t, :len(b)] = b
    ids, orecs, olists = trackref.track(recs, flat.reshape(-1), S, None, streams, spec, state)
    g_state, g_ids, g_recs, g_lists = bufs.read()
    assert g_state.tobytes() == state.tobytes(), what + ": state"
    assert g_ids.tobytes() == ids.tobytes(), what + ": ids"
    assert g_recs.tobytes() == orecs.tobytes(), what + ": tracked records"
    assert g_lists.tobytes() == olists.tobytes(), what + ": tracked lists"
    return ids, orecs, olists


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_track_entries(F, net, picture, flags):
    """data/test.bmp in 4 entries as one video stream (flags 32: FFGPU_SPLIT2), min_hits 2: equal to trackref on the boxes read back; identical frames
    give identical boxes, a box's IoU with itself is 1 and the survivors of the net's NMS overlap less, so at iou_thresh 1 every box of entries
    1 .. 3 carries as a positive id what entry 0 gave it as a negative one.  The records, the lists and the captured graph stay."""
    dev, pitch = picture_on_device(picture)
    frames = [(dev.data_ptr(), 640, 424, pitch)] * 4
    spec = trackref.Spec(16, max_missed=0, min_hits=2, iou_thresh=1.0)
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(4)], ex.graph_captures
        assert len(boxes[0]) == 3 and all(b.tobytes() == boxes[0].tobytes() for b in boxes)
        bufs = Buffers(4, ex.cand_capacity, 1, 16)
        ex.track([0, 0, 0, 0], F.track_spec(16, 0, 2, 1.0), bufs.state.data_ptr(), 1, bufs.ids.data_ptr(), bufs.recs.data_ptr(), bufs.lists.data_ptr())
        state = trackref.State(1, 16)
        ids, orecs, olists = against_trackref(bufs, dets, boxes, [0] * 4, spec, state, "exec entries, flags %d" % flags)
        assert [int(v) for v in ids[0, 8:11]] == [-1, -2, -3] and all([int(v) for v in ids[t, 8:11]] == [1, 2, 3] for t in (1, 2, 3))
        assert [int(v) for v in ids[:, 7]] == [0, 1, 2, 3] and [int(r["count"]) for r in orecs] == [0, 3, 3, 3]
        assert [int(v) for v in orecs[3]["box"]["type"][:3]] == [1, 2, 3] and orecs[3]["box"]["x1"][:3].tobytes() == boxes[0]["x1"].tobytes()
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(4))
        # the next forward continues the stream: two entries ignored
        ex.forward_bgr_frames_dev(frames)
        ex.track([0, -1, -1, 0], F.track_spec(16, 0, 2, 1.0), bufs.state.data_ptr(), 1, bufs.ids.data_ptr(), bufs.recs.data_ptr(), bufs.lists.data_ptr())
        ids, _, _ = against_trackref(bufs, dets, boxes, [0, -1, -1, 0], spec, state, "exec entries again, flags %d" % flags)
        assert [int(v) for v in ids[:, 7]] == [4, 0, 0, 5] and [int(v) for v in ids[3, 8:11]] == [1, 2, 3]


def test_exec_track_merged_and_rejections(F, net, picture):
    """FFGPU_TRACK_MERGED behind a two-tile merge of a 1280 x 424 picture, twice: the second time every merged box has the positive id of the first;
    before any merge, on the wrong stream, with a wrong ntargets or `which`: rejected, and the executor and the state stay usable"""
    import torch
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    dev, pitch = picture_on_device(wide, pad=7)
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    assert len(plan) == 2
    frames = [(dev.data_ptr() + y0 * pitch + 3 * x0, tw, th, pitch) for x0, y0, tw, th in plan]
    spec, cs = trackref.Spec(32, max_missed=0, min_hits=2, iou_thresh=1.0), F.track_spec(32, 0, 2, 1.0)
    L = F.lib()
    with net.executor(2) as ex:
        ex.forward_bgr_frames_dev(frames)
        bufs = Buffers(1, 2 * ex.cand_capacity, 1, 32)
        p = (bufs.state.data_ptr(), 1, bufs.ids.data_ptr(), bufs.recs.data_ptr(), bufs.lists.data_ptr())
        one = (C.c_int * 2)(0, 0)
        with pytest.raises(RuntimeError, match="no ffgpu_exec_merge_tiles has run"):
            ex.track([0], cs, *p, which=F.TRACK_MERGED)
        for call, msg in ((lambda: L.ffgpu_exec_track(ex.h, 2, one, 2, cs, *p, None), "which = 2"),
                          (lambda: L.ffgpu_exec_track(ex.h, 0, one, 1, cs, *p, None), "1 targets for an executor of batch 2"),
                          (lambda: L.ffgpu_exec_track(ex.h, 0, one, 2, cs, *p, torch.cuda.Stream().cuda_stream), "stream of the forward"),
                          (lambda: L.ffgpu_exec_track(ex.h, 0, None, 2, cs, *p, None), "NULL streams"),
                          (lambda: L.ffgpu_exec_track(ex.h, 0, one, 2, cs, p[0] + 4, *p[1:], None), "16-byte aligned"),
                          (lambda: L.ffgpu_exec_track(ex.h, 0, one, 2, cs, p[0], 1, p[2], None, p[4], None), "d_out_lists without d_out_records"),
                          (lambda: L.ffgpu_exec_track(ex.h, 0, (C.c_int * 2)(0, 1), 2, cs, *p, None), "target 1: stream 1 is outside")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert not bufs.state.cpu().numpy().any() and (bufs.ids.cpu().numpy() == 0xA5).all()      # nothing was launched
        state = trackref.State(1, 32)
        for rep in range(2):
            if rep:
                ex.forward_bgr_frames_dev(frames)
            ex.merge_tiles([(0, x0, y0) for x0, y0, _, _ in plan], 1)
            merged, lists = ex.read_merged(1), [ex.read_merged_boxes(0)]
            n = len(lists[0])
            assert n >= 4
            with pytest.raises(RuntimeError, match="2 targets for a merge of 1 pictures"):
                ex.track([0, 0], cs, *p, which=F.TRACK_MERGED)
            ex.track([0], cs, *p, which=F.TRACK_MERGED)
            ids, orecs, _ = against_trackref(bufs, merged, lists, [0], spec, state, "exec merged %d" % rep)
            want = np.arange(1, n + 1)
            assert (ids[0, 8:8 + n] == (want if rep else -want)).all() and int(orecs[0]["nfull"]) == (n if rep else 0)
            assert ex.read_merged(1).tobytes() == merged.tobytes() and ex.graph_captures == 1


def test_tracked_record_draws_per_object(F):
    """the composition: the tracked record drawn with ffgpu_draw_boxes_bgr_dev equals drawref on trackref's tracked record -- the palette entry is
    type mod npalette and type is the track id, so an object keeps its colour while its class and its place in the list change"""
    import torch
    w, h, pitch = 96, 64, 300
    a = np.zeros(3, BOX)
    a[0], a[1], a[2] = (5, 0.9, 4, 4, 30, 30), (5, 0.8, 40, 10, 80, 50), (2, 0.7, 10, 40, 30, 60)
    b = a[[2, 0, 1]].copy()                                                           # the next frame: another order, moved a little, one class changed
    for c in ("x1", "x2"):
        b[c] += F32(2)
    b["type"][1] = 6
    recs = np.zeros(2, DETS)
    for t, l in enumerate((a, b)):
        recs[t]["count"], recs[t]["nfull"], recs[t]["ncand"] = 3, 3, 3
        recs[t]["box"][:3] = l
    spec = trackref.Spec(8, iou_thresh=0.5, class_aware=0)
    state = trackref.State(1, 8)
    ids, orecs, _ = trackref.track(recs, None, 0, None, [0, 0], spec, state)
    assert [int(v) for v in orecs[1]["box"]["type"][:3]] == [3, 1, 2]
    palette = [(255, 0, 0, 0), (0, 255, 0, 0), (0, 0, 255, 0), (9, 99, 199, 0)]
    rng = np.random.default_rng(5570)
    start = rng.integers(0, 256, 2 * pitch * h, dtype=np.uint8)
    dev = torch.from_numpy(start.copy()).cuda()
    d_recs = to_dev(recs)
    d_state = torch.zeros(trackref.state_nbytes(1, 8), dtype=torch.uint8, device="cuda")
    d_ids = torch.zeros(4 * 2 * (8 + 128), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(DETS.itemsize * 2, dtype=torch.uint8, device="cuda")
    F.track_boxes_dev(d_recs.data_ptr(), None, 0, [0, 0], F.track_spec(8, iou_thresh=0.5, class_aware=0), d_state.data_ptr(), 1, d_ids.data_ptr(), d_out.data_ptr())
    targets = [(dev.data_ptr(), w, h, pitch), (dev.data_ptr() + pitch * h, w, h, pitch)]
    F.draw_boxes_bgr_dev(d_out.data_ptr(), None, 0, targets, F.draw_style(palette=palette))
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == orecs.tobytes()
    want = start.copy()
    for t in range(2):
        bx = orecs[t]["box"][:int(orecs[t]["count"])]
        drawref.draw_bgr(want, t * pitch * h, w, h, pitch, bx, drawref.colours_of(bx, palette=palette))
    assert dev.cpu().numpy().tobytes() == want.tobytes()
    assert (want != start).any()
