"""Tracking the detections across frames, without a GPU: the exported symbols, the layout of ffgpu_track_spec / ffgpu_track in the ctypes mirror and
the constants in the header, ffgpu_track_state_bytes, tests/tracks/trackref.py (the numpy restatement of the contract the GPU tests compare with)
pinned to a literal scalar loop on seeded cases and to hand-written cases, the host glue under ASan + UBSan (san/track_driver.cc, run as a child
process), and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tracks import trackref

SYMBOLS = ["ffgpu_track_state_bytes", "ffgpu_track_reset_dev", "ffgpu_track_boxes_dev", "ffgpu_exec_track"]
NAN, INF = float("nan"), float("inf")
F32 = np.float32
S = trackref.Spec
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def boxes_of(rows):
    """rows: (x1, y1, x2, y2[, type[, score]])"""
    b = np.zeros(len(rows), trackref.BOX_DTYPE)
    for k, r in enumerate(rows):
        b[k] = (r[4] if len(r) > 4 else 0, r[5] if len(r) > 5 else 0.5, r[0], r[1], r[2], r[3])
    return b


def run(frames, spec, stride=None):
    """one stream, its frames one after the other: ([header dict per frame], [ids per frame], [tracked boxes per frame], the state)"""
    st = trackref.State(1, spec.capacity)
    hdrs, ids, outs = [], [], []
    for b in frames:
        n = stride or max(1, len(b))
        row, tb = trackref.frame(st.hdr[0], st.slots[0], b, spec, n)
        hdrs.append(dict(zip(trackref.HEADER, (int(v) for v in row[:8]))))
        ids.append([int(v) for v in row[8:8 + len(b)]])
        outs.append(tb)
    return hdrs, ids, outs, st


def test_track_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_track_struct_layout(capi):
    P, T = capi.TrackSpec, capi.Track
    assert C.sizeof(P) == 32 and C.sizeof(T) == 48
    assert [getattr(P, f).offset for f in ("capacity", "max_missed", "min_hits", "iou_thresh", "min_score", "birth_score", "class_aware",
                                           "reserved")] == list(range(0, 32, 4))
    assert [f[0] for f in T._fields_] == list(trackref.TRACK_DTYPE.names) and [getattr(T, f[0]).offset for f in T._fields_] == list(range(0, 48, 4))
    assert capi.TRACK_DTYPE == trackref.TRACK_DTYPE and capi.TRACK_DTYPE.itemsize == 48 and trackref.BOX_DTYPE == capi.BOX_DTYPE
    assert (capi.TRACK_DETS, capi.TRACK_ENTRIES, capi.TRACK_MERGED) == (128, 0, 1) and trackref.DETS == 128
    assert capi.TRACK_IDS_HEADER == trackref.HEADER and len(trackref.HEADER) == 8
    sp = capi.track_spec(5, max_missed=2, min_hits=3, iou_thresh=0.25, min_score=0.125, birth_score=0.5, class_aware=0)
    assert (sp.capacity, sp.max_missed, sp.min_hits, sp.iou_thresh, sp.min_score, sp.birth_score, sp.class_aware, sp.reserved) == (5, 2, 3, 0.25, 0.125, 0.5, 0, 0)
    hdr, slots = capi.track_state(np.zeros(3 * (16 + 48 * 5), np.uint8), 3, 5)
    assert len(hdr) == 3 and hdr[0] == dict(issued=0, frames=0, live=0, reserved=0) and slots.shape == (3, 5)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    assert "} ffgpu_track_spec;" in hdr and "} ffgpu_track;" in hdr and "32 bytes" in hdr and "16-byte header" in hdr
    for name, val in (("FFGPU_TRACK_DETS", 128), ("FFGPU_TRACK_ENTRIES", 0), ("FFGPU_TRACK_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(ROOT, "ffcnn_amd", "csrc", "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_track.inc"' in inc and inc.index('#include "ffgpu_crop.inc"') < inc.index('#include "ffgpu_track.inc"')


def test_state_bytes_is_pure_host_code(capi):
    """no device needed; 0 for arguments outside their ranges"""
    assert [capi.track_state_bytes(*a) for a in ((1, 1), (1, 128), (3, 5), (65536, 128))] == [64, 16 + 48 * 128, 3 * (16 + 240), 65536 * (16 + 48 * 128)]
    assert [capi.track_state_bytes(*a) for a in ((0, 1), (-1, 1), (65537, 1), (1, 0), (1, -3), (1, 129), (0, 0))] == [0] * 7
    for ns, cap in ((1, 1), (3, 5), (65, 128)):
        assert capi.track_state_bytes(ns, cap) == trackref.state_nbytes(ns, cap) == len(trackref.State(ns, cap).tobytes())


# ------------------------------------------------------------------------------------------------- trackref against a literal scalar loop
def literal_iou(a, b):
    """one pair, one np.float32 operation per line of the contract"""
    def area(x1, y1, x2, y2):
        return F32(F32(x2 - x1) * F32(y2 - y1))
    ax1, ay1, ax2, ay2 = (F32(a[c]) for c in ("x1", "y1", "x2", "y2"))
    bx1, by1, bx2, by2 = (F32(b[c]) for c in ("x1", "y1", "x2", "y2"))
    xa, ya = (ax1 if ax1 > bx1 else bx1), (ay1 if ay1 > by1 else by1)
    xb, yb = (ax2 if ax2 < bx2 else bx2), (ay2 if ay2 < by2 else by2)
    with np.errstate(all="ignore"):
        inter = area(xa, ya, xb, yb) if (xa < xb and ya < yb) else F32(0)
        uni = F32(F32(area(ax1, ay1, ax2, ay2) + area(bx1, by1, bx2, by2)) - inter)
        return F32(inter / uni)


def literal_frame(hdr, slots, boxes, spec, stride):
    """the contract word for word on Python lists of dicts; the matching takes the first remaining pair of the total order again and again"""
    cons, dropped = [], 0
    for k, b in enumerate(boxes):
        if b["score"] >= spec.min_score:
            if len(cons) < 128:
                cons.append(k)
            else:
                dropped += 1
    pairs = {}
    for s, tr in enumerate(slots):
        for j, k in enumerate(cons):
            if tr["id"] != 0:
                v = literal_iou(tr, boxes[k])
                if v >= spec.iou_thresh and (not spec.class_aware or tr["type"] == boxes[k]["type"]):
                    pairs[(s, j)] = v
    tmatch, dmatch = {}, {}
    while True:
        best = None
        for (s, j) in sorted(pairs):                                   # slot ascending, then detection ascending: a strict > keeps the first
            if s in tmatch or j in dmatch:
                continue
            if best is None or pairs[(s, j)] > pairs[best]:
                best = (s, j)
        if best is None:
            break
        tmatch[best[0]], dmatch[best[1]] = best[1], best[0]
    freed = 0
    for s, tr in enumerate(slots):
        if tr["id"] == 0:
            continue
        if s in tmatch:
            b = boxes[cons[tmatch[s]]]
            tr.update(type=b["type"], score=b["score"], x1=b["x1"], y1=b["y1"], x2=b["x2"], y2=b["y2"], hits=tr["hits"] + 1, missed=0, det=cons[tmatch[s]])
        else:
            tr.update(missed=tr["missed"] + 1, det=-1)
            if tr["missed"] > spec.max_missed:
                slots[s] = dict.fromkeys(trackref.TRACK_DTYPE.names, 0)
                freed += 1
    born = refused = 0
    for j, k in enumerate(cons):
        b = boxes[k]
        if j in dmatch or not b["score"] >= spec.birth_score:
            continue
        free = [s for s, tr in enumerate(slots) if tr["id"] == 0]
        if not free:
            refused += 1
            continue
        hdr["issued"] += 1
        slots[free[0]] = dict(id=hdr["issued"], type=b["type"], score=b["score"], x1=b["x1"], y1=b["y1"], x2=b["x2"], y2=b["y2"], hits=1, missed=0,
                              born=hdr["frames"], det=k, reserved=0)
        dmatch[j] = free[0]
        born += 1
    frame_no = hdr["frames"]
    hdr["frames"] += 1
    hdr["live"] = sum(tr["id"] != 0 for tr in slots)
    row = [len(cons), len(tmatch), born, refused, dropped, freed, hdr["live"], frame_no] + [0] * stride
    out = []
    for j, k in enumerate(cons):
        if j in dmatch:
            tr = slots[dmatch[j]]
            row[8 + k] = tr["id"] if tr["hits"] >= spec.min_hits else -tr["id"]
            if tr["hits"] >= spec.min_hits:
                out.append((tr["id"],) + tuple(boxes[k][c] for c in ("score", "x1", "y1", "x2", "y2")))
    return row, out


def same_bits(a, b):
    return np.asarray(a, F32).tobytes() == np.asarray(b, F32).tobytes()


def seeded_frame(rng, prev, n):
    """n boxes: some near the previous frame's (so they match), some exact copies of each other (exact ties), some new, NaN / Inf sprinkled in"""
    b = np.zeros(n, trackref.BOX_DTYPE)
    for k in range(n):
        kind = rng.random()
        if kind < 0.45 and len(prev):
            b[k] = prev[int(rng.integers(0, len(prev)))]
            if rng.random() < 0.6:
                for c in ("x1", "y1", "x2", "y2"):
                    b[k][c] += F32(rng.integers(-3, 4))
            if rng.random() < 0.15:
                b[k]["type"] += 1
        elif kind < 0.6 and k:
            b[k] = b[int(rng.integers(0, k))]
        else:
            x, y = rng.integers(0, 60, 2)
            b[k] = (int(rng.integers(0, 3)), 0, x, y, x + int(rng.integers(1, 30)), y + int(rng.integers(1, 30)))
        b[k]["score"] = F32(rng.integers(0, 9)) / F32(8)
        if rng.random() < 0.04:
            b[k][("x1", "y1", "x2", "y2", "score")[int(rng.integers(0, 5))]] = (NAN, INF, -INF)[int(rng.integers(0, 3))]
    return b


def test_trackref_is_the_literal_loop():
    rng = np.random.default_rng(5400)
    seen = dict.fromkeys(("matched", "born", "refused", "freed", "tie", "neg"), 0)
    for case in range(60):
        cap = int(rng.choice([1, 2, 3, 7, 16]))
        spec = S(cap, max_missed=int(rng.integers(0, 3)), min_hits=int(rng.integers(1, 4)), iou_thresh=float(rng.choice([0.0, 0.25, 0.5, 1.0])),
                 min_score=float(rng.choice([0.0, 0.25])), birth_score=float(rng.choice([0.0, 0.5])), class_aware=int(rng.integers(0, 2)))
        st = trackref.State(1, cap)
        hdr, slots = dict(issued=0, frames=0, live=0), [dict.fromkeys(trackref.TRACK_DTYPE.names, 0) for _ in range(cap)]
        prev = np.zeros(0, trackref.BOX_DTYPE)
        for f in range(6):
            b = seeded_frame(rng, prev, int(rng.integers(0, 12)))
            stride = len(b) + 2
            row, tb = trackref.frame(st.hdr[0], st.slots[0], b, spec, stride)
            lrow, lout = literal_frame(hdr, slots, [dict(zip(b.dtype.names, (x[c] for c in b.dtype.names))) for x in b], spec, stride)
            assert list(row) == lrow, (case, f)
            assert len(tb) == len(lout) and all(int(x["type"]) == o[0] and same_bits([x[c] for c in ("score", "x1", "y1", "x2", "y2")], o[1:]) for x, o in zip(tb, lout)), (case, f)
            assert [int(v) for v in st.hdr[0][:3]] == [hdr["issued"], hdr["frames"], hdr["live"]]
            for s in range(cap):
                for c in trackref.TRACK_DTYPE.names:
                    assert same_bits(st.slots[0][s][c], slots[s][c]) if c in ("score", "x1", "y1", "x2", "y2") else int(st.slots[0][s][c]) == int(slots[s][c]), (case, f, s, c)
            for k, name in ((1, "matched"), (2, "born"), (3, "refused"), (5, "freed")):
                seen[name] += int(row[k])
            seen["neg"] += int((row[8:] < 0).sum())
            if len(b) > 1:
                m = trackref.iou_matrix(b, b)
                seen["tie"] += int(((m == m[:, :1]) & np.isfinite(m)).sum() > len(b))
            prev = b
    assert all(v > 0 for v in seen.values()), seen


def test_iou_with_itself_is_exactly_one():
    """finite non-degenerate boxes: inter == area and a + a - a is exact.  The end-to-end property of the GPU tests (identical frames keep their ids
    at any threshold up to 1) rests on this."""
    rng = np.random.default_rng(5401)
    b = np.zeros(4000, trackref.BOX_DTYPE)
    b["x1"], b["y1"] = rng.uniform(-500, 500, len(b)), rng.uniform(-500, 500, len(b))
    b["x2"], b["y2"] = b["x1"] + rng.uniform(1e-3, 700, len(b)).astype(F32), b["y1"] + rng.uniform(1e-3, 700, len(b)).astype(F32)
    b = b[(b["x2"] > b["x1"]) & (b["y2"] > b["y1"])]
    assert len(b) > 3900
    for k in range(0, len(b), 500):
        m = trackref.iou_matrix(b[k:k + 500], b[k:k + 500])
        assert (np.diagonal(m) == F32(1)).all()
    assert all(literal_iou(x, x) == F32(1) for x in b[:200])


# ------------------------------------------------------------------------------------------------- hand-written cases
def test_ties_are_broken_by_slot_then_index():
    """two identical boxes against two identical tracks: all four pairs have iou 1; slot 0 takes box 0 and slot 1 box 1"""
    two = boxes_of([(10, 10, 20, 20), (10, 10, 20, 20)])
    hdrs, ids, outs, st = run([two, two], S(2))
    assert ids == [[1, 2], [1, 2]] and hdrs[1]["matched"] == 2 and hdrs[1]["born"] == 0
    assert [int(v) for v in st.slots[0]["det"]] == [0, 1] and [int(v) for v in st.slots[0]["hits"]] == [2, 2]
    # a higher iou wins over a lower slot: slot 1's exact copy goes first, slot 0 takes what is left
    hdrs, ids, outs, st = run([boxes_of([(10, 10, 20, 20), (11, 10, 21, 20)]), boxes_of([(11, 10, 21, 20), (10.5, 10, 20.5, 20)])], S(2))
    assert ids[1] == [2, 1]


def test_nan_inf_zero_area_and_nan_score():
    sp = S(4, iou_thresh=0.25)
    first = boxes_of([(NAN, 0, 10, 10), (0, 0, INF, 10), (5, 5, 5, 9), (30, 30, 40, 40), (50, 50, 60, 60, 0, NAN)])
    hdrs, ids, outs, st = run([first, first], sp)
    assert hdrs[0] == dict(considered=4, matched=0, born=4, refused=0, dropped=0, freed=0, live=4, frame=0) and ids[0] == [1, 2, 3, 4, 0]
    # NaN corner: area NaN -> iou NaN, never eligible; Inf: inf / inf = NaN; zero area: 0 / 0 = NaN; only the finite box matches itself
    m = trackref.iou_matrix(first[:4], first[:4])
    assert np.isnan(np.diagonal(m)[:3]).all() and m[3, 3] == 1
    assert hdrs[1]["matched"] == 1 and hdrs[1]["freed"] == 3 and hdrs[1]["refused"] == 0 and ids[1] == [5, 6, 7, 4, 0]
    assert st.hdr[0][0] == 7


def test_max_missed_zero_frees_and_the_birth_reuses_the_slot():
    a, b = boxes_of([(0, 0, 10, 10)]), boxes_of([(50, 50, 60, 60)])
    hdrs, ids, outs, st = run([a, b], S(1, max_missed=0))
    assert hdrs[1] == dict(considered=1, matched=0, born=1, refused=0, dropped=0, freed=1, live=1, frame=1) and ids == [[1], [2]]
    assert int(st.slots[0][0]["id"]) == 2 and int(st.slots[0][0]["born"]) == 1
    # with max_missed = 1 the track stays, the slot is taken and the birth is refused at capacity 1
    hdrs, ids, outs, st = run([a, b, b], S(1, max_missed=1))
    assert (hdrs[1]["freed"], hdrs[1]["refused"], hdrs[1]["live"]) == (0, 1, 1) and ids[1] == [0]
    assert int(st.slots[0][0]["id"]) == 2 and (hdrs[2]["freed"], hdrs[2]["born"]) == (1, 1)


def test_class_flip():
    a, b = boxes_of([(0, 0, 10, 10, 1)]), boxes_of([(0, 0, 10, 10, 2)])
    hdrs, ids, outs, st = run([a, b], S(2, class_aware=1, max_missed=3))
    assert ids == [[1], [2]] and hdrs[1]["matched"] == 0 and hdrs[1]["live"] == 2
    hdrs, ids, outs, st = run([a, b], S(2, class_aware=0, max_missed=3))
    assert ids == [[1], [1]] and int(st.slots[0][0]["type"]) == 2


def test_min_hits_gives_negative_then_positive_ids():
    a = boxes_of([(0, 0, 10, 10, 7, 0.75)])
    hdrs, ids, outs, st = run([a] * 4, S(3, min_hits=3))
    assert ids == [[-1], [-1], [1], [1]] and [len(o) for o in outs] == [0, 0, 1, 1]
    o = outs[2][0]
    assert (int(o["type"]), float(o["score"]), float(o["x2"])) == (1, 0.75, 10.0)


def test_the_129th_qualifying_box_is_dropped():
    b = boxes_of([(4 * k, 0, 4 * k + 3, 3, 0, 0.5 if k != 5 else 0.1) for k in range(131)])
    hdrs, ids, outs, st = run([b], S(128, min_score=0.25))
    assert hdrs[0] == dict(considered=128, matched=0, born=128, refused=0, dropped=2, freed=0, live=128, frame=0)
    assert ids[0][5] == 0 and ids[0][128] == 128 and ids[0][129:] == [0, 0] and ids[0][:5] == [1, 2, 3, 4, 5] and ids[0][6] == 6


def test_birth_score_and_stream_independence():
    b = boxes_of([(0, 0, 10, 10, 0, 0.25), (20, 0, 30, 10, 0, 0.75)])
    hdrs, ids, outs, st = run([b, b], S(4, birth_score=0.5))
    assert ids == [[0, 1], [0, 1]] and hdrs[0]["considered"] == 2
    recs = np.zeros(4, trackref.DETS_DTYPE)
    for t in range(4):
        recs[t]["count"], recs[t]["nfull"], recs[t]["ncand"], recs[t]["overflow"] = 2, 2, 9, 1
        recs[t]["box"][:2] = b
    state = trackref.State(2, 4)
    ids_, orec, olist = trackref.track(recs, None, 0, None, [1, -1, 0, 1], S(4), state)
    assert [int(v) for v in state.hdr[:, 1]] == [1, 2] and not ids_[1].any() and orec[1].tobytes() == bytes(trackref.DETS_DTYPE.itemsize)
    assert list(ids_[3][:11]) == [2, 2, 0, 0, 0, 0, 2, 1, 1, 2, 0] and (int(orec[3]["ncand"]), int(orec[3]["overflow"]), int(orec[3]["nfull"])) == (9, 1, 2)
    assert [int(v) for v in olist[3]["type"][:3]] == [1, 2, 0]
    recs[0]["count"] = 1000                                                            # a count outside its range is clamped
    assert trackref.track(recs, None, 0, None, [0, -1, -1, -1], S(4), trackref.State(1, 4))[0][0][0] == 128


def test_track_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_track_boxes_dev(None, None, 0, None, None, 1, None, None, 1, None, None, None, None),
                 lambda: L.ffgpu_track_reset_dev(None, 1, 1, -1, None),
                 lambda: L.ffgpu_exec_track(None, 0, None, 1, None, None, 1, None, None, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


def test_host_glue_under_the_sanitizers():
    """san/track_driver.cc: the state's size, the spec and argument checks of ffgpu_track_host.hpp and a launch's entry table on the CPU under
    ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    host = open(os.path.join(CSRC, "ffgpu_track_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    inc, drv = open(os.path.join(CSRC, "ffgpu_track.inc")).read(), open(os.path.join(CSRC, "san", "track_driver.cc")).read()
    assert int(re.search(r"#define TRACK_ARG_ENTRIES\s+(\d+)", inc).group(1)) == 128 == int(re.search(r"#define ENTRIES\s+(\d+)", drv).group(1))
    subprocess.check_call(["make", "-s", "-C", CSRC, "track"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_track_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"track_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 68, out[-1]
    assert not any("WRONG" in ln for ln in out)
    for ln in ("args.stream_high -1 op: target 1: stream 2 is outside -1 .. 1", "args.lists_without_records -1 op: d_out_lists without d_out_records",
               "order.lists_before_streams -1 op: d_out_lists without d_out_records", "spec.min_hits_0 -1 op: min_hits 0 is outside 1..2^20",
               "spec.class_aware_2 -1 op: class_aware 2 is neither 0 nor 1", "bytes.65536_128 %d" % (65536 * (16 + 48 * 128)), "bytes.1_129 0",
               "entries.full_0 groups=54 ignored=31", "entries.tail groups=3 ignored=1", "entries.all_ignored groups=1 ignored=40", "entries.all_distinct groups=128 ignored=0"):
        assert ln in out, ln
