"""Tracking across frames: a float32 numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_track_boxes_dev), one frame of one video
stream at a time, in the contract's own words:

    1. the record's list in list order: a box is considered when score >= min_score (NaN never), until DETS boxes are; the rest is `dropped`;
    2. iou of every (track, detection) pair with the merge's arithmetic (use_min == 0), every operation one np.float32 operation in the stated order;
       eligible: iou >= iou_thresh (NaN never) and, class_aware, equal types;
    3. the eligible pairs SORTED by (iou descending, slot ascending, detection ascending) and walked: both unmatched -> a match;
    4. matched tracks take the detection; 5. unmatched ones age and are freed beyond max_missed; 6. births into the lowest free slots in detection
       order; 7. frames += 1, live counted.

GPU results are compared with THIS, byte for byte.  tests/test_tracks_abi.py pins it to a literal scalar loop and to hand-written cases."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS = 128
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])
TRACK_DTYPE = np.dtype([("id", "<i4"), ("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"),
                        ("hits", "<i4"), ("missed", "<i4"), ("born", "<i4"), ("det", "<i4"), ("reserved", "<i4")])
HEADER = ("considered", "matched", "born", "refused", "dropped", "freed", "live", "frame")
F32 = np.float32


class Spec:
    def __init__(self, capacity, max_missed=0, min_hits=1, iou_thresh=0.3, min_score=0.0, birth_score=0.0, class_aware=1):
        self.capacity, self.max_missed, self.min_hits, self.class_aware = capacity, max_missed, min_hits, int(class_aware)
        self.iou_thresh, self.min_score, self.birth_score = F32(iou_thresh), F32(min_score), F32(birth_score)


class State:
    """nstreams headers { issued, frames, live, reserved } and nstreams x capacity slots; all zero: empty"""

    def __init__(self, nstreams, capacity, raw=None):
        self.nstreams, self.capacity = nstreams, capacity
        self.hdr = np.zeros((nstreams, 4), "<i4")
        self.slots = np.zeros((nstreams, capacity), TRACK_DTYPE)
        if raw is not None:
            raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, 16 + 48 * capacity)
            self.hdr[:] = np.ascontiguousarray(raw[:, :16]).view("<i4")
            self.slots[:] = np.ascontiguousarray(raw[:, 16:]).view(TRACK_DTYPE).reshape(nstreams, capacity)

    def tobytes(self):
        return b"".join(self.hdr[s].tobytes() + self.slots[s].tobytes() for s in range(self.nstreams))

    def copy(self):
        return State(self.nstreams, self.capacity, np.frombuffer(self.tobytes(), np.uint8))


def state_nbytes(nstreams, capacity):
    return nstreams * (16 + 48 * capacity)


def iou_matrix(tracks, dets):
    """fp32 [len(tracks), len(dets)]: area = (x2 - x1) * (y2 - y1); inter from the max / min corners if xa < xb and ya < yb, else 0;
    inter / (area_a + area_j - inter).  The corner selections are the C expressions a > b ? a : b and a < b ? a : b (a NaN in a loses)."""
    ax1, ay1, ax2, ay2 = (np.asarray(tracks[c], F32)[:, None] for c in ("x1", "y1", "x2", "y2"))
    bx1, by1, bx2, by2 = (np.asarray(dets[c], F32)[None, :] for c in ("x1", "y1", "x2", "y2"))
    with np.errstate(all="ignore"):
        area_a = (ax2 - ax1) * (ay2 - ay1)
        area_j = (bx2 - bx1) * (by2 - by1)
        xa, ya = np.where(ax1 > bx1, ax1, bx1), np.where(ay1 > by1, ay1, by1)
        xb, yb = np.where(ax2 < bx2, ax2, bx2), np.where(ay2 < by2, ay2, by2)
        inter = np.where((xa < xb) & (ya < yb), (xb - xa) * (yb - ya), F32(0))
        uni = (area_a + area_j) - inter
        out = inter / uni
    assert out.dtype == np.float32
    return out


def frame(hdr, slots, boxes, spec, stride):
    """one frame: hdr (4 ints) and slots (capacity entries) of the stream are updated in place; boxes: the record's list, already clamped.
    Returns (ids row of 8 + stride ints, the tracked boxes)."""
    row = np.zeros(8 + stride, "<i4")
    boxes = np.asarray(boxes, BOX_DTYPE)
    with np.errstate(invalid="ignore"):
        qual = np.nonzero(boxes["score"] >= spec.min_score)[0]
    cons, dropped = qual[:DETS], max(0, len(qual) - DETS)
    det = boxes[cons]
    occ = np.nonzero(slots["id"] != 0)[0]
    tmatch, dmatch = {}, {}
    if len(occ) and len(det):
        m = iou_matrix(slots[occ], det)
        with np.errstate(invalid="ignore"):
            ok = m >= spec.iou_thresh
        if spec.class_aware:
            ok &= slots["type"][occ][:, None] == det["type"][None, :]
        a, j = np.nonzero(ok)
        order = np.lexsort((j, occ[a], -m[a, j].astype(np.float64)))
        for a_, j_ in zip(occ[a][order], j[order]):
            if int(a_) not in tmatch and int(j_) not in dmatch:
                tmatch[int(a_)], dmatch[int(j_)] = int(j_), int(a_)
    freed = 0
    for s in occ:
        tr = slots[s]
        if int(s) in tmatch:
            b = det[tmatch[int(s)]]
            for c in ("type", "score", "x1", "y1", "x2", "y2"):
                tr[c] = b[c]
            tr["hits"] += 1
            tr["missed"] = 0
            tr["det"] = cons[tmatch[int(s)]]
        else:
            tr["missed"] += 1
            tr["det"] = -1
            if tr["missed"] > spec.max_missed:
                slots[s] = np.zeros((), TRACK_DTYPE)
                freed += 1
    born = refused = 0
    issued, frames = int(hdr[0]), int(hdr[1])
    for j_ in range(len(det)):
        with np.errstate(invalid="ignore"):
            if j_ in dmatch or not det[j_]["score"] >= spec.birth_score:
                continue
        free = np.nonzero(slots["id"] == 0)[0]
        if not len(free):
            refused += 1
            continue
        issued += 1
        b = det[j_]
        slots[free[0]] = (issued, b["type"], b["score"], b["x1"], b["y1"], b["x2"], b["y2"], 1, 0, frames, cons[j_], 0)
        dmatch[j_] = int(free[0])
        born += 1
    live = int((slots["id"] != 0).sum())
    hdr[0], hdr[1], hdr[2] = issued, frames + 1, live
    row[:8] = (len(det), len(tmatch), born, refused, dropped, freed, live, frames)
    out = []
    for j_ in sorted(dmatch):
        tr = slots[dmatch[j_]]
        sure = int(tr["hits"]) >= spec.min_hits
        row[8 + cons[j_]] = int(tr["id"]) if sure else -int(tr["id"])
        if sure:
            b = det[j_].copy()
            b["type"] = tr["id"]
            out.append(b)
    return row, (np.array(out, BOX_DTYPE) if out else np.zeros(0, BOX_DTYPE))


def tracked_record(tracked, rec):
    r = np.zeros((), DETS_DTYPE)
    n = len(tracked)
    r["count"], r["nfull"], r["ncand"] = min(n, MAX_DET), n, rec["ncand"]
    r["overflow"] = (int(rec["overflow"]) & 1) | (4 if n > MAX_DET else 0)
    r["box"][:min(n, MAX_DET)] = tracked[:MAX_DET]
    return r


def track(records, flat, stride, first, streams, spec, state):
    """the whole operator.  records: DETS_DTYPE array; flat: the lists' memory as one BOX_DTYPE array, or None (the records' own boxes, stride =
    MAX_DET); first: list starts (None: t * stride); streams: one video stream per record, -1: ignored; state: a State, updated in place.
    Returns (ids [ntargets, 8 + stride], tracked records [ntargets], tracked lists [ntargets, stride])."""
    if flat is None:
        stride = MAX_DET
    n = len(records)
    ids = np.zeros((n, 8 + stride), "<i4")
    recs, lists = np.zeros(n, DETS_DTYPE), np.zeros((n, stride), BOX_DTYPE)
    for t in range(n):
        if streams[t] < 0:
            continue
        r = records[t]
        cnt = max(0, min(int(r["nfull"] if flat is not None else r["count"]), stride))
        if flat is None:
            boxes = r["box"][:cnt]
        else:
            f0 = t * stride if first is None else first[t]
            boxes = flat[f0:f0 + cnt]
        ids[t], tb = frame(state.hdr[streams[t]], state.slots[streams[t]], boxes, spec, stride)
        recs[t] = tracked_record(tb, r)
        lists[t, :len(tb)] = tb
    return ids, recs, lists
