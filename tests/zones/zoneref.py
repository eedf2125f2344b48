"""Zones and lines: a float32 numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_zones_boxes_dev), one frame of one video stream at a
time, in the contract's own words:

    1. the record's list in list order: a box is considered when score >= min_score (NaN never), until DETS boxes are; the rest is `dropped`;
    2. anchor and inside mask of every considered box, every operation one np.float32 operation in the stated order, edge by edge (even-odd rule);
    3. owners: the first considered box of each identity > 0; later ones are duplicates, identities <= 0 anonymous;
    4. the owners SORTED by identity and walked: one whose identity is in a slot is known: entered / left / since / lines / loitering, the slot updated;
    5. slots nobody named age out beyond max_missed; every zone of their mask counts one left;
    6. the other owners in list order take the lowest free slot, or are refused;
    7. totals, live, frames += 1.

GPU results are compared with THIS, byte for byte.  tests/test_zones_abi.py pins it to a literal scalar loop and to properties."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS = 128
ROW = 64
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])
ZONE_DTYPE = np.dtype([("x", "<f4", (8,)), ("y", "<f4", (8,)), ("nverts", "<i4"), ("dwell_frames", "<i4"), ("classes", "<u4", (4,)), ("reserved", "<i4", (2,))])
LINE_DTYPE = np.dtype([("ax", "<f4"), ("ay", "<f4"), ("bx", "<f4"), ("by", "<f4"), ("classes", "<u4", (4,))])
SCENE_DTYPE = np.dtype([("zone", ZONE_DTYPE, (8,)), ("line", LINE_DTYPE, (8,)), ("nzones", "<i4"), ("nlines", "<i4"), ("anchor", "<i4"), ("reserved", "<i4")])
SLOT_DTYPE = np.dtype([("id", "<i4"), ("px", "<f4"), ("py", "<f4"), ("inside", "<i4"), ("last", "<i4"), ("reserved", "<i4", (3,)), ("since", "<i4", (8,))])
HEADER = ("considered", "known", "fresh", "refused", "duplicate", "anonymous", "dropped", "freed", "live", "frame")
STATE_HEADER = 144
NONE, TYPE, IDS = 0, 1, 2
KNOWN, FRESH, REFUSED, DUPLICATE, ANONYMOUS = (1 << b for b in (16, 17, 18, 19, 20))
F32 = np.float32
assert (ZONE_DTYPE.itemsize, LINE_DTYPE.itemsize, SCENE_DTYPE.itemsize, SLOT_DTYPE.itemsize) == (96, 32, 1040, 64)


class Spec:
    def __init__(self, capacity, max_missed=0, identity=IDS, min_score=0.0, gate_zone=0, gate_line=0, invert=False):
        self.capacity, self.max_missed, self.identity, self.invert = capacity, max_missed, identity, bool(invert)
        self.min_score, self.gate_zone, self.gate_line = F32(min_score), int(gate_zone), int(gate_line)


class State:
    """nstreams headers { frames, live, reserved x 2, total_entered[8], total_left[8], total_fwd[8], total_back[8] } and nstreams x capacity slots;
    all zero: empty"""

    def __init__(self, nstreams, capacity, raw=None):
        self.nstreams, self.capacity = nstreams, capacity
        self.hdr = np.zeros((nstreams, 36), "<u4")
        self.slots = np.zeros((nstreams, capacity), SLOT_DTYPE)
        if raw is not None:
            raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, STATE_HEADER + 64 * capacity)
            self.hdr[:] = np.ascontiguousarray(raw[:, :STATE_HEADER]).view("<u4")
            self.slots[:] = np.ascontiguousarray(raw[:, STATE_HEADER:]).view(SLOT_DTYPE).reshape(nstreams, capacity)

    def tobytes(self):
        return b"".join(self.hdr[s].tobytes() + self.slots[s].tobytes() for s in range(self.nstreams))

    def copy(self):
        return State(self.nstreams, self.capacity, np.frombuffer(self.tobytes(), np.uint8))


def state_nbytes(nstreams, capacity):
    return nstreams * (STATE_HEADER + 64 * capacity)


def class_mask(classes=None):
    m = [0, 0, 0, 0]
    for c in classes or ():
        m[c >> 5] |= 1 << (c & 31)
    return m


def make_scene(zones=(), lines=(), anchor=0):
    """zones = [(vertices[, dwell_frames[, classes]]), ...], lines = [((ax, ay), (bx, by)[, classes]), ...] -> a SCENE_DTYPE scalar"""
    sc = np.zeros((), SCENE_DTYPE)
    sc["nzones"], sc["nlines"], sc["anchor"] = len(zones), len(lines), anchor
    for z, zn in enumerate(zones):
        v = zn[0]
        sc["zone"][z]["nverts"], sc["zone"][z]["dwell_frames"] = len(v), zn[1] if len(zn) > 1 else 0
        sc["zone"][z]["x"][:len(v)], sc["zone"][z]["y"][:len(v)] = [p[0] for p in v], [p[1] for p in v]
        sc["zone"][z]["classes"] = class_mask(zn[2] if len(zn) > 2 else None)
    for l, ln in enumerate(lines):
        sc["line"][l]["ax"], sc["line"][l]["ay"], sc["line"][l]["bx"], sc["line"][l]["by"] = ln[0][0], ln[0][1], ln[1][0], ln[1][1]
        sc["line"][l]["classes"] = class_mask(ln[2] if len(ln) > 2 else None)
    return sc


def sdiff(a, b):
    """a - b modulo 2^32, read as signed"""
    return ((int(a) - int(b) + 2 ** 31) % 2 ** 32) - 2 ** 31


def admits(mask, cls, cls_known):
    """mask: 4 words; cls: an int array -> bool array"""
    cls = np.asarray(cls, np.int64)
    if not np.asarray(mask).any():
        return np.ones(cls.shape, bool)
    if not cls_known:
        return np.zeros(cls.shape, bool)
    ok = (cls >= 0) & (cls < 128)
    c = np.where(ok, cls, 0)
    return ok & (((np.asarray(mask, np.int64)[c >> 5] >> (c & 31)) & 1) == 1)


def anchors(boxes, anchor):
    x1, y1, x2, y2 = (np.asarray(boxes[c], F32) for c in ("x1", "y1", "x2", "y2"))
    with np.errstate(all="ignore"):
        px = (x1 + x2) * F32(0.5)
        py = y2.copy() if anchor != 0 else (y1 + y2) * F32(0.5)
    assert px.dtype == np.float32 and py.dtype == np.float32
    return px, py


def inside(zone, px, py):
    """the even-odd rule for the points (px, py) (fp32 arrays) -> bool array; a zone with nverts outside 3..8 or a NaN vertex contains nothing"""
    nv = int(zone["nverts"])
    out = np.zeros(np.shape(px), bool)
    if nv < 3 or nv > 8 or np.isnan(zone["x"][:nv]).any() or np.isnan(zone["y"][:nv]).any():
        return out
    with np.errstate(all="ignore"):
        for i in range(nv):
            j = (i + 1) % nv
            xi, yi, xj, yj = F32(zone["x"][i]), F32(zone["y"][i]), F32(zone["x"][j]), F32(zone["y"][j])
            straddles = (yi > py) != (yj > py)
            d = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)
            assert d.dtype == np.float32
            out ^= straddles & ((d > 0) if yj > yi else (d < 0))
    return out


def side(ax, ay, bx, by, px, py):
    with np.errstate(all="ignore"):
        return bool((F32(bx) - F32(ax)) * (F32(py) - F32(ay)) - (F32(by) - F32(ay)) * (F32(px) - F32(ax)) > 0)


def crossing(line, p0, p1):
    """0: none, 1: forward, 2: backward"""
    a, b = (line["ax"], line["ay"]), (line["bx"], line["by"])
    s0, s1 = side(*a, *b, *p0), side(*a, *b, *p1)
    if s0 == s1 or side(*p0, *p1, *a) == side(*p0, *p1, *b):
        return 0
    return 1 if s1 else 2


def frame(hdr, slots, scene, boxes, idrow, spec, stride):
    """one frame: hdr (36 words) and slots (capacity entries) of the stream are updated in place; boxes: the record's list, already clamped; idrow:
    the record's row of ids (8 + stride ints) or None.  Returns (event row of ROW + 2 stride ints, the gated boxes)."""
    row = np.zeros(ROW + 2 * stride, "<i4")
    boxes = np.asarray(boxes, BOX_DTYPE)
    with np.errstate(invalid="ignore"):
        qual = np.nonzero(boxes["score"] >= spec.min_score)[0]
    cons, dropped = qual[:DETS], max(0, len(qual) - DETS)
    det = boxes[cons]
    nd = len(det)
    fr = int(hdr[0])
    nz, nl = max(0, min(int(scene["nzones"]), 8)), max(0, min(int(scene["nlines"]), 8))
    px, py = anchors(det, int(scene["anchor"]))
    cls_known = spec.identity != TYPE
    ident = np.zeros(nd, np.int64) if spec.identity == NONE else det["type"].astype(np.int64) if spec.identity == TYPE else np.asarray(idrow)[8 + cons].astype(np.int64)
    ins = np.zeros(nd, np.int64)
    for z in range(nz):
        ins |= (inside(scene["zone"][z], px, py) & admits(scene["zone"][z]["classes"], det["type"], cls_known)).astype(np.int64) << z
    w0, w1 = ins.copy(), np.zeros(nd, np.int64)
    ev = np.zeros((8, 4), np.int64)                                       # occupancy, entered, left, loitering
    ln = np.zeros((8, 2), np.int64)                                       # fwd, back
    for z in range(8):
        ev[z, 0] = int(((ins >> z) & 1).sum())
    owners = {}
    for j in range(nd):
        if ident[j] <= 0:
            w1[j] |= ANONYMOUS
        elif int(ident[j]) in owners:
            w1[j] |= DUPLICATE
        else:
            owners[int(ident[j])] = j
    named, unknown = set(), []
    for id_, j in sorted(owners.items()):
        hit = np.nonzero(slots["id"] == id_)[0]
        if not len(hit):
            unknown.append(j)
            continue
        q = slots[hit[0]]
        named.add(int(hit[0]))
        was = int(q["inside"]) & 0xff
        entered, left = int(ins[j]) & ~was, was & ~int(ins[j])
        p0, p1 = (q["px"], q["py"]), (px[j], py[j])
        for z in range(8):
            if (entered >> z) & 1:
                q["since"][z] = fr
        for l in range(nl):
            if admits(scene["line"][l]["classes"], det["type"][j], cls_known):
                c = crossing(scene["line"][l], p0, p1)
                if c:
                    w1[j] |= 1 << (l + 8 * (c - 1))
                    ln[l, c - 1] += 1
        loit = 0
        for z in range(nz):
            dwell = int(scene["zone"][z]["dwell_frames"])
            if (int(ins[j]) >> z) & 1 and dwell > 0 and sdiff(fr, q["since"][z]) >= dwell:
                loit |= 1 << z
        q["px"], q["py"], q["inside"], q["last"] = px[j], py[j], ins[j], fr
        w0[j] |= entered << 8 | left << 16 | loit << 24
        w1[j] |= KNOWN
        for z in range(8):
            ev[z, 1] += (entered >> z) & 1
            ev[z, 2] += (left >> z) & 1
            ev[z, 3] += (loit >> z) & 1
    freed = 0
    for s in range(len(slots)):
        q = slots[s]
        if int(q["id"]) != 0 and s not in named and sdiff(fr, q["last"]) > spec.max_missed:
            for z in range(8):
                ev[z, 2] += (int(q["inside"]) >> z) & 1
            slots[s] = np.zeros((), SLOT_DTYPE)
            freed += 1
    fresh = refused = 0
    for j in sorted(unknown):
        free = np.nonzero(slots["id"] == 0)[0]
        if not len(free):
            w1[j] |= REFUSED
            refused += 1
            continue
        q = slots[free[0]]
        q["id"], q["px"], q["py"], q["inside"], q["last"], q["reserved"] = ident[j], px[j], py[j], ins[j], fr, 0
        q["since"] = [fr if (int(ins[j]) >> z) & 1 else 0 for z in range(8)]
        w0[j] |= int(ins[j]) << 8
        w1[j] |= FRESH
        fresh += 1
        for z in range(8):
            ev[z, 1] += (int(ins[j]) >> z) & 1
    live = int((slots["id"] != 0).sum())
    hdr[0], hdr[1] = (fr + 1) % 2 ** 32, live
    for k in range(8):
        hdr[4 + k] = (int(hdr[4 + k]) + int(ev[k, 1])) % 2 ** 32
        hdr[12 + k] = (int(hdr[12 + k]) + int(ev[k, 2])) % 2 ** 32
        hdr[20 + k] = (int(hdr[20 + k]) + int(ln[k, 0])) % 2 ** 32
        hdr[28 + k] = (int(hdr[28 + k]) + int(ln[k, 1])) % 2 ** 32
    known = len(owners) - len(unknown)
    row[:10] = (nd, known, fresh, refused, int(((w1 & DUPLICATE) != 0).sum()), int(((w1 & ANONYMOUS) != 0).sum()), dropped, freed, live,
                np.array(fr, np.uint32).astype(np.int32))
    row[16:48] = ev.reshape(-1)
    row[48:64] = ln.reshape(-1)
    row[ROW + 2 * cons] = w0.astype(np.uint32).view(np.int32) if nd else []
    row[ROW + 2 * cons + 1] = w1.astype(np.uint32).view(np.int32) if nd else []
    sel = (((w0 & spec.gate_zone) | (w1 & spec.gate_line)) != 0) != spec.invert
    return row, det[sel]


def gated_record(gated, rec):
    r = np.zeros((), DETS_DTYPE)
    n = len(gated)
    r["count"], r["nfull"], r["ncand"] = min(n, MAX_DET), n, rec["ncand"]
    r["overflow"] = (int(rec["overflow"]) & 1) | (4 if n > MAX_DET else 0)
    r["box"][:min(n, MAX_DET)] = gated[:MAX_DET]
    return r


def zones(records, flat, stride, first, streams, spec, scenes, state, ids=None):
    """the whole operator.  records: DETS_DTYPE array; flat: the lists' memory as one BOX_DTYPE array, or None (the records' own boxes, stride =
    MAX_DET); first: list starts (None: t * stride); streams: one video stream per record, -1: ignored; scenes: SCENE_DTYPE array, one per stream;
    state: a State, updated in place; ids: [ntargets, 8 + stride] ints (identity IDS).
    Returns (events [ntargets, ROW + 2 stride], gated records [ntargets], gated lists [ntargets, stride])."""
    if flat is None:
        stride = MAX_DET
    n = len(records)
    events = np.zeros((n, ROW + 2 * stride), "<i4")
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
        s = streams[t]
        events[t], gb = frame(state.hdr[s], state.slots[s], scenes[s], boxes, None if ids is None else ids[t], spec, stride)
        recs[t] = gated_record(gb, r)
        lists[t, :len(gb)] = gb
    return events, recs, lists
