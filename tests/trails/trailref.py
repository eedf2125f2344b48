"""Track trails: a numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_trails_boxes_dev), one frame of one video stream at a time, in the
contract's own words:

    1. the record's list in list order: a box is considered when score >= min_score (NaN never), until DETS boxes are; the rest is `dropped`;
    2. the anchor in fp32, every operation one np.float32 operation in the stated order, then converted (toward zero, saturating, NaN -> 0);
    3. owners: the first considered box of each identity > 0; later ones are duplicates, identities <= 0 anonymous;
    4. an owner whose identity is in a slot (the lowest) is known: the anchor is appended to the ring when it moved min_move from the newest point;
    5. slots nobody named age out beyond max_missed and are zeroed, all 416 bytes;
    6. the other owners in list order take the lowest free slot, or are refused;
    7. live, frames += 1;
then the motion rows and the items of the state as it is right after the record.  Wherever a slot's n and head are read, n is clamped to 0..points
and head taken modulo 32.

GPU results are compared with THIS, byte for byte.  tests/test_trails_abi.py pins it to a naive second implementation that keeps Python lists of points
per identity and no ring."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS = 128
ROW = 16
POINTS = 32
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])
POINT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("frame", "<i4")])
SLOT_DTYPE = np.dtype([("id", "<i4"), ("last", "<i4"), ("n", "<i4"), ("head", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("reserved", "<i4", (2,)), ("ring", POINT_DTYPE, (POINTS,))])
ITEM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("color", "u1", (4,)), ("thickness", "u1"), ("dash", "u1"), ("flags", "u1"),
                       ("reserved", "u1"), ("reserved2", "<i4", (2,))])
HEADER = ("considered", "known", "fresh", "refused", "duplicate", "anonymous", "dropped", "freed", "live", "frame", "appended", "drawn", "clipped")
STATE_HEADER = 16
NONE, TYPE, IDS = 0, 1, 2
COAST, TAPER = 1, 2
F32 = np.float32
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1
assert (POINT_DTYPE.itemsize, SLOT_DTYPE.itemsize, ITEM_DTYPE.itemsize) == (12, 416, 32)


class Spec:
    def __init__(self, capacity, max_missed=0, identity=IDS, min_score=0.0, anchor=0, points=POINTS, min_move=0, thickness=1, coast=False, taper=False,
                 coast_dash=0, color=(0, 0, 0), palette=None):
        self.capacity, self.max_missed, self.identity, self.anchor, self.points, self.min_move = capacity, max_missed, identity, anchor, points, min_move
        self.thickness, self.coast, self.taper, self.coast_dash, self.color, self.palette = thickness, bool(coast), bool(taper), coast_dash, tuple(color), palette
        self.min_score = F32(min_score)

    def colour(self, ident):
        c = self.color if self.palette is None else self.palette[int(ident) % len(self.palette)]        # (Python's %: the non-negative remainder)
        return (int(c[0]), int(c[1]), int(c[2]), 0)


class State:
    """nstreams headers { frames, live, reserved x 2 } and nstreams x capacity slots; all zero: empty"""

    def __init__(self, nstreams, capacity, raw=None):
        self.nstreams, self.capacity = nstreams, capacity
        self.hdr = np.zeros((nstreams, 4), "<i4")
        self.slots = np.zeros((nstreams, capacity), SLOT_DTYPE)
        if raw is not None:
            raw = np.ascontiguousarray(raw, np.uint8).reshape(nstreams, STATE_HEADER + 416 * capacity)
            self.hdr[:] = np.ascontiguousarray(raw[:, :STATE_HEADER]).view("<i4")
            self.slots[:] = np.ascontiguousarray(raw[:, STATE_HEADER:]).view(SLOT_DTYPE).reshape(nstreams, capacity)

    def tobytes(self):
        return b"".join(self.hdr[s].tobytes() + self.slots[s].tobytes() for s in range(self.nstreams))

    def copy(self):
        return State(self.nstreams, self.capacity, np.frombuffer(self.tobytes(), np.uint8))


def state_nbytes(nstreams, capacity):
    return nstreams * (STATE_HEADER + 416 * capacity)


def sdiff(a, b):
    """a - b modulo 2^32, read as signed"""
    return ((int(a) - int(b) + 2 ** 31) % 2 ** 32) - 2 ** 31


def sat(v):
    return max(IMIN, min(IMAX, int(v)))


def f2i(v):
    """the draw contract's conversion of one fp32: toward zero, saturating, NaN -> 0"""
    v = F32(v)
    if np.isnan(v):
        return 0
    if v >= F32(2147483648.0):
        return IMAX
    if v <= F32(-2147483648.0):
        return IMIN
    return int(v)


def anchors(boxes, anchor):
    """the converted anchors of the boxes: two int lists"""
    x1, y1, x2, y2 = (np.asarray(boxes[c], F32) for c in ("x1", "y1", "x2", "y2"))
    with np.errstate(all="ignore"):
        px = (x1 + x2) * F32(0.5)
        py = y2.copy() if anchor != 0 else (y1 + y2) * F32(0.5)
    assert px.dtype == np.float32 and py.dtype == np.float32
    return [f2i(v) for v in px], [f2i(v) for v in py]


def window(q, points):
    """what is read of a slot's n and head"""
    return max(0, min(int(q["n"]), points)), int(q["head"]) % POINTS


def make_item(x0, y0, x1, y1, color, thickness, dash=0):
    it = np.zeros((), ITEM_DTYPE)
    it["x0"], it["y0"], it["x1"], it["y1"], it["thickness"], it["dash"] = sat(x0), sat(y0), sat(x1), sat(y1), thickness, dash
    it["color"] = color
    return it


def compose(slots, fr, spec, nitems):
    """the nitems item slots of a record from the stream's slots right after it; returns (items, drawn, clipped)"""
    P = spec.points
    items = np.zeros(nitems, ITEM_DTYPE)
    drawn = clipped = 0
    for q in slots:
        n, head = window(q, P)
        if int(q["id"]) == 0 or n < 1 or not (int(q["last"]) == fr or spec.coast):
            continue
        if (drawn + 1) * P > nitems:
            clipped += 1
            continue
        reg = items[drawn * P:(drawn + 1) * P]
        drawn += 1
        col = spec.colour(q["id"])
        dash = spec.coast_dash if int(q["last"]) != fr else 0
        pt = [q["ring"][(head + j) % POINTS] for j in range(n)]
        for j in range(n - 1):
            T = 1 + ((spec.thickness - 1) * (j + 1)) // n if spec.taper else spec.thickness
            reg[j] = make_item(pt[j]["x"], pt[j]["y"], pt[j + 1]["x"], pt[j + 1]["y"], col, T, dash)
        reg[P - 1] = make_item(pt[-1]["x"], pt[-1]["y"], q["cx"], q["cy"], col, spec.thickness, dash)
    return items, drawn, clipped


def frame(hdr, slots, boxes, idrow, spec, stride, nitems):
    """one frame: hdr (4 ints) and slots (capacity entries) of the stream are updated in place; boxes: the record's list, already clamped; idrow: the
    record's row of ids (8 + stride ints) or None.  Returns (row of ROW + 4 stride ints, nitems items)."""
    row = np.zeros(ROW + 4 * stride, "<i4")
    boxes = np.asarray(boxes, BOX_DTYPE)
    with np.errstate(invalid="ignore"):
        qual = np.nonzero(boxes["score"] >= spec.min_score)[0]
    cons, dropped = qual[:DETS], max(0, len(qual) - DETS)
    det = boxes[cons]
    nd = len(det)
    fr = int(hdr[0])                                                       # (as a signed int: what a slot's `last` and a point's frame hold)
    P = spec.points
    ax, ay = anchors(det, spec.anchor)
    ident = [int(v) for v in (det["type"] if spec.identity == TYPE else np.asarray(idrow)[8 + cons])]
    owners, ndup, nanon = {}, 0, 0
    for j in range(nd):
        if ident[j] <= 0:
            nanon += 1
        elif ident[j] in owners:
            ndup += 1
        else:
            owners[ident[j]] = j
    named, unknown, appended, holder = set(), [], 0, {}
    for id_, j in owners.items():
        hit = np.nonzero(slots["id"] == id_)[0]
        if not len(hit):
            unknown.append(j)
            continue
        s = int(hit[0])
        q = slots[s]
        named.add(s)
        holder[j] = s
        n, head = window(q, P)
        move = True
        if n > 0:
            N = q["ring"][(head + n - 1) % POINTS]
            move = max(abs(ax[j] - int(N["x"])), abs(ay[j] - int(N["y"]))) >= spec.min_move
        if move:
            if n == P:
                head = (head + 1) % POINTS
            else:
                n += 1
            q["ring"][(head + n - 1) % POINTS] = (ax[j], ay[j], fr)
            appended += 1
        q["n"], q["head"], q["cx"], q["cy"], q["last"] = n, head, ax[j], ay[j], fr
    freed = 0
    for s in range(len(slots)):
        q = slots[s]
        if int(q["id"]) != 0 and s not in named and sdiff(fr, q["last"]) > spec.max_missed:
            slots[s] = np.zeros((), SLOT_DTYPE)
            freed += 1
    fresh = refused = 0
    for j in sorted(unknown):
        free = np.nonzero(slots["id"] == 0)[0]
        if not len(free):
            refused += 1
            continue
        s = int(free[0])
        slots[s] = np.zeros((), SLOT_DTYPE)
        q = slots[s]
        q["id"], q["last"], q["n"], q["head"], q["cx"], q["cy"] = ident[j], fr, 1, 0, ax[j], ay[j]
        q["ring"][0] = (ax[j], ay[j], fr)
        holder[j] = s
        fresh += 1
    live = int((slots["id"] != 0).sum())
    for j, s in holder.items():
        q = slots[s]
        n, head = window(q, P)
        O = q["ring"][head]
        row[ROW + 4 * cons[j]:ROW + 4 * cons[j] + 4] = (n, sat(int(q["cx"]) - int(O["x"])), sat(int(q["cy"]) - int(O["y"])), sdiff(fr, O["frame"]))
    items, drawn, clipped = compose(slots, fr, spec, nitems)
    row[:13] = (nd, len(owners) - len(unknown), fresh, refused, ndup, nanon, dropped, freed, live, fr, appended, drawn, clipped)
    hdr[0], hdr[1] = np.array((fr + 1) % 2 ** 32, np.uint32).astype(np.int32), live
    return row, items


def trails(records, flat, stride, first, streams, spec, state, ids=None, nitems=0):
    """the whole operator.  records: DETS_DTYPE array; flat: the lists' memory as one BOX_DTYPE array, or None (the records' own boxes, stride =
    MAX_DET); first: list starts (None: t * stride); streams: one video stream per record, -1: ignored; state: a State, updated in place; ids:
    [ntargets, 8 + stride] ints (identity IDS); nitems: the item slots written per record.
    Returns (rows [ntargets, ROW + 4 stride], items [ntargets, nitems])."""
    if flat is None:
        stride = MAX_DET
    n = len(records)
    rows = np.zeros((n, ROW + 4 * stride), "<i4")
    items = np.zeros((n, nitems), ITEM_DTYPE)
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
        rows[t], items[t] = frame(state.hdr[s], state.slots[s], boxes, None if ids is None else ids[t], spec, stride, nitems)
    return rows, items
