"""The seeded cases of the trails fuzz (tests/trails/test_gpu_fuzz_input.py) and the conditions that keep it from passing vacuously.  The cases are made
here, on the CPU and before any device call: the inputs, the arena of seeded random bytes (64 guard bytes around state, rows and items) and what
trailref makes of them -- so tests/test_trails_abi.py can hold the conditions against trailref alone.

A parametrisation is a capacity (1, 2, 128); each has the same kinds of call:
    ring         1 stream x 40 records in one call, points 32 (the ring wraps), three objects always seen, taper with T = 8, nitems exactly drawn x P,
                 first_item > 0;
    streams      6 streams x 8 frames interleaved with -1 entries, points 2, identity from type, list_first given and permuted, coasting slots drawn
                 dashed, max_missed 1, min_move 4, nitems no multiple of P;
    records 65   65 records of 2 streams: one more than a launch takes, so the state passes through memory; max_missed 0; no items at all;
    long lists   lists of 300 boxes of which more than 128 qualify (a second chunk of the list walk), from a state whose frame counter stands at
                 2^32 - 2; corners of NaN, +-Inf and 1e30; nitems smaller than one region;
    junk state   a state of seeded random bytes (totality): n and head out of range, ids that repeat, points anywhere."""
import numpy as np

from trails import trailref

BOX, DETS, ITEM = trailref.BOX_DTYPE, trailref.DETS_DTYPE, trailref.ITEM_DTYPE
GUARD = 64
F32 = np.float32
NAN, INF = float("nan"), float("inf")
CAPACITIES = (1, 2, 128)
EXTENT = 64                                                                        # the pictures' coordinates: 0 .. EXTENT


def video(rng, nframes, counts, nobj=None, seen=0.85, step=5, type_is_id=False, weird=0.02):
    """nframes lists of one stream and their identities: objects that persist and move up to `step` pixels per frame, now and then missing;
    identities repeated (duplicates), zero and negative (anonymous); scores on a grid of eighths; corners on a grid of halves"""
    nobj = max(counts) + 4 if nobj is None else nobj
    pos = rng.integers(4, EXTENT - 4, (nobj, 2)).astype(np.float64)
    size = rng.integers(2, 12, (nobj, 2)) / 2
    lists, idents = [], []
    for f in range(nframes):
        n = counts[f % len(counts)]
        pos += rng.integers(-step, step + 1, pos.shape)
        pos = np.clip(pos, -4, EXTENT + 4)
        who = [k for k in range(nobj) if rng.random() < seen][:n]
        who += list(rng.integers(0, nobj, n - len(who)))                           # (filled up with repeats: duplicates)
        b, ids = np.zeros(n, BOX), np.zeros(n, np.int64)
        for k, o in enumerate(who):
            ids[k] = o + 1
            b[k] = (o % 5, F32(rng.integers(0, 9)) / F32(8), pos[o, 0] - size[o, 0], pos[o, 1] - size[o, 1], pos[o, 0] + size[o, 0], pos[o, 1] + size[o, 1])
            if seen < 1 and rng.random() < 0.06:
                ids[k] = (0, -ids[k])[int(rng.integers(0, 2))]
            if rng.random() < weird:
                b[k][("x1", "y1", "x2", "y2", "score")[int(rng.integers(0, 5))]] = (NAN, INF, -INF, 1e30)[int(rng.integers(0, 4))]
        if type_is_id:
            b["type"] = ids
        lists.append(b)
        idents.append(ids)
    return lists, idents


class Case:
    """one sequence of records over some video streams: the arena, the inputs, and what trailref makes of them from the state the arena starts with"""

    def __init__(self, seed, nstreams, spec, streams, lists, idents, first_given=False, items=None, frames0=None, junk_state=False, what=""):
        rng = self.rng = np.random.default_rng(seed)
        self.nstreams, self.spec, self.streams, self.what = nstreams, spec, list(streams), what
        n = self.n = len(streams)
        self.stride = max(1, max(len(b) for b in lists)) + 3
        self.items_stride, self.first_item, self.nitems = items if items else (0, 0, 0)
        self.recs = np.zeros(n, DETS)
        for t, b in enumerate(lists):
            r = self.recs[t]
            r["count"], r["nfull"], r["ncand"], r["overflow"] = min(len(b), 128), len(b), len(b) + t, int(rng.integers(0, 8))
            r["box"][:min(len(b), 128)] = b[:128]
        order = list(rng.permutation(n)) if first_given else list(range(n))      # list t lies in slot order[t] of the lists' memory
        self.first = [int(s) * self.stride + int(s) % 3 for s in order] if first_given else None
        self.flat = np.zeros(n * self.stride + 3, BOX)
        self.flat.view(np.uint8)[:] = 0x3C                                        # (slots behind a list hold junk: never read)
        for t, b in enumerate(lists):
            f0 = self.first[t] if first_given else t * self.stride
            self.flat[f0:f0 + len(b)] = b
        self.ids = None
        if spec.identity == trailref.IDS:                                         # rows as ffgpu_track_boxes_dev lays them out; junk in the header and behind the list
            self.ids = rng.integers(-5, 40, (n, 8 + self.stride)).astype("<i4")
            for t, v in enumerate(idents):
                self.ids[t, 8:8 + len(v)] = v
        nstate = trailref.state_nbytes(nstreams, spec.capacity)
        self.ar_size = 0
        self.state_off = self._alloc(nstate, 16)
        self.row_off = self._alloc(4 * n * (trailref.ROW + 4 * self.stride), 4)
        self.items_off = self._alloc(32 * n * self.items_stride, 4) if items else None
        self.ar_size += GUARD
        self.start = rng.integers(0, 256, self.ar_size, dtype=np.uint8)
        if not junk_state:
            self.start[self.state_off:self.state_off + nstate] = 0                # the empty state
        st = trailref.State(nstreams, spec.capacity, self.start[self.state_off:self.state_off + nstate])
        if frames0 is not None:
            st.hdr[:, 0] = np.array(frames0, np.uint32).astype(np.int32)
            self.start[self.state_off:self.state_off + nstate] = np.frombuffer(st.tobytes(), np.uint8)
        self.state0 = st.copy()
        self.rows, self.items = trailref.trails(self.recs, self.flat, self.stride, self.first, self.streams, spec, st, self.ids, self.nitems)
        self.state = st
        self.want = self.start.copy()
        self._put(self.state_off, np.frombuffer(st.tobytes(), np.uint8))
        self._put(self.row_off, self.rows)
        for t in range(n if items else 0):
            self._put(self.items_off + 32 * (t * self.items_stride + self.first_item), self.items[t])

    def _alloc(self, nbytes, align):
        off = -(-(self.ar_size + GUARD) // align) * align
        self.ar_size = off + nbytes
        return off

    def _put(self, off, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.want[off:off + len(raw)] = raw

    def regions(self):
        r = [("state", self.state_off, trailref.state_nbytes(self.nstreams, self.spec.capacity)), ("rows", self.row_off, 4 * self.n * (trailref.ROW + 4 * self.stride))]
        if self.items_off is not None:
            r.append(("items", self.items_off, 32 * self.n * self.items_stride))
        return r

    def stats(self):
        """what the case shows, summed over its records"""
        rw = self.rows
        hs = {k: int(rw[:, i].sum()) for i, k in enumerate(trailref.HEADER)}
        hs["not_appended"] = hs["known"] - hs["appended"]
        hs["wrapped"] = int(((self.state.slots["id"] != 0) & (self.state.slots["head"] != 0)).sum())
        hs["dashed"] = int((self.items["dash"] != 0).sum())
        hs["thicknesses"] = max([len(set(int(v) for v in row["thickness"] if v)) for row in self.items] or [0])
        sat = (self.state.slots["cx"] == trailref.IMAX) | (self.state.slots["cx"] == trailref.IMIN) | (self.state.slots["cy"] == trailref.IMAX) | (self.state.slots["cy"] == trailref.IMIN)
        hs["saturated"] = int(sat.sum())
        fr = [int(np.uint32(v)) for t, v in enumerate(rw[:, 9]) if self.streams[t] >= 0]
        hs["frame_wraps"] = int(0xffffffff in fr and 0 in fr)
        hs["max_considered"] = int(rw[:, 0].max())
        return hs


def interleave(rng, per_stream, per_ids, ignored=0):
    """the streams' frames in one table: each stream's frames in order, the streams interleaved at random, `ignored` entries of stream -1 in between"""
    left = [len(v) for v in per_stream]
    streams, lists, idents = [], [], []
    pool = [s for s, k in enumerate(left) for _ in range(k)] + [-1] * ignored
    for s in rng.permutation(pool):
        s = int(s)
        streams.append(s)
        if s < 0:
            b, i = video(rng, 1, [5])
            lists.append(b[0])
            idents.append(i[0])
        else:
            k = len(per_stream[s]) - left[s]
            lists.append(per_stream[s][k])
            idents.append(per_ids[s][k])
            left[s] -= 1
    return streams, lists, idents


# one generator seed per capacity: the first from 5700, 5710, 5720 on whose cases meet check_stats on trailref alone
SEEDS = {1: 5700, 2: 5710, 128: 5720}
NAMES = ("ring", "streams", "records 65", "long lists", "junk state")
PALETTE = [(200, 10, 20), (30, 220, 40), (50, 60, 240), (250, 250, 5), (7, 200, 200)]
_CASES = {}


def fuzz_cases(cap, seed=None):
    """one parametrisation's calls: {name: Case}"""
    key = (cap, seed)
    if key in _CASES:
        return _CASES[key]
    seed = SEEDS[cap] if seed is None else seed
    S, c = trailref.Spec, {}
    rng = np.random.default_rng(seed)
    # 1 stream x 40 records, three objects always seen and always moving: a 32-point ring wraps; taper with T = 8; the item range is exactly the drawn regions
    lists, idents = video(rng, 40, [3], nobj=3, seen=1.0, weird=0.0)
    drawn = min(3, cap)
    c["ring"] = Case(seed + 1, 1, S(cap, max_missed=1, identity=trailref.IDS, points=32, thickness=8, taper=True, palette=PALETTE), [0] * 40, lists, idents,
                     items=(drawn * 32 + 5, 2, drawn * 32), what="cap %d, 1 x 40 records" % cap)
    # 6 streams x 8 frames and 4 ignored entries: identity from type, list_first permuted, coasting slots dashed, a point needs 4 pixels, 7 item slots for P = 2
    per = [video(rng, 8, [int(rng.integers(2, 9))], seen=0.7, type_is_id=True) for _ in range(6)]
    streams, lists, idents = interleave(rng, [p[0] for p in per], [p[1] for p in per], 4)
    c["streams"] = Case(seed + 2, 6, S(cap, max_missed=1, identity=trailref.TYPE, anchor=1, points=2, min_move=4, thickness=3, coast=True, coast_dash=3, color=(9, 8, 7)),
                        streams, lists, idents, first_given=True, items=(9, 1, 7), what="cap %d, 6 streams, list_first" % cap)
    # 65 records: two launches, both streams span the boundary; nobody survives a missed frame; no items
    per = [video(rng, k, [int(rng.integers(0, 7)) for _ in range(3)], seen=0.7) for k in (33, 31)]
    streams, lists, idents = interleave(rng, [p[0] for p in per], [p[1] for p in per], 1)
    assert len(streams) == 65
    c["records 65"] = Case(seed + 3, 2, S(cap, max_missed=0, identity=trailref.IDS, min_score=0.125, points=32, min_move=2), streams, lists, idents,
                           what="cap %d, 65 records" % cap)
    # lists of 300 boxes, more than 128 of them qualifying; the frame counter passes 2^32; hostile corners; one item slot for regions of two
    lists, idents = video(rng, 4, [300, 290, 1, 300], nobj=200, weird=0.05)
    for f, b in enumerate(lists):
        if len(b) > 8:
            b["score"][:4] = 1
            idents[f][:4] = (7, 8, 9, 10)
            b["x2"][0], b["y1"][1], b["x1"][2], b["y2"][3] = 1e30, NAN, -INF, INF
    c["long lists"] = Case(seed + 4, 1, S(cap, max_missed=1, identity=trailref.IDS, min_score=0.25, points=2, thickness=2, coast=True), [0] * 4, lists, idents,
                           items=(3, 2, 1), frames0=2 ** 32 - 2, what="cap %d, long lists" % cap)
    # a state of random bytes under two streams
    per = [video(rng, 4, [int(rng.integers(3, 9))]) for _ in range(2)]
    streams, lists, idents = interleave(rng, [p[0] for p in per], [p[1] for p in per], 0)
    c["junk state"] = Case(seed + 5, 2, S(cap, max_missed=2 ** 20, identity=trailref.IDS, points=32, min_move=1, thickness=8, coast=True, taper=True, coast_dash=6,
                                          palette=PALETTE), streams, lists, idents, items=(512, 0, 512), junk_state=True, what="cap %d, junk state" % cap)
    assert tuple(c) == NAMES
    _CASES[key] = c
    return c


SHOWN = ("known", "fresh", "refused", "duplicate", "anonymous", "dropped", "freed", "appended", "not_appended", "drawn", "clipped", "wrapped", "dashed", "saturated")


def check_stats(cases):
    """one parametrisation's cases together show every kind of box and slot event the contract names (tests/test_trails_abi.py lists them)"""
    total = {}
    for c in cases.values():
        for k, v in c.stats().items():
            total[k] = total.get(k, 0) + v
    assert all(total[k] > 0 for k in SHOWN), {k: total[k] for k in SHOWN}
    assert cases["records 65"].spec.max_missed == 0 and cases["records 65"].stats()["freed"] > 0            # freed with max_missed 0 ...
    assert cases["streams"].spec.max_missed > 0 and cases["streams"].stats()["freed"] > 0                   # ... and with max_missed > 0
    assert cases["ring"].spec.thickness == 8 and cases["ring"].stats()["thicknesses"] >= 3                  # a taper that shows
    assert cases["ring"].stats()["wrapped"] > 0 and cases["long lists"].stats()["frame_wraps"] == 1
    assert cases["long lists"].stats()["max_considered"] == 128 and cases["long lists"].stats()["dropped"] > 0
    assert cases["streams"].stats()["dashed"] > 0 and cases["long lists"].stats()["clipped"] > 0
    return total
