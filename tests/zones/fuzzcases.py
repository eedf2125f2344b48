"""The seeded cases of the zones fuzz (tests/zones/test_gpu_fuzz_input.py) and the conditions that keep it from passing vacuously.  The cases are made
here, on the CPU and before any device call: the inputs, the arena of seeded random bytes (64 guard bytes around state, events, gated records and gated
lists) and what zoneref makes of them from the empty state -- so tests/test_zones_abi.py can hold the conditions against zoneref alone.

A parametrisation is a capacity (1, 2, 128); each has the same kinds of call: one stream x 9 frames with lists of 0, 1, 127, 128, 129, 255, 256, 257
boxes; 5 streams x 1 frame with list_first given and permuted; 131 records (two launches, streams spanning the boundary, ignored entries); the
records' own boxes with claimed counts out of range; claimed list lengths out of range."""
import numpy as np

from zones import zoneref

BOX, DETS, SCENE = zoneref.BOX_DTYPE, zoneref.DETS_DTYPE, zoneref.SCENE_DTYPE
GUARD = 64
F32 = np.float32
NAN, INF = float("nan"), float("inf")
CAPACITIES = (1, 2, 128)
EXTENT = 48                                                                        # the pictures' coordinates: 0 .. EXTENT, integers


def rand_scene(rng, k):
    """zones and lines on the integer grid over the picture; counts 0, 8 and out of range, nverts 0, 2, 3, 8 and out of range, NaN / Inf sprinkled in"""
    sc = np.frombuffer(rng.integers(0, 256, SCENE.itemsize, dtype=np.uint8).tobytes(), SCENE).copy()[0]     # unused bytes are junk
    sc["nzones"] = (8, 8, 11, 3, 0, -3)[k % 6]
    sc["nlines"] = (8, 12, 8, 2, -1, 0)[k % 6]
    sc["anchor"] = (0, 1, 7, 0, 1)[k % 5]
    for z in range(8):
        zn = sc["zone"][z]
        nv = (4, 3, 8, 5, 0, 2, 8, 9)[(z + k) % 8]
        zn["nverts"] = nv
        cx, cy = rng.integers(8, EXTENT - 8, 2)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 8))
        rad = rng.integers(6, 30, 8)
        zn["x"], zn["y"] = np.round(cx + rad * np.cos(ang)), np.round(cy + rad * np.sin(ang))
        if z % 3 == 2:
            zn["x"][:4], zn["y"][:4] = (0, EXTENT, EXTENT, 0), (0, 0, EXTENT // 2 + z, EXTENT // 2 + z)     # a plain rectangle over half the picture
        zn["dwell_frames"] = (1, 2, 0, 1)[z % 4]
        zn["classes"] = zoneref.class_mask(None if z % 2 == 0 else [0, 1, 3][:1 + z % 3])
        if rng.random() < 0.08:
            zn["x" if rng.random() < 0.5 else "y"][int(rng.integers(0, 8))] = (NAN, INF, -INF)[int(rng.integers(0, 3))]
    for l in range(8):
        ln = sc["line"][l]
        if l % 2 == 0:                                                            # long lines through the middle, both directions
            v = int(rng.integers(8, EXTENT - 8))
            pts = ((-8, v), (EXTENT + 8, v)) if l % 4 == 0 else ((v, EXTENT + 8), (v, -8))
        else:
            pts = (tuple(rng.integers(0, EXTENT, 2)), tuple(rng.integers(0, EXTENT, 2)))
        ln["ax"], ln["ay"], ln["bx"], ln["by"] = pts[0][0], pts[0][1], pts[1][0], pts[1][1]
        ln["classes"] = zoneref.class_mask(None if l % 3 else [1, 2])
        if rng.random() < 0.05:
            ln["ax"] = NAN
    return sc


def video(rng, nframes, counts, type_is_id=False, weird=0.02):
    """nframes lists of one stream and their identities: objects that persist in a stable order and move a few pixels per frame (so they enter, leave,
    cross and loiter), now and then missing; identities repeated (duplicates), zero and negative (anonymous); scores on a grid of eighths"""
    nobj = max(counts) + 4
    pos = rng.integers(4, EXTENT - 4, (nobj, 2)).astype(np.float64)
    size = rng.integers(2, 12, (nobj, 2))
    cls = rng.choice([0, 1, 2, 3, 3, -1, 130], nobj)
    lists, idents = [], []
    for f in range(nframes):
        n = counts[f % len(counts)]
        pos += rng.integers(-7, 8, pos.shape)
        pos = np.clip(pos, -4, EXTENT + 4)
        who = [k for k in range(nobj) if rng.random() < 0.85][:n]
        who += list(rng.integers(0, nobj, n - len(who)))                           # (filled up with repeats: duplicates)
        b, ids = np.zeros(n, BOX), np.zeros(n, np.int64)
        for k, o in enumerate(who):
            ids[k] = o + 1
            b[k] = (cls[o], F32(rng.integers(0, 9)) / F32(8), pos[o, 0] - size[o, 0], pos[o, 1] - size[o, 1], pos[o, 0] + size[o, 0], pos[o, 1] + size[o, 1])
            r = rng.random()
            if r < 0.06:
                ids[k] = (0, -ids[k])[int(rng.integers(0, 2))]
            if rng.random() < weird:
                b[k][("x1", "y1", "x2", "y2", "score")[int(rng.integers(0, 5))]] = (NAN, INF, -INF, 1e30)[int(rng.integers(0, 4))]
        if type_is_id:
            b["type"] = ids
        lists.append(b)
        idents.append(ids)
    return lists, idents


class Case:
    """one sequence of records over some video streams: the arena, the inputs, and what zoneref makes of them from the empty state"""

    def __init__(self, seed, nstreams, spec, streams, lists, idents, use_records=False, first_given=False, claimed=None, with_lists_out=True, with_out=True, what=""):
        rng = self.rng = np.random.default_rng(seed)
        self.nstreams, self.spec, self.streams, self.use_records, self.what = nstreams, spec, list(streams), use_records, what
        n = self.n = len(streams)
        self.stride = 128 if use_records else max(1, max(len(b) for b in lists)) + 3
        self.scenes = np.array([rand_scene(rng, seed + s) for s in range(nstreams)], SCENE)
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
                    self.flat[f0 + len(b):f0 + self.stride] = video(rng, 1, [self.stride - len(b)])[0][0]
        self.ids = None
        if spec.identity == zoneref.IDS:                                          # rows as ffgpu_track_boxes_dev lays them out; junk in the header and behind the list
            self.ids = rng.integers(-5, 40, (n, 8 + self.stride)).astype("<i4")
            for t, v in enumerate(idents):
                self.ids[t, 8:8 + min(len(v), self.stride)] = v[:self.stride]
        self.ar_size = 0
        self.state_off = self._alloc(zoneref.state_nbytes(nstreams, spec.capacity), 16)
        self.ev_off = self._alloc(4 * n * (zoneref.ROW + 2 * self.stride), 4)
        self.rec_off = self._alloc(DETS.itemsize * n, 4) if with_out else None
        self.list_off = self._alloc(24 * n * self.stride, 4) if with_out and with_lists_out else None
        self.ar_size += GUARD
        self.start = rng.integers(0, 256, self.ar_size, dtype=np.uint8)
        self.start[self.state_off:self.state_off + zoneref.state_nbytes(nstreams, spec.capacity)] = 0          # the empty state
        st = zoneref.State(nstreams, spec.capacity)
        self.events, self.orecs, self.olists = zoneref.zones(self.recs, self.flat, self.stride, self.first, self.streams, spec, self.scenes, st, self.ids)
        self.state = st
        self.want = self.start.copy()
        self._put(self.state_off, np.frombuffer(st.tobytes(), np.uint8))
        self._put(self.ev_off, self.events)
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
        r = [("state", self.state_off, zoneref.state_nbytes(self.nstreams, self.spec.capacity)), ("events", self.ev_off, 4 * self.n * (zoneref.ROW + 2 * self.stride))]
        if self.rec_off is not None:
            r.append(("gated records", self.rec_off, DETS.itemsize * self.n))
        if self.list_off is not None:
            r.append(("gated lists", self.list_off, 24 * self.n * self.stride))
        return r

    def float_words(self):
        """a bool per arena byte: it belongs to an fp32 a NaN may reach (the slots' px, py; the gated boxes): compared as a NaN pattern, not by payload"""
        m = np.zeros(self.ar_size, bool)
        one = zoneref.STATE_HEADER + 64 * self.spec.capacity
        for s in range(self.nstreams):
            for k in range(self.spec.capacity):
                o = self.state_off + s * one + zoneref.STATE_HEADER + 64 * k
                m[o + 4:o + 12] = True
        for name, off, nb in self.regions()[2:]:
            m[off:off + nb] = True
        return m

    def stats(self):
        """what the case shows, summed over its records"""
        ev = self.events
        hs = {k: int(ev[:, i].sum()) for i, k in enumerate(zoneref.HEADER)}
        z = ev[:, 16:48].reshape(-1, 8, 4).sum(axis=(0, 1))
        ln = ev[:, 48:64].reshape(-1, 8, 2).sum(axis=(0, 1))
        hs.update(occupancy=int(z[0]), entered=int(z[1]), left=int(z[2]), loitering=int(z[3]), fwd=int(ln[0]), back=int(ln[1]))
        live = [t for t in range(self.n) if self.streams[t] >= 0]
        hs["gated_nonempty"] = sum(int(self.orecs[t]["nfull"]) > 0 for t in live)
        hs["gated_nonfull"] = sum(int(self.orecs[t]["nfull"]) < int(ev[t, 0]) for t in live)
        hs["nan_px"] = int(np.isnan(self.state.slots["px"]).sum() + np.isnan(self.state.slots["py"]).sum())
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


# one generator seed per capacity: the first from 5600, 5610, 5620 on whose cases meet check_stats on zoneref alone
SEEDS = {1: 5600, 2: 5610, 128: 5620}
NAMES = ("frames", "streams", "records 131", "own boxes", "clamped lists")
_CASES = {}


def fuzz_cases(cap, seed=None):
    """one parametrisation's calls: {name: Case}"""
    key = (cap, seed)
    if key in _CASES:
        return _CASES[key]
    seed = SEEDS[cap] if seed is None else seed
    S, c = zoneref.Spec, {}
    inside_any, events_any = 0xff, 0xffffff00
    # 1 stream x 9 frames: every list length at which the compaction takes another path; identity from ids; gate: inside any zone
    rng = np.random.default_rng(seed)
    lists, idents = video(rng, 9, [0, 1, 127, 128, 129, 255, 256, 257, 6])
    c["frames"] = Case(seed + 1, 1, S(cap, max_missed=1, identity=zoneref.IDS, min_score=0.25, gate_zone=inside_any), [0] * 9, lists, idents, what="cap %d, 1 x 9 frames" % cap)
    # 5 streams x 1 frame, twice over (the second frame makes them known): list_first given and permuted; identity from type; no output lists;
    # gate: everybody who did NOT cross a line or cause a zone event
    per = [video(rng, 2, [int(rng.integers(3, 12))], type_is_id=True) for _ in range(5)]
    streams, lists, idents = [0, 1, 2, 3, 4] * 2, [per[s][0][f] for f in (0, 1) for s in range(5)], [per[s][1][f] for f in (0, 1) for s in range(5)]
    c["streams"] = Case(seed + 2, 5, S(cap, max_missed=0, identity=zoneref.TYPE, gate_zone=events_any, gate_line=0xffff, invert=True), streams, lists, idents,
                        first_given=True, with_lists_out=False, what="cap %d, 5 streams, list_first" % cap)
    # 131 records: two launches, the streams span the boundary, ignored entries in both
    nfr = [40, 44, 41]
    per = [video(rng, nfr[s], [int(rng.integers(0, 9)) for _ in range(3)]) for s in range(3)]
    streams, lists, idents = interleave(rng, [p[0] for p in per], [p[1] for p in per], 6)
    assert len(streams) == 131
    c["records 131"] = Case(seed + 3, 3, S(cap, max_missed=2, identity=zoneref.IDS, gate_line=0xffff | zoneref.FRESH), streams, lists, idents, what="cap %d, 131 records" % cap)
    # the records' own boxes, counts outside their range; no identity (geometry only: everybody anonymous); no gated record at all
    lists, idents = video(rng, 5, [128, 100, 9])
    c["own boxes"] = Case(seed + 4, 2, S(cap, max_missed=1, identity=zoneref.NONE, min_score=0.125), [0, 1, 0, -1, 1], lists, idents, use_records=True,
                          claimed={0: 129, 1: -7, 4: 2 ** 31 - 1}, with_out=False, what="cap %d, own boxes" % cap)
    # claimed list lengths outside their range are clamped to [0, stride]
    lists, idents = video(rng, 6, [20, 18, 22], weird=0.1)
    c["clamped lists"] = Case(seed + 5, 2, S(cap, max_missed=1, identity=zoneref.IDS, gate_zone=inside_any << 8, invert=True), [0, 0, 1, 0, 1, 1], lists, idents,
                              claimed={0: -1, 1: 2 ** 31 - 1, 2: -2 ** 31, 3: 26, 4: 1000}, what="cap %d, clamped nfull" % cap)
    assert tuple(c) == NAMES
    _CASES[key] = c
    return c


SHOWN = ("entered", "left", "fwd", "back", "loitering", "fresh", "refused", "duplicate", "anonymous", "freed", "dropped", "known", "gated_nonempty", "gated_nonfull")


def check_stats(cases):
    """one parametrisation's cases together show every event, every kind of box, a non-empty and a non-full gated record, every clamp of the scene"""
    total = {}
    for c in cases.values():
        for k, v in c.stats().items():
            total[k] = total.get(k, 0) + v
    assert all(total[k] > 0 for k in SHOWN), {k: total[k] for k in SHOWN}
    fr = cases["frames"].events
    assert int(fr[:, 6].max()) > 0 and int(fr[:, 0].max()) == 128
    return total
