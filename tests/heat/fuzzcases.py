"""The seeded cases of the heat fuzz (tests/heat/test_gpu_fuzz_input.py) and what each of them shows.  The cases are made here, on the CPU and before any
device call: the inputs, the arena of seeded random bytes (64 guard bytes around every region) and what heatref makes of them -- so
tests/test_heat_abi.py can hold the conditions that keep the fuzz from passing vacuously against heatref alone.  Every case carries `trace`, the counts
heatref kept while it made the expected bytes.

Accumulate (ACC_NAMES): grids 1 x 1, 3 x 2, 17 x 5 and 128 x 128; cell_log2 1, 3, 6, 8; both footprints; spread 0, 1, 4; decay_shift 0, 1, 4, 16; gain 1
and 65536; 1 to 3 streams of 0 to 9 records, -1 entries; lists of 0 to 7 boxes with NaN, infinite and inverted ones and one of 300; list_first; clamped
counts; a NaN min_score; a class table; 65 records in one call; a state of random bytes; cells that saturate.
Blend (BLEND_NAMES x FORMATS): targets 1 x 1, 2 x 3, 5 x 4, 63 to 66 wide and high and 129 x 70 at odd addresses with row padding; grids smaller and
larger than the target; cell_log2 1, 3, 6, 8; both samplings; floors 0, 1, 128; RAMP_ALPHA; a caller's palette and the built-in one; skipped targets,
stream -1 and 65 targets in one call; a state of random bytes."""
import functools

import numpy as np

from heat import heatref

BOX, DETS = heatref.BOX_DTYPE, heatref.DETS_DTYPE
GUARD = 64
F32 = np.float32
NAN, INF = float("nan"), float("inf")
FORMATS = ("bgr", "nv12")


class Arena:
    def __init__(self):
        self.size, self.regs = 0, []

    def alloc(self, name, nbytes, align, odd=False):
        off = -(-(self.size + GUARD) // align) * align + (1 if odd else 0)
        self.size = off + nbytes
        self.regs.append((name, off, nbytes))
        return off

    def fill(self, rng):
        return rng.integers(0, 256, self.size + GUARD, dtype=np.uint8)


def put(buf, off, a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf[off:off + len(raw)] = raw


def rand_boxes(rng, n, ew, eh, weird=0.1):
    """n boxes round an extent of ew x eh: corners on a grid of halves, some beyond the extent, scores on a grid of eighths, types 0..4; now and then a
    NaN, an infinity, 1e30, or a box whose corners are the wrong way round"""
    b = np.zeros(n, BOX)
    for k in range(n):
        cx, cy = rng.integers(-2 * ew // 8 - 4, 2 * (ew + ew // 8) + 8) / 2, rng.integers(-2 * eh // 8 - 4, 2 * (eh + eh // 8) + 8) / 2
        hw, hh = rng.integers(0, max(2, ew // 2)) / 2, rng.integers(0, max(2, eh // 2)) / 2
        b[k] = (int(rng.integers(0, 5)), F32(rng.integers(0, 9)) / F32(8), cx - hw, cy - hh, cx + hw, cy + hh)
        r = rng.random()
        if r < weird:
            b[k][("x1", "y1", "x2", "y2", "score")[int(rng.integers(0, 5))]] = (NAN, INF, -INF, 1e30)[int(rng.integers(0, 4))]
        elif r < 2 * weird:
            b[k]["x1"], b[k]["x2"] = b[k]["x2"] + 1, b[k]["x1"]
    return b


def box(x1, y1, x2, y2, type_=0, score=1.0):
    return np.array([(type_, score, x1, y1, x2, y2)], BOX)


class AccCase:
    """one sequence of records over some video streams: the arena (state, rows), the inputs, and what heatref makes of them from the state the arena
    starts with"""

    def __init__(self, seed, nstreams, spec, streams, lists, first_given=False, own_boxes=False, state=None, counts=None, what=""):
        rng = np.random.default_rng(seed)
        self.nstreams, self.spec, self.streams, self.what = nstreams, spec, list(streams), what
        n = self.n = len(streams)
        self.stride = heatref.MAX_DET if own_boxes else max(1, max(len(b) for b in lists)) + 3
        self.recs = np.zeros(n, DETS)
        for t, b in enumerate(lists):
            r = self.recs[t]
            r["count"], r["nfull"], r["ncand"], r["overflow"] = min(len(b), 128), len(b), len(b) + t, int(rng.integers(0, 8))
            r["box"][:min(len(b), 128)] = b[:128]
        for t, v in (counts or {}).items():                                       # (counts the kernel has to clamp)
            self.recs[t]["count" if own_boxes else "nfull"] = v
        order = list(rng.permutation(n)) if first_given else list(range(n))
        self.first = [int(s) * self.stride + int(s) % 3 for s in order] if first_given else None
        self.flat = None
        if not own_boxes:
            self.flat = rand_boxes(rng, n * self.stride + 3, 64, 64, 0.3)          # (slots behind a list hold boxes, too: read only by a clamped count)
            for t, b in enumerate(lists):
                f0 = self.first[t] if first_given else t * self.stride
                self.flat[f0:f0 + len(b)] = b
        ar = Arena()
        nstate = heatref.state_nbytes(nstreams, spec.gw, spec.gh)
        self.state_off = ar.alloc("state", nstate, 16)
        self.row_off = ar.alloc("rows", 4 * n * heatref.ROW, 4)
        self._regs = ar.regs
        self.start = ar.fill(rng)
        if state != "junk":
            self.start[self.state_off:self.state_off + nstate] = 0                # the empty state
        st = heatref.State(nstreams, spec.gw, spec.gh, self.start[self.state_off:self.state_off + nstate])
        if callable(state):
            state(st, rng)
            self.start[self.state_off:self.state_off + nstate] = st.raw.reshape(-1)
        self.state0 = st.copy()
        self.trace = {}
        self.rows = heatref.accumulate(self.recs, self.flat, self.stride, self.first, self.streams, spec, st, self.trace)
        self.state = st
        self.want = self.start.copy()
        put(self.want, self.state_off, st.raw)
        put(self.want, self.row_off, self.rows)
        self.grid_changed = st.cells.tobytes() != self.state0.cells.tobytes()

    def regions(self):
        return self._regs


def _acc_cases():
    S = heatref.Spec
    rng = np.random.default_rng(7100)
    cases = {}

    def lists_for(sizes, ew, eh, extra=None):
        ls = [rand_boxes(rng, s, ew, eh) for s in sizes]
        for t, b in (extra or {}).items():
            ls[t] = np.concatenate([b, ls[t]]) if len(ls[t]) else b
        return ls

    # 1 x 1 cells of 256 pixels: every spread reaches over the grid's edge
    cases["grid 1x1"] = AccCase(7101, 1, S(1, 1, 8, heatref.ANCHOR, 0, 4, 65536, 1), [0] * 9, lists_for([0, 1, 2, 3, 4, 5, 6, 7, 2], 256, 256), what="grid 1x1")
    # 3 x 2 cells of 8: the BOX footprint, a class table, list_first, three streams and ignored entries
    span, clipped, away, inverted = box(2, 1, 20, 12), box(-5, -3, 30, 9), box(40, 2, 50, 9), box(9, 3, 4, 8)
    streams = [0, 1, -1, 2, 0, 0, -1, 1, 2, 0, 1, 0]
    cases["grid 3x2 box"] = AccCase(7102, 3, S(3, 2, 3, heatref.BOX, 0, 0, 1, 0, 0.25, classes=[1, 0, 1, 1]), streams,
                                    lists_for([3, 0, 2, 5, 7, 1, 4, 6, 2, 3, 0, 5], 24, 16, {0: span, 3: clipped, 4: away, 7: inverted}), first_given=True, what="grid 3x2 box")
    # 17 x 5 cells of 2, bottom anchors: both sides of a cell border, a negative anchor, one beyond the extent; gain 1 decays to 0 in the next frame;
    # stream 2 has no record at all
    edge = np.concatenate([box(4, 1, 6, 3), box(5, 1, 7, 3), box(-8, 1, 2, 3), box(30, 1, 50, 3), box(3, 1, 4, 30)])
    cases["grid 17x5 anchor"] = AccCase(7103, 3, S(17, 5, 1, heatref.ANCHOR, 1, 1, 1, 4), [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0],
                                        lists_for([5, 0, 2, 7, 0, 3, 1, 0, 4, 6, 2], 34, 10, {0: edge}), what="grid 17x5 anchor")
    # 128 x 128 cells of 64: the LDS limit
    cases["grid 128x128"] = AccCase(7104, 1, S(128, 128, 6, heatref.ANCHOR, 0, 4, 65536, 16), [0, 0], lists_for([7, 5], 8192, 8192), what="grid 128x128")
    # 65 records of two streams in one call: one more than a launch takes, so the state passes through memory
    cases["records 65"] = AccCase(7105, 2, S(3, 2, 3, heatref.ANCHOR, 0, 0, 1, 1), [int(v) for v in rng.integers(0, 2, 65)],
                                  lists_for([int(v) for v in rng.integers(0, 4, 65)], 24, 16), what="records 65")
    # 130 records of three streams and ignored entries: three launches
    cases["records 130"] = AccCase(7106, 3, S(3, 2, 3, heatref.BOX, 0, 0, 65536, 4), [int(v) for v in rng.integers(-1, 3, 130)],
                                   lists_for([int(v) for v in rng.integers(0, 3, 130)], 24, 16), what="records 130")
    # a list of 300 boxes of which all qualify: a second chunk of the list walk, `dropped`
    big = rand_boxes(rng, 300, 136, 40, 0.0)
    big["score"] = 1
    cases["long list"] = AccCase(7107, 1, S(17, 5, 3, heatref.BOX, 0, 0, 65536, 0), [0, 0], [big, rand_boxes(rng, 4, 136, 40)], what="long list")
    # a state of random bytes: half of the cells have the top bit set and read as FFGPU_HEAT_MAX
    cases["junk state"] = AccCase(7108, 2, S(17, 5, 3, heatref.ANCHOR, 0, 4, 65536, 0), [1, 0, 1], lists_for([6, 3, 7], 136, 40), state="junk", what="junk state")

    def nearly_full(st, _rng):
        st.cells[:] = heatref.MAX - 3 * 65536 + 5
        st.hdr[:, 0], st.hdr[:, 1] = 2 ** 32 - 2, heatref.MAX - 3 * 65536 + 5      # (the frame counter wraps, too)
    whole = box(0, 0, 767, 511)
    cases["saturate"] = AccCase(7109, 1, S(3, 2, 8, heatref.BOX, 0, 0, 65536, 0), [0, 0, 0], [np.concatenate([whole, whole]), whole, whole], state=nearly_full, what="saturate")

    def some_heat(st, rng_):
        st.cells[:] = rng_.integers(0, 40, st.cells.shape)
    # a NaN min_score: nothing qualifies, the grid only decays
    cases["nan min_score"] = AccCase(7110, 1, S(3, 2, 6, heatref.ANCHOR, 0, 1, 7, 1, NAN), [0, 0, 0], lists_for([4, 0, 6], 192, 128), state=some_heat, what="nan min_score")
    # the records' own boxes, counts the kernel clamps: negative, above 128
    cases["own boxes"] = AccCase(7111, 2, S(17, 5, 3, heatref.ANCHOR, 0, 1, 1, 0), [0, 1, 0, 1, 0], lists_for([5, 7, 3, 6, 2], 136, 40), own_boxes=True,
                                 counts={1: -3, 2: 200}, what="own boxes")
    # full lists whose nfull lies above the stride and below 0
    cases["clamped counts"] = AccCase(7112, 1, S(3, 2, 3, heatref.BOX, 0, 0, 1, 0), [0, 0, 0], lists_for([2, 4, 3], 24, 16), counts={0: 2 ** 31 - 1, 2: -2 ** 31}, what="clamped counts")
    return cases


@functools.lru_cache(None)
def acc_cases():
    return _acc_cases()


ACC_NAMES = ("grid 1x1", "grid 3x2 box", "grid 17x5 anchor", "grid 128x128", "records 65", "records 130", "long list", "junk state", "saturate", "nan min_score",
             "own boxes", "clamped counts")


class BlendCase:
    """one blend call: the arena (the state, then every target's planes at odd addresses with row padding), and what heatref makes of it.
    targets: (w, h) or None (a skipped target); streams[t]: the stream target t shows, or -1"""

    def __init__(self, seed, fmt, bspec, nstreams, targets, streams, fill_state, what=""):
        rng = np.random.default_rng(seed)
        self.fmt, self.bspec, self.nstreams, self.targets, self.streams, self.what = fmt, bspec, nstreams, list(targets), list(streams), what
        ar = Arena()
        nstate = heatref.state_nbytes(nstreams, bspec.gw, bspec.gh)
        self.state_off = ar.alloc("state", nstate, 16)
        self.desc = []                                                            # per target: None, (off, w, h, pitch) or (off_y, off_uv, w, h, pitch_y, pitch_uv)
        for t, wh in enumerate(self.targets):
            if wh is None:
                self.desc.append(None)
                continue
            w, h = wh
            pad = int(rng.integers(0, 6))
            if fmt == "bgr":
                pitch = 3 * w + pad
                self.desc.append((ar.alloc("target %d" % t, pitch * (h - 1) + 3 * w, 4, odd=t % 2 == 0), w, h, pitch))
            else:
                py, puv = w + pad, 2 * ((w + 1) // 2) + 2 * (pad // 2)
                oy = ar.alloc("target %d y" % t, py * (h - 1) + w, 4, odd=t % 2 == 0)
                ouv = ar.alloc("target %d uv" % t, puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2) + 2, 4) + 2 * (t % 2)   # (2-byte aligned, not always 4)
                self.desc.append((oy, ouv, w, h, py, puv))
        self._regs = ar.regs
        self.start = ar.fill(rng)
        st = heatref.State(nstreams, bspec.gw, bspec.gh, self.start[self.state_off:self.state_off + nstate])
        fill_state(st, rng)
        self.start[self.state_off:self.state_off + nstate] = st.raw.reshape(-1)
        self.state = st
        self.trace = {}
        self.want = self.start.copy()
        self.apply(self.want, self.trace)
        self.inside_unchanged = self._inside_unchanged()

    def apply(self, buf, trace=None):
        for d, s in zip(self.desc, self.streams):
            if d is None or s < 0:
                continue
            if self.fmt == "bgr":
                heatref.blend_bgr(buf, d[0], d[1], d[2], d[3], self.state.hdr[s], self.state.cells[s], self.bspec, trace)
            else:
                heatref.blend_nv12(buf, d[0], d[1], d[2], d[3], d[4], d[5], self.state.hdr[s], self.state.cells[s], self.bspec, trace)

    def _inside_unchanged(self):
        """some luma / BGR pixel inside the extent of a blended target is as it was"""
        ew, eh = self.bspec.gw << self.bspec.cell_log2, self.bspec.gh << self.bspec.cell_log2
        for d, s in zip(self.desc, self.streams):
            if d is None or s < 0:
                continue
            off, w, h, pitch, bpp = (d[0], d[1], d[2], d[3], 3) if self.fmt == "bgr" else (d[0], d[2], d[3], d[4], 1)
            for y in range(min(h, eh)):
                a = off + y * pitch
                same = (self.want[a:a + bpp * min(w, ew)] == self.start[a:a + bpp * min(w, ew)]).reshape(-1, bpp).all(axis=1)
                if same.any():
                    return True
        return False

    def grid_nonzero(self):
        return any(self.state.cells[s].any() for d, s in zip(self.desc, self.streams) if d is not None and s >= 0)

    def regions(self):
        return self._regs


def sparse(p, top=1000):
    def fill(st, rng):
        st.raw[:] = 0
        st.cells[:] = np.where(rng.random(st.cells.shape) < p, rng.integers(1, top, st.cells.shape), 0)
        st.cells[:, 0, 0] = top                                                    # (every stream shows something)
        st.hdr[:, 0], st.hdr[:, 1] = 9, st.cells.reshape(st.nstreams, -1).max(axis=1)
    return fill


def sparse_but_last(p):
    def fill(st, rng):
        sparse(p)(st, rng)
        st.raw[-1] = 0                                                             # the last stream: the empty state, peak 0
    return fill


def left_cell_only(st, rng):
    st.raw[:] = 0
    st.cells[:, :, 0] = 500
    st.hdr[:, 1] = 500


def junk(st, rng):
    st.hdr[0, 1] |= np.uint32(2 ** 31)                                             # the arena's random bytes as they are, but one peak surely above FFGPU_HEAT_MAX


def _blend_cases(fmt):
    B = heatref.BlendSpec
    seed = 7200 if fmt == "bgr" else 7300
    pal = np.random.default_rng(7290).integers(0, 256, (256, 3), dtype=np.uint8)
    cases = {}

    def add(k, name, *a):
        cases[name] = BlendCase(seed + k, fmt, *a, what="%s %s" % (name, fmt))
    # the smallest targets; the built-in palette, opacity 255; stream 1 is empty: automatic full_scale with peak 0
    add(1, "tiny", B(5, 4, 1, 0, 0, 255), 2, [(1, 1), (2, 3), (5, 4), (5, 4)], [0, 0, 0, 1], sparse_but_last(0.5))
    # round a block's side, SMOOTH over a grid of 8 x 8 cells of 8 pixels: i0 = -1 on the left, i0 + 1 clamped on the right, pixels beyond the extent
    add(2, "edges smooth", B(8, 8, 3, 0, 0, 200, True), 1, [(63, 66), (64, 65), (65, 64), (66, 63)], [0] * 4, sparse(0.4))
    add(3, "edges nearest", B(9, 9, 3, 600, 1, 77, False, False, pal), 1, [(63, 66), (64, 65), (65, 64), (66, 63)], [0] * 4, sparse(0.4))
    # a grid smaller than the target; opacity 1 with RAMP_ALPHA: a = 0 below level 128
    add(4, "small grid", B(3, 2, 5, 0, 1, 1, True, True), 1, [(129, 70)], [0], sparse(0.6))
    # a cell of 256 pixels is larger than a block; a fixed full_scale below the cells: levels clamped to 255; floor 128; a caller's palette
    add(5, "big cell", B(2, 1, 8, 300, 128, 140, True, False, pal), 2, [(129, 70), (66, 66)], [1, 0], sparse(0.5))
    # cells of 64: the left column hot, the rest cold -- a block wholly below the floor next to one that is not
    add(6, "cold blocks", B(3, 2, 6, 0, 0, 128), 1, [(129, 70)], [0], left_cell_only)
    add(7, "cold blocks ramp", B(3, 2, 6, 1000, 1, 255, False, True), 1, [(129, 70)], [0], left_cell_only)
    # 65 targets: two launches; skipped targets and stream -1 among them
    t65 = [(5, 4)] * 65
    t65[3] = t65[64] = None
    s65 = [k % 3 for k in range(65)]
    s65[5] = s65[63] = -1
    add(8, "targets 65", B(5, 4, 1, 0, 0, 90, True), 3, t65, s65, sparse(0.5))
    # a state of random bytes: cells and peak with the top bit set
    add(9, "junk state", B(17, 5, 3, 0, 1, 128, True, True), 2, [(66, 63), (5, 4)], [1, 0], junk)
    add(10, "junk state scaled", B(17, 5, 3, 2 ** 31 - 1, 0, 255, False), 2, [(129, 70)], [0], junk)
    return cases


@functools.lru_cache(None)
def blend_cases(fmt):
    return _blend_cases(fmt)


BLEND_NAMES = ("tiny", "edges smooth", "edges nearest", "small grid", "big cell", "cold blocks", "cold blocks ramp", "targets 65", "junk state", "junk state scaled")
