"""The seeded cases of the motion fuzz (tests/motion/test_gpu_fuzz_input.py) and what each of them shows.  The cases are made here, on the CPU and
before any device call: the inputs, the arena of seeded random bytes (64 guard bytes around every region) and what motionref makes of them -- so
tests/test_motion_abi.py can hold the conditions that keep the fuzz from passing vacuously against motionref alone.  Every case carries `trace`, the
counts motionref kept while it made the expected bytes.

Update (UPDATE_NAMES x FORMATS): frames 1 x 1, 7 x 5 in one partial cell of 8, 17 x 9, 67 x 35 with padded pitches at an odd address; 63, 64 and 65
wide and high (the workgroup's tile is 64 x 64) and 130 x 70; every cell_log2; NV12 with a separate uv plane that is never read; states of random
bytes with frames 0, not 0 and 2^32 - 1; |d| exactly threshold << 8 and one above; learn_shift 0, 1, 15, 16 and 18 frames after which the model has
reached the frame exactly; learn_shift_changed 16; -1 and NULL targets among live ones; 3 streams x 4 frames; 65 and 130 targets in one call.
Gate (GATE_NAMES): inverted boxes, boxes wholly outside, boxes ending on a cell boundary and one pixel past it; cover 256 and 1; min_pixels 1 and
c c; 130 qualifying boxes; NaN scores, a NaN min_score, a class list; INVERT; streams with frames 0, not warm and warm; list_first; the records' own
boxes; NULL outputs; 65 and 130 records with -1 entries; a state of random bytes; a row of 512 cells."""
import functools

import numpy as np

from heat.fuzzcases import GUARD, Arena, box, put, rand_boxes  # noqa: F401  (GUARD: for the test module)
from motion import motionref

BOX, DETS = motionref.BOX_DTYPE, motionref.DETS_DTYPE
F32 = np.float32
NAN = float("nan")
FORMATS = ("bgr", "nv12")


def gray(fmt, luma):
    """a frame's pixels with the given luma: B = G = R = y (29 + 150 + 77 = 256), or the Y plane itself"""
    luma = np.asarray(luma, np.uint8)
    return luma if fmt == "nv12" else np.repeat(luma[:, :, None], 3, axis=2)


def luma_of(fmt, img):
    return np.asarray(img).astype(np.int64) if fmt == "nv12" else motionref.luma_bgr(img)


def scene_frames(rng, fmt, w, h, n):
    """n frames of one stream: a fixed background of random pixels with +-3 of noise and a rectangle of inverted pixels that moves from frame to frame"""
    shape = (h, w) if fmt == "nv12" else (h, w, 3)
    base = rng.integers(0, 256, shape).astype(np.int64)
    out = []
    for j in range(n):
        f = np.clip(base + rng.integers(-3, 4, shape), 0, 255)
        rw, rh = max(1, w // 2), max(1, h // 2)
        x0, y0 = (3 + 5 * j) % max(1, w - rw + 1), (1 + 3 * j) % max(1, h - rh + 1)
        f[y0:y0 + rh, x0:x0 + rw] = 255 - f[y0:y0 + rh, x0:x0 + rw]
        out.append(f.astype(np.uint8))
    return out


class UpdateCase:
    """one call of the update over some video streams: the arena (state, rows, the frames), and what motionref makes of it from the state the arena
    starts with.  seq: (stream, image or None) per target; state: None (empty), "junk" (random bytes, frames as they fall) or a function of the
    State and the rng."""

    def __init__(self, seed, fmt, spec, nstreams, seq, state=None, pad=0, odd=False, what=""):
        rng = np.random.default_rng(seed)
        self.fmt, self.spec, self.nstreams, self.what = fmt, spec, nstreams, what
        w, h = spec.w, spec.h
        self.streams = [int(s) for s, _ in seq]
        n = self.n = len(seq)
        ar = Arena()
        nstate = motionref.state_nbytes(nstreams, w, h, spec.cell_log2)
        self.state_off = ar.alloc("state", nstate, 16)
        self.row_off = ar.alloc("rows", 4 * n * motionref.ROW, 4)
        self.desc, self.lumas, frames = [], [], []
        for t, (s, img) in enumerate(seq):
            if img is None:
                self.desc.append(None)
                self.lumas.append(None)
                continue
            if fmt == "bgr":
                pitch = 3 * w + pad
                off = ar.alloc("frame %d" % t, pitch * (h - 1) + 3 * w, 4, odd)
                self.desc.append((off, w, h, pitch))
                frames.append((off, pitch, np.asarray(img, np.uint8).reshape(h, 3 * w)))
            else:
                py, puv = w + pad, 2 * ((w + 1) // 2) + 2 * (pad // 2)
                off = ar.alloc("y %d" % t, py * (h - 1) + w, 4, odd)
                ouv = ar.alloc("uv %d" % t, puv * ((h + 1) // 2), 2)                 # (random bytes: never read)
                self.desc.append((off, ouv, w, h, py, puv))
                frames.append((off, py, np.asarray(img, np.uint8)))
            self.lumas.append(luma_of(fmt, img))
        self._regs = ar.regs
        self.start = ar.fill(rng)
        for off, pitch, rows in frames:
            np.lib.stride_tricks.as_strided(self.start[off:], shape=rows.shape, strides=(pitch, 1), writeable=True)[...] = rows
        if state is None:
            self.start[self.state_off:self.state_off + nstate] = 0                # the empty state
        st = motionref.State(nstreams, w, h, spec.cell_log2, self.start[self.state_off:self.state_off + nstate])
        if callable(state):
            state(st, rng)
            self.start[self.state_off:self.state_off + nstate] = st.raw.reshape(-1)
        self.state0 = st.copy()
        self.trace = {}
        self.rows = motionref.update(self.lumas, self.streams, spec, st, self.trace)
        self.state = st
        self.want = self.start.copy()
        put(self.want, self.state_off, st.raw)
        put(self.want, self.row_off, self.rows)

    def regions(self):
        return self._regs


def seeded(lumas_of_stream, frames=7):
    """a state setter: random bytes everywhere, `frames` in every header, and the left half of every stream's plane within 300 of the given luma << 8"""
    def fn(st, rng):
        st.raw[:] = rng.integers(0, 256, st.raw.shape, dtype=np.uint8)
        st.hdr[:, 0] = frames
        for s, lu in lumas_of_stream.items():
            half = st.w // 2 + 1
            st.plane[s][:, :half] = np.clip((np.asarray(lu).astype(np.int64)[:, :half] << 8) + rng.integers(-300, 301, (st.h, half)), 0, 65535).astype(np.uint16)
    return fn


def _update_cases(fmt):
    S = motionref.Spec
    rng = np.random.default_rng(8100 + (fmt == "nv12"))
    cases = {}

    def add(name, seed, spec, nstreams, seq, **kw):
        cases[name] = UpdateCase(seed, fmt, spec, nstreams, seq, what="%s %s" % (fmt, name), **kw)

    def scene(w, h, n):
        return scene_frames(rng, fmt, w, h, n)

    def inter(per_stream):
        """the streams' frames interleaved: frame j of every stream, then frame j + 1"""
        return [(s, f[j]) for j in range(max(len(f) for f in per_stream.values())) for s, f in sorted(per_stream.items()) if j < len(f)]

    # one pixel, one cell
    one = [np.full((1, 1), v, np.uint8) for v in (10, 200, 203, 90)]
    add("1x1", 8101, S(1, 1, 2, 50, 1, 0, 1), 1, [(0, gray(fmt, v)) for v in one])
    # a single partial cell of 8
    add("7x5 cell 8", 8102, S(7, 5, 3, 40, 2, 6, 3), 1, [(0, f) for f in scene(7, 5, 3)])
    add("17x9", 8103, S(17, 9, 2, 40, 3, 5, 4), 2, inter({0: scene(17, 9, 3), 1: scene(17, 9, 2)}))
    # padded pitches, the pixels at an odd address; a state of random bytes, the left half of the plane near the first frame: frames != 0
    f67 = scene(67, 35, 3)
    add("67x35 odd", 8104, S(67, 35, 3, 30, 4, 7, 20), 1, [(0, f) for f in f67], pad=5, odd=True, state=seeded({0: luma_of(fmt, f67[0])}))
    # one less than, equal to and one more than the tile, every cell size
    for name, seed, w, h, k in (("63x65", 8105, 63, 65, 4), ("64x64", 8106, 64, 64, 5), ("65x63", 8107, 65, 63, 6), ("130x70", 8108, 130, 70, 2), ("65x65", 8109, 65, 65, 3)):
        fs = scene(w, h, 2)
        add(name, seed, S(w, h, k, 35, 3, 9, max(1, (1 << (2 * k)) // 3)), 1, [(0, f) for f in fs], pad=seed % 4, odd=bool(seed & 1), state=seeded({0: luma_of(fmt, fs[0])}, 3 + seed))
    # random bytes with frames 0: everything is taken from the frame
    def frames0(st, r):
        st.raw[:] = r.integers(0, 256, st.raw.shape, dtype=np.uint8)
        st.hdr[:, 0] = 0
    add("junk frames 0", 8110, S(33, 18, 3, 25, 2, 4, 10), 2, inter({0: scene(33, 18, 2), 1: scene(33, 18, 2)}), state=frames0)
    # frames 2^32 - 1: the increment wraps, the next frame is a first frame again
    f20 = scene(20, 12, 3)
    add("wrap", 8111, S(20, 12, 2, 25, 2, 4, 3, warmup=0), 1, [(0, f) for f in f20], state=seeded({0: luma_of(fmt, f20[0])}, 2 ** 32 - 1))
    # |d| exactly threshold << 8 (not changed) and one above (changed): the plane is set from the frame
    lu = rng.integers(60, 200, (9, 24)).astype(np.int64)

    def edge(st, r):
        st.raw[:] = r.integers(0, 256, st.raw.shape, dtype=np.uint8)
        st.hdr[:, 0] = 5
        x = np.arange(24)[None, :]
        y = np.arange(9)[:, None]
        one = np.where(y < 4, 1, 0)                                               # (the rows from 4 on: at the threshold only, so their cells stay inactive)
        off = np.where(x % 4 == 0, 45 << 8, np.where(x % 4 == 1, (45 << 8) + one, np.where(x % 4 == 2, -(45 << 8), -(45 << 8) - one)))
        st.plane[0][:] = ((lu << 8) + off).astype(np.uint16)
    add("threshold edge", 8112, S(24, 9, 2, 45, 3, 5, 2), 1, [(0, gray(fmt, lu))], state=edge)
    # the learning rates: 0 (differencing), 1 for 18 frames of one picture (the model reaches it exactly), 15, 16 (nothing learnt)
    still = scene(21, 10, 1)[0]
    far = seeded({0: luma_of(fmt, still)}, 9)
    add("learn 0", 8113, S(21, 10, 3, 20, 0, 0, 5), 1, [(0, f) for f in scene(21, 10, 3)])
    add("learn 1 converges", 8114, S(21, 10, 3, 20, 1, 1, 5), 1, [(0, still)] * 18, state=far)
    add("learn 15", 8115, S(21, 10, 3, 20, 15, 15, 5), 1, [(0, still)] * 2, state=far)
    l16 = scene(21, 10, 3)
    add("learn 16", 8116, S(21, 10, 3, 20, 16, 16, 5), 1, [(0, f) for f in l16], state=seeded({0: luma_of(fmt, l16[0])}, 9))
    # a changed region frozen: the model keeps what it had there, and the region stays changed
    add("freeze changed", 8117, S(21, 10, 3, 20, 2, 16, 5), 1, [(0, still)] * 3, state=far)
    # -1 and NULL targets among live ones
    fa, fb = scene(19, 11, 3), scene(19, 11, 2)
    add("skipped", 8118, S(19, 11, 2, 30, 2, 5, 3), 3, [(0, fa[0]), (-1, fa[1]), (2, None), (1, fb[0]), (0, fa[1]), (-1, None), (1, fb[1]), (0, fa[2])])
    # 3 streams x 4 frames in one call: four rounds
    add("3 streams x 4", 8119, S(23, 13, 3, 30, 2, 5, 6), 3, inter({s: scene(23, 13, 4) for s in range(3)}))
    # 65 targets of 65 streams (two launches a round); 130 targets of 67 streams (two rounds) with skipped ones
    small = [scene(9, 5, 2) for _ in range(67)]
    add("targets 65", 8120, S(9, 5, 2, 30, 2, 5, 2), 65, [(s, small[s][0]) for s in range(65)], state=seeded({s: luma_of(fmt, small[s][0]) for s in range(65)}))
    seq = [(s, small[s][0]) for s in range(67)] + [(s, small[s][1]) for s in range(63)]
    seq[5], seq[70] = (-1, small[5][0]), (3, None)
    add("targets 130", 8121, S(9, 5, 2, 30, 2, 5, 2), 67, seq)
    return cases


@functools.lru_cache(maxsize=None)
def update_cases(fmt):
    return _update_cases(fmt)


UPDATE_NAMES = ("1x1", "7x5 cell 8", "17x9", "67x35 odd", "63x65", "64x64", "65x63", "130x70", "65x65", "junk frames 0", "wrap", "threshold edge", "learn 0",
                "learn 1 converges", "learn 15", "learn 16", "freeze changed", "skipped", "3 streams x 4", "targets 65", "targets 130")


class GateCase:
    """one call of the gate: the arena (state, words, gated records and lists), the inputs, and what motionref makes of them"""

    def __init__(self, seed, nstreams, spec, streams, lists, state, first_given=False, own_boxes=False, records=True, out_lists=True, counts=None, what=""):
        rng = np.random.default_rng(seed)
        self.nstreams, self.spec, self.streams, self.what = nstreams, spec, list(streams), what
        n = self.n = len(streams)
        self.stride = motionref.MAX_DET if own_boxes else max(1, max(len(b) for b in lists)) + 3
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
            self.flat = rand_boxes(rng, n * self.stride + 3, spec.w, spec.h, 0.3)  # (slots behind a list hold boxes, too: read only by a clamped count)
            for t, b in enumerate(lists):
                f0 = self.first[t] if first_given else t * self.stride
                self.flat[f0:f0 + len(b)] = b
        ar = Arena()
        nstate = motionref.state_nbytes(nstreams, spec.w, spec.h, spec.cell_log2)
        self.state_off = ar.alloc("state", nstate, 16)
        self.words_off = ar.alloc("words", 4 * n * (motionref.WORDS + 2 * self.stride), 4)
        self.recs_off = ar.alloc("gated records", n * DETS.itemsize, 4) if records else None
        self.lists_off = ar.alloc("gated lists", n * self.stride * BOX.itemsize, 4) if records and out_lists else None
        self._regs = ar.regs
        self.start = ar.fill(rng)
        st = motionref.State(nstreams, spec.w, spec.h, spec.cell_log2, self.start[self.state_off:self.state_off + nstate])
        state(st, rng)
        self.start[self.state_off:self.state_off + nstate] = st.raw.reshape(-1)
        self.state = st
        self.trace = {}
        self.words, self.out_recs, self.out_lists = motionref.gate(self.recs, self.flat, self.stride, self.first, self.streams, spec, st, records,
                                                                   records and out_lists, self.trace)
        self.want = self.start.copy()
        put(self.want, self.words_off, self.words)
        if self.recs_off is not None:
            put(self.want, self.recs_off, self.out_recs)
        if self.lists_off is not None:
            put(self.want, self.lists_off, self.out_lists)

    def regions(self):
        return self._regs


def cells_state(frames, top, force=()):
    """a state setter: random bytes in the plane, header and padding; cells between 0 and `top`, but cell (j, i) of stream s = v for (s, j, i, v) in
    `force`; frames[s]"""
    def fn(st, rng, top=top):
        st.raw[:] = rng.integers(0, 256, st.raw.shape, dtype=np.uint8)
        st.cells[:] = rng.integers(0, top + 1, st.cells.shape)
        for s, j, i, v in force:
            st.cells[s, j, i] = v
        st.hdr[:, 0] = frames
    return fn


def _gate_cases():
    S = motionref.Spec
    rng = np.random.default_rng(8300)
    cases = {}

    def add(name, seed, nstreams, spec, streams, lists, frames=None, top=None, state=None, force=(), **kw):
        top = 2 * spec.min_pixels if top is None else top
        cases[name] = GateCase(seed, nstreams, spec, streams, lists, state or cells_state([spec.warmup + 1 + s for s in range(nstreams)] if frames is None else frames, top, force),
                               what=name, **kw)

    def lists_for(sizes, w, h, extra=None):
        ls = [rand_boxes(rng, s, w, h) for s in sizes]
        for t, b in (extra or {}).items():
            ls[t] = np.concatenate([b, ls[t]]) if len(ls[t]) else b
        return ls

    # 5 x 3 cells of 8: the corners' cases by hand
    hand = np.concatenate([box(9, 3, 4, 8), box(3, 9, 8, 4), box(50, 2, 60, 9), box(-20, -9, -3, -1), box(2, 1, 15, 7), box(2, 1, 16, 7), box(0, 0, 39, 23), box(8, 8, 8, 8)])
    add("corners", 8301, 2, S(40, 24, 3, min_pixels=4, cover=128, warmup=3, min_score=0.25), [0, 1, 0], lists_for([0, 5, 7], 40, 24, {0: hand}))
    add("cover 256", 8302, 1, S(40, 24, 3, min_pixels=4, cover=256, warmup=0), [0, 0], lists_for([9, 6], 40, 24, {0: box(8, 8, 15, 15)}), top=12, force=[(0, 1, 1, 4)])
    add("cover 1", 8303, 1, S(40, 24, 3, min_pixels=4, cover=1, warmup=0), [0, 0], lists_for([9, 6], 40, 24), top=5)
    add("min_pixels 1", 8304, 1, S(40, 24, 3, min_pixels=1, cover=100, warmup=0), [0, 0], lists_for([9, 6], 40, 24), top=1)
    add("min_pixels cc", 8305, 1, S(40, 24, 2, min_pixels=16, cover=100, warmup=0), [0, 0], lists_for([9, 6], 40, 24, {1: box(8, 4, 11, 7)}), top=16, force=[(0, 1, 2, 16)])
    # 130 boxes qualify: 128 are considered, 2 dropped; the gated list is longer than a record
    many = rand_boxes(rng, 133, 40, 24, 0.0)
    many["score"] = 1
    many["score"][[7, 50, 90]] = 0
    add("dropped", 8306, 1, S(40, 24, 3, min_pixels=4, cover=1, warmup=0, min_score=0.5), [0], [many], top=9)
    # NaN scores never qualify; a class list
    nans = rand_boxes(rng, 12, 40, 24, 0.0)
    nans["score"][[1, 4, 9]] = NAN
    add("nan scores classes", 8307, 2, S(40, 24, 3, min_pixels=4, cover=128, warmup=0, min_score=0.25, classes=[1, 0, 1, 1]), [1, 0], [nans, rand_boxes(rng, 10, 40, 24)])
    add("nan min_score", 8308, 1, S(40, 24, 3, min_pixels=4, cover=128, warmup=0, min_score=NAN), [0], lists_for([8], 40, 24))
    add("invert", 8309, 2, S(40, 24, 3, min_pixels=4, cover=128, warmup=2, invert=True), [0, 1, 1], lists_for([8, 9, 3], 40, 24))
    # frames 0, not warm (frames == warmup) and warm: the gate fails open until frames > warmup
    add("warmth", 8310, 3, S(40, 24, 3, min_pixels=4, cover=200, warmup=6), [0, 1, 2, 1], lists_for([6, 6, 8, 5], 40, 24), frames=[0, 6, 7])
    add("warmth inverted", 8311, 3, S(40, 24, 3, min_pixels=4, cover=200, warmup=6, invert=True), [0, 1, 2], lists_for([6, 6, 8], 40, 24), frames=[0, 6, 7])
    add("list_first", 8312, 2, S(33, 17, 2, min_pixels=3, cover=90, warmup=0), [1, 0, -1, 1, 0], lists_for([5, 0, 4, 7, 6], 33, 17), first_given=True)
    add("own boxes", 8313, 2, S(33, 17, 2, min_pixels=3, cover=90, warmup=0), [1, 0, 1], lists_for([5, 9, 2], 33, 17), own_boxes=True, counts={2: 300})
    add("no outputs", 8314, 1, S(40, 24, 3, min_pixels=4, cover=128, warmup=0), [0, 0], lists_for([7, 4], 40, 24), records=False)
    add("records only", 8315, 1, S(40, 24, 3, min_pixels=4, cover=128, warmup=0), [0, 0], lists_for([7, 4], 40, 24), out_lists=False, counts={1: -5})
    add("records 65", 8316, 2, S(24, 16, 3, min_pixels=4, cover=128, warmup=0), [int(v) for v in rng.integers(-1, 2, 65)], lists_for([int(v) for v in rng.integers(0, 5, 65)], 24, 16))
    add("records 130", 8317, 3, S(24, 16, 3, min_pixels=4, cover=128, warmup=1, invert=True), [int(v) for v in rng.integers(-1, 3, 130)],
        lists_for([int(v) for v in rng.integers(0, 4, 130)], 24, 16))
    # a state of random bytes: cells of any value, frames as they fall

    def junk(st, r):
        st.raw[:] = r.integers(0, 256, st.raw.shape, dtype=np.uint8)
        st.cells[::2, ::2, ::2] = r.integers(0, 3, st.cells[::2, ::2, ::2].shape)
    add("junk state", 8318, 2, S(40, 24, 3, min_pixels=2, cover=128, warmup=65535), [0, 1, 0], lists_for([7, 8, 5], 40, 24), state=junk)
    # a row of 512 cells: a box wider than a wave's 64 lanes
    wide = np.concatenate([box(3, 0, 2040, 7), box(700, 2, 1500, 5), box(0, 0, 255, 3)])
    add("wide grid", 8319, 1, S(2048, 8, 2, min_pixels=8, cover=120, warmup=0), [0], lists_for([4], 2048, 8, {0: wide}))
    return cases


@functools.lru_cache(maxsize=None)
def gate_cases():
    return _gate_cases()


GATE_NAMES = ("corners", "cover 256", "cover 1", "min_pixels 1", "min_pixels cc", "dropped", "nan scores classes", "nan min_score", "invert", "warmth", "warmth inverted",
              "list_first", "own boxes", "no outputs", "records only", "records 65", "records 130", "junk state", "wide grid")
