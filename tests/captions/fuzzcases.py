"""The seeded cases of the captions fuzz (tests/captions/test_gpu_fuzz_input.py) and the conditions that keep it from passing vacuously.  The cases are
made here, on the CPU and before any device call: the items, the targets in one arena of seeded random bytes (64 guard bytes around each surface) and
what textref makes of them -- so tests/test_captions_abi.py can hold the conditions against textref alone.

Rasteriser cases (TextCase), for BGR and NV12 alike: heavy overlap under a random font; the built-in font with 64 and 256 items per target; 70 small
targets (two launches) with a skipped target and one whose items are all empty; hostile items (random bytes, len above 44, scale above 4, corners of
the int range).  Composer cases (BoxCase, SceneCase): lists of 0, 1, 127, 128, 129, 255, 256, 257 boxes, the records' own boxes with claimed counts
out of range, list_first given, 131 records (two launches), boxes with NaN / Inf / huge corners, scores and types; scenes from the zones fuzz with
counts and nverts out of range, random state and events, 520 targets (two launches)."""
import numpy as np

from captions import textref
from zones import fuzzcases as zonecases

BOX, DETS, ITEM, SCENE = textref.BOX_DTYPE, textref.DETS_DTYPE, textref.ITEM_DTYPE, textref.SCENE_DTYPE
GUARD = 64
F32 = np.float32
NAN, INF = float("nan"), float("inf")
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------------- the rasteriser
def rand_item(rng, w, h, ascii_only=False, long_text=False):
    """an item whose rectangle meets the target (or nearly): every scale, both paper settings, junk in the ignored flag bits and behind len"""
    it = np.frombuffer(rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), ITEM).copy()[0]
    s = int(rng.integers(1, 5))
    n = int(rng.integers(1, 45 if long_text else 7))
    it["scale"], it["len"] = s, n
    it["flags"] = int(rng.integers(0, 2)) | (int(rng.integers(0, 128)) << 1)
    it["x"], it["y"] = int(rng.integers(-8 * s * n + 1, w)), int(rng.integers(-8 * s + 1, h))
    if ascii_only:
        it["text"] = rng.integers(32, 127, 44)
    return it


class TextCase:
    """items_stride items for each of the targets; targets[t] is None (skipped) or a dict: BGR (off, w, h, pitch), NV12 (y_off, uv_off, w, h, pitch_y,
    pitch_uv), offsets into the arena `start`"""

    def __init__(self, what, nv12, seed, sizes, stride, make_items, font="random", skipped=()):
        rng = np.random.default_rng(seed)
        self.what, self.nv12, self.stride, self.n = what, nv12, stride, len(sizes)
        self.font = rng.integers(0, 256, (256, 8), dtype=np.uint8) if font == "random" else None
        self.targets, size = [], GUARD
        for t, (w, h) in enumerate(sizes):
            if t in skipped:
                self.targets.append(None)
                continue
            if nv12:
                pitch_y, pitch_uv = w + int(rng.integers(0, 5)), 2 * ((w + 1) // 2) + 2 * int(rng.integers(0, 3))
                y_off = size + int(rng.integers(0, 3))                              # (any byte alignment)
                uv_off = (y_off + pitch_y * h + GUARD + 1) & ~1                    # (2-byte aligned: the arena's base is)
                self.targets.append(dict(y_off=y_off, uv_off=uv_off, w=w, h=h, pitch_y=pitch_y, pitch_uv=pitch_uv))
                size = uv_off + pitch_uv * ((h + 1) // 2) + GUARD
            else:
                pitch = 3 * w + int(rng.integers(0, 6))
                off = size + int(rng.integers(0, 4))
                self.targets.append(dict(off=off, w=w, h=h, pitch=pitch))
                size = off + pitch * h + GUARD
        self.start = rng.integers(0, 256, size, dtype=np.uint8)
        self.items = np.zeros((self.n, stride), ITEM)
        for t, (w, h) in enumerate(sizes):
            self.items[t] = make_items(rng, t, w, h, stride)
        self._want = None

    def font_or(self, builtin):
        return np.asarray(builtin, np.uint8).reshape(256, 8) if self.font is None else self.font

    def want(self, builtin):
        """the arena after the call, by textref (computed once)"""
        if self._want is None:
            out = self.start.copy()
            for t, tg in enumerate(self.targets):
                if tg is None:
                    continue
                if self.nv12:
                    textref.draw_nv12(out, tg["y_off"], tg["uv_off"], tg["w"], tg["h"], tg["pitch_y"], tg["pitch_uv"], self.items[t], self.font_or(builtin))
                else:
                    textref.draw_bgr(out, tg["off"], tg["w"], tg["h"], tg["pitch"], self.items[t], self.font_or(builtin))
            self._want = out
        return self._want

    def descs(self, base):
        """the targets as ffcnn_amd.capi takes them, the arena at device address `base`"""
        if self.nv12:
            return [None if g is None else (base + g["y_off"], base + g["uv_off"], g["w"], g["h"], g["pitch_y"], g["pitch_uv"]) for g in self.targets]
        return [None if g is None else (base + g["off"], g["w"], g["h"], g["pitch"]) for g in self.targets]

    def stats(self, builtin):
        """per target, by textref's masks alone: two items write a common pixel with different values; an item is clipped by an edge; (NV12) a chroma
        sample's luma pixels are written by two different items; a sample whose deciding item writes only paper there; and the raw settings seen"""
        font = self.font_or(builtin)
        st = dict(targets=0, overlap=0, clipped=0, shared_sample=0, paper_sample=0, scales=set(), opaque=set(), empty_unchanged=0, len_over=0, scale_over=0)
        want = self.want(builtin)
        for t, tg in enumerate(self.targets):
            if tg is None:
                continue
            st["targets"] += 1
            w, h = tg["w"], tg["h"]
            value = np.full((h, w), -1, np.int64)
            owner = np.full(((h + 1) // 2, (w + 1) // 2), -1, np.int64)
            paper = np.zeros(owner.shape, bool)
            overlap = clipped = shared = False
            for k, it in enumerate(self.items[t]):
                st["len_over"] += int(it["len"]) > 44
                st["scale_over"] += int(it["scale"]) > 4
                m = textref.masks(it, font, w, h)
                if m is None:
                    continue
                s, n = textref.clamped(it)
                st["scales"].add(s)
                st["opaque"].add(int(it["flags"]) & 1)
                x0, y0, written, ink = m
                clipped |= written.shape != (8 * s, 8 * s * n)
                col = [int(it[c][0]) | int(it[c][1]) << 8 | int(it[c][2]) << 16 for c in ("bg", "fg")]
                new = np.where(ink, col[1], col[0])
                old = value[y0:y0 + written.shape[0], x0:x0 + written.shape[1]]
                overlap |= bool((written & (old >= 0) & (old != new)).any())
                old[written] = new[written]
                ys, xs = np.nonzero(written)
                sy, sx = (y0 + ys) >> 1, (x0 + xs) >> 1
                shared |= bool(((owner[sy, sx] >= 0) & (owner[sy, sx] != k)).any())
                owner[sy, sx] = k
                paper[sy, sx] = True
                paper[sy[ink[ys, xs]], sx[ink[ys, xs]]] = False
            st["overlap"] += overlap
            st["clipped"] += clipped
            st["shared_sample"] += shared
            st["paper_sample"] += int((paper & (owner >= 0)).sum())
            if not self.items[t]["len"].any():
                lo, hi = (tg["y_off"], tg["uv_off"] + tg["pitch_uv"] * ((h + 1) // 2)) if self.nv12 else (tg["off"], tg["off"] + tg["pitch"] * h)
                st["empty_unchanged"] += want[lo:hi].tobytes() == self.start[lo:hi].tobytes()
        return st


def _overlap_items(rng, t, w, h, stride):
    return np.array([rand_item(rng, w, h) for _ in range(stride)], ITEM)


def _builtin_items(rng, t, w, h, stride):
    out = np.array([rand_item(rng, w, h, ascii_only=True, long_text=k % 5 == 0) for k in range(stride)], ITEM)
    out["len"][rng.random(stride) < 0.3] = 0                                        # unused slots among the used ones
    return out


def _many_items(rng, t, w, h, stride):
    out = np.array([rand_item(rng, w, h) for _ in range(stride)], ITEM)
    if t % 9 == 4:
        out["len"] = 0                                                              # a target whose items are all empty
    return out


def _hostile_items(rng, t, w, h, stride):
    """random bytes; every other item moved to where it can be seen; the corners of the int range"""
    out = np.frombuffer(rng.integers(0, 256, 64 * stride, dtype=np.uint8).tobytes(), ITEM).copy()
    for k in range(0, stride, 2):
        out[k]["x"], out[k]["y"] = int(rng.integers(-40, w)), int(rng.integers(-20, h))
    corners = [(IMIN, IMIN), (IMAX, IMAX), (IMIN, 0), (0, IMIN), (IMAX, 0), (0, IMAX), (IMAX - 3, 2), (2, IMAX - 3), (IMIN + 5, 1)]
    for k, (x, y) in enumerate(corners[:stride // 2]):
        out[2 * k + 1]["x"], out[2 * k + 1]["y"] = x, y
    out[0]["len"], out[0]["scale"] = 200, 9                                          # reads as 44 characters at scale 4
    return out


SIZES = [(37, 21), (64, 32), (101, 47), (33, 90), (200, 17), (1, 1), (2, 3), (129, 65)]
TEXT_NAMES = ("overlap", "builtin 64", "builtin 256", "targets 70", "hostile")
_TEXT = {}


def text_cases(nv12):
    """the rasteriser's cases for one surface format, by name"""
    if nv12 not in _TEXT:
        seed = 5700 + 50 * int(nv12)
        odd = [(w | 1, h | 1) if k % 2 == 0 else (w, h) for k, (w, h) in enumerate(SIZES)]
        small = [(24 + t % 7, 17 + t % 5) for t in range(70)]
        _TEXT[nv12] = {
            "overlap": TextCase("overlap", nv12, seed, odd, 7, _overlap_items),
            "builtin 64": TextCase("builtin 64", nv12, seed + 1, odd[:4], 64, _builtin_items, font=None),
            "builtin 256": TextCase("builtin 256", nv12, seed + 2, [(160, 64), (75, 33)], 256, _builtin_items, font=None),
            "targets 70": TextCase("targets 70", nv12, seed + 3, small, 3, _many_items, skipped=(0, 63, 64)),
            "hostile": TextCase("hostile", nv12, seed + 4, odd[:6], 20, _hostile_items),
        }
    return _TEXT[nv12]


def check_text_stats(builtin):
    """the conditions of the issue over the case set, per format; returns the totals"""
    out = {}
    for nv12 in (False, True):
        tot = None
        for c in text_cases(nv12).values():
            st = c.stats(builtin)
            if tot is None:
                tot = st
            else:
                for k, v in st.items():
                    tot[k] = tot[k] | v if isinstance(v, set) else tot[k] + v
        n = tot["targets"]
        assert 4 * tot["overlap"] >= n and 4 * tot["clipped"] >= n, (nv12, tot)
        assert tot["scales"] == {1, 2, 3, 4} and tot["opaque"] == {0, 1}, (nv12, tot)
        assert tot["empty_unchanged"] >= 1 and tot["len_over"] >= 1 and tot["scale_over"] >= 1, (nv12, tot)
        if nv12:
            assert 4 * tot["shared_sample"] >= n and tot["paper_sample"] >= 1, tot
        out[nv12] = tot
    return out


# ---------------------------------------------------------------------------------------------------------------- the box composer
NAMES80 = [b"", b"p", b"person", b"fifteen-bytes-xx", b"sixteen bytes, ok", b"traffic light"] + [b"class %d" % k for k in range(6, 80)]


def names_rows(names=NAMES80):
    out = np.zeros((len(names), 16), np.uint8)
    for k, nm in enumerate(names):
        out[k, :min(16, len(nm))] = np.frombuffer(nm[:16], np.uint8)
    return out


def rand_boxes(rng, n, weird=0.1):
    """boxes over a 200 x 120 picture: classes in and out of the names, scores on both sides of every bound, now and then a corner or a score that is
    NaN, infinite or beyond int"""
    b = np.zeros(n, BOX)
    b["type"] = rng.choice([0, 1, 2, 3, 4, 5, 79, 80, -1, 130, IMAX, IMIN, 7, 8], n)
    b["score"] = rng.choice([0.0, 0.004999, 0.005, 0.25, 0.5, 0.93, 0.995, 1.0, 9.99, 0.1249, 0.125], n).astype(F32)
    b["x1"], b["y1"] = rng.uniform(-20, 200, n), rng.uniform(-20, 120, n)
    b["x2"], b["y2"] = b["x1"] + rng.uniform(2, 60, n), b["y1"] + rng.uniform(2, 60, n)
    for k in np.nonzero(rng.random(n) < weird)[0]:
        b[k][str(rng.choice(["score", "x1", "y1"]))] = rng.choice([NAN, INF, -INF, 1e9, -3e9, 2147483648.0, -2147483648.0, 1e30])
    return b


class BoxCase:
    """one ffgpu_caption_boxes_dev call: records, lists (or the records' own boxes), ids, spec; the items lie in an arena of seeded random bytes"""

    def __init__(self, what, seed, counts, stride, items_stride, spec, use_records=False, first_given=False, claimed=None):
        rng = np.random.default_rng(seed)
        self.what, self.n, self.items_stride, self.spec = what, len(counts), items_stride, spec
        self.recs = np.frombuffer(rng.integers(0, 256, DETS.itemsize * self.n, dtype=np.uint8).tobytes(), DETS).copy()
        self.stride = stride if not use_records else 0
        S = textref.MAX_DET if use_records else stride
        self.flat, self.first = None, None
        if use_records:
            for t, c in enumerate(counts):
                self.recs[t]["box"] = rand_boxes(rng, textref.MAX_DET)
                self.recs[t]["count"] = c if claimed is None else claimed[t]
        else:
            order = rng.permutation(self.n) if first_given else np.arange(self.n)
            self.flat = rand_boxes(rng, self.n * stride + 3)
            self.first = [int(order[t]) * stride + (3 if first_given else 0) for t in range(self.n)] if first_given else None
            for t, c in enumerate(counts):
                self.recs[t]["nfull"] = c if claimed is None else claimed[t]
        self.ids = None
        if spec.identity == textref.IDS:
            self.ids = rng.choice([0, 1, 2, 12, -1, -7, IMAX, IMIN, 1000000], (self.n, 8 + S)).astype("<i4")
        self.items_off = GUARD
        self.start = rng.integers(0, 256, GUARD + 64 * self.n * items_stride + GUARD, dtype=np.uint8)
        self.want_items = textref.caption_boxes(self.recs, self.flat, stride, self.first, spec, self.ids, items_stride)
        self.want = self.start.copy()
        self.want[GUARD:GUARD + self.want_items.nbytes] = self.want_items.view(np.uint8).reshape(-1)


BOX_NAMES = ("lists", "own boxes", "first given", "records 131", "clamped lists")
_BOXES = {}


def box_cases():
    if not _BOXES:
        S, names = textref.Spec, names_rows()
        allp = textref.NAME | textref.SCORE | textref.ID
        pal = [(10, 20, 30), (40, 50, 60), (70, 80, 90), (1, 2, 3), (4, 5, 6), (250, 251, 252), (9, 9, 9)]
        _BOXES.update({
            "lists": BoxCase("lists", 5800, [0, 1, 127, 128, 129, 255, 256, 257, 6], 257, 256,
                             S(allp | textref.CAPTION_OPAQUE, 0.125, textref.IDS, 2, (255, 254, 253), palette=pal, names=names)),
            "own boxes": BoxCase("own boxes", 5801, [0, 3, 128, 128, 128, 5], 0, 5, S(allp, 0.0, textref.TYPE, 1, color=(7, 8, 9)), use_records=True,
                                 claimed=[0, 3, 128, 129, -4, IMAX]),
            "first given": BoxCase("first given", 5802, [4, 0, 9, 2, 7], 9, 1, S(textref.NAME | textref.SCORE, 0.005, textref.NONE, 4, names=names), first_given=True),
            "records 131": BoxCase("records 131", 5803, [t % 5 for t in range(131)], 4, 3,
                                   S(allp | textref.CAPTION_OPAQUE, 0.25, textref.IDS, 3, palette=pal[:1], names=names[:3])),
            "clamped lists": BoxCase("clamped lists", 5804, [6, 6, 6, 6], 6, 16, S(textref.SCORE | textref.ID, 1.0, textref.TYPE, 1), claimed=[7, -1, IMAX, IMIN]),
        })
    return _BOXES


def check_box_stats():
    """what the cases show, over the set: a target that captions min(128, items_stride) boxes and leaves qualifying ones out, one that captions none, every
    part, a name from the table and a class in decimal, a pending id, a tag above its box and one inside it, scores at both clamps"""
    seen = dict.fromkeys(("full", "none", "name", "decimal", "pending", "above", "inside", "percent_999", "percent_0"), 0)
    for c in box_cases().values():
        for t in range(c.n):
            used = int((c.want_items[t]["len"] > 0).sum())
            seen["full"] += used == min(128, c.items_stride)
            seen["none"] += used == 0
            for it in c.want_items[t][:used]:
                txt = bytes(it["text"][:int(it["len"])])
                seen["name"] += txt.startswith((b"person", b"class "))
                seen["decimal"] += txt.startswith((b"-1 ", b"130 ", b"2147483647 ", b"-2147483648 "))
                seen["pending"] += txt.endswith(b"?")
                seen["percent_999"] += b"999%" in txt
                seen["percent_0"] += txt.startswith(b"0%") or b" 0%" in txt
        boxes_y = c.want_items["y"][c.want_items["len"] > 0]
        seen["above"] += int((boxes_y > 8).sum())
        seen["inside"] += int((boxes_y <= 0).sum())
    assert all(v > 0 for v in seen.values()), seen
    return seen


# ---------------------------------------------------------------------------------------------------------------- the scene composer
class SceneCase:
    def __init__(self, what, seed, nstreams, capacity, ntargets, S, items_stride, spec):
        rng = np.random.default_rng(seed)
        self.what, self.nstreams, self.capacity, self.n, self.items_stride, self.spec = what, nstreams, capacity, ntargets, items_stride, spec
        self.scenes = np.array([zonecases.rand_scene(rng, s) for s in range(nstreams)], SCENE)
        self.scenes["zone"]["x"][0, 0, 0], self.scenes["zone"]["y"][0, 1, 0] = 3e9, NAN
        self.state = rng.integers(0, 256, nstreams * (144 + 64 * capacity), dtype=np.uint8)
        hdr = self.state.reshape(nstreams, -1)[:, :144].view("<u4")
        hdr[:, 20:36] = rng.choice([0, 1, 9, 10, 4294967295, 1000000000, 123456789, 99], (nstreams, 16))
        self.events_stride = 64 + 2 * S
        self.events = rng.choice([0, 1, 7, 128, 4294967295, 2147483648, 10, 100], (ntargets, self.events_stride)).astype("<u4")
        self.streams = [int(v) for v in rng.integers(-1, nstreams, ntargets)]
        self.streams[:3] = [0, -1, nstreams - 1]
        self.items_off = GUARD
        self.start = rng.integers(0, 256, GUARD + 64 * ntargets * items_stride + GUARD, dtype=np.uint8)
        self.want_items = textref.caption_scene(self.scenes, self.state, nstreams, capacity, self.events, self.events_stride, self.streams, spec, items_stride)
        self.want = self.start.copy()
        self.want[GUARD:GUARD + self.want_items.nbytes] = self.want_items.view(np.uint8).reshape(-1)


SCENE_NAMES = ("six streams", "targets 520", "stride 256")
_SCENES = {}


def scene_cases():
    if not _SCENES:
        S = textref.Spec
        pal = [(k, 2 * k, 255 - k) for k in range(5)]
        _SCENES.update({
            "six streams": SceneCase("six streams", 5900, 6, 3, 12, 9, 16, S(textref.CAPTION_OPAQUE, scale=2, fg=(1, 2, 3), palette=pal)),
            "targets 520": SceneCase("targets 520", 5901, 7, 1, 520, 1, 17, S(0, scale=1, color=(200, 100, 50))),
            "stride 256": SceneCase("stride 256", 5902, 2, 128, 3, 40, 256, S(textref.CAPTION_OPAQUE | textref.NAME, scale=4, palette=pal[:3])),
        })
    return _SCENES
