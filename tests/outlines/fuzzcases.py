"""The seeded cases of the outlines fuzz (tests/outlines/test_gpu_fuzz_input.py) and the conditions that keep it from passing vacuously.  The cases are
made here, on the CPU and before any device call: the items and the targets in one arena of seeded random bytes (64 guard bytes around each surface
and around the items) and what lineref makes of them -- so tests/test_outlines_abi.py can hold the conditions against lineref alone.

Primitive cases (SegCase), for BGR and NV12 alike, surfaces of 64 x 48 at most: heavy overlap of 64 random items; 512 items per target; 70 small
targets (two launches) with skipped targets and targets whose items are all empty; the named cases of tests/test_outlines_abi.py, the long 64-bit
segment included; hostile items (random bytes, thickness and dash above their clamps, the corners of the int range).  Composer cases (SceneCase):
scenes from the zones fuzz with counts and nverts out of range, NaN, Inf and far-off vertices, random events, a random state with seen slots planted
in it, streams with -1 entries, 520 targets (two launches), items_stride 80, 81 and 512."""
import numpy as np

from outlines import lineref
from zones import fuzzcases as zonecases

ITEM, SCENE = lineref.ITEM_DTYPE, lineref.SCENE_DTYPE
GUARD = 64
NAN, INF = float("nan"), float("inf")
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1
LIMIT = lineref.SEG_LIMIT


# ---------------------------------------------------------------------------------------------------------------- the primitive
def seg(x0, y0, x1, y1, color=(200, 100, 50), thickness=1, dash=0):
    return lineref.make_item(x0, y0, x1, y1, color, thickness, dash)


def rand_item(rng, w, h, reach=8):
    """an item whose end points lie in or near the target: every thickness and dash, junk in the ignored bytes"""
    it = np.frombuffer(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), ITEM).copy()[0]
    it["x0"], it["x1"] = rng.integers(-reach, w + reach, 2)
    it["y0"], it["y1"] = rng.integers(-reach, h + reach, 2)
    it["thickness"], it["dash"] = int(rng.integers(1, 9)), int(rng.integers(0, 7)) if rng.random() < 0.4 else 0
    return it


def named_items():
    """the named cases: [(name, item)], to be drawn into a 37 x 23 target (and any other)"""
    out = []
    for k, (dx, dy) in enumerate(((9, 4), (4, 9), (-4, 9), (-9, 4), (-9, -4), (-4, -9), (4, -9), (9, -4))):
        out.append(("octant %d" % k, seg(18, 11, 18 + dx, 11 + dy, (10 + k, 20, 30))))
        out.append(("octant %d back" % k, seg(20 + dx, 12 + dy, 20, 12, (40, 50 + k, 60))))
    out.append(("point", seg(5, 6, 5, 6, (1, 2, 3), 5)))
    out.append(("diagonal", seg(2, 3, 14, 15, (4, 5, 6), 2)))
    out.append(("antidiagonal", seg(30, 2, 22, 10, (7, 8, 9), 3)))
    out.append(("tie", seg(0, 0, 4, 2, (11, 12, 13))))
    for T in range(1, 10):
        out.append(("thickness %d" % T, seg(1 + 4 * T, 1, 3 + 4 * T, 21, (100 + T, 2 * T, 3 * T), T)))
    out.append(("dash 7", seg(-3, 20, 40, 18, (90, 91, 92), 1, 7)))
    out.append(("dash 1", seg(0, 16, 36, 17, (93, 94, 95), 2, 1)))
    out.append(("at the limit x", seg(-LIMIT, 5, LIMIT, 5, (21, 22, 23))))
    out.append(("at the limit y", seg(3, LIMIT, 3, -LIMIT, (24, 25, 26), 2)))
    for k, (a, b) in enumerate((((-LIMIT - 1, 5), (10, 5)), ((10, 5), (LIMIT + 1, 5)), ((3, -LIMIT - 1), (3, 9)), ((3, 9), (3, LIMIT + 1)),
                                ((IMIN, IMIN), (IMAX, IMAX)), ((0, 0), (IMAX, 0)), ((IMIN, 7), (IMAX, 7)), ((4, IMAX), (4, IMIN)))):
        out.append(("beyond the limit %d" % k, seg(*a, *b, (250, 251, 252), 8)))
    out.append(("long", seg(-LIMIT, -LIMIT + 3, LIMIT, LIMIT, (31, 32, 33), 2)))
    out.append(("thickness 0", seg(0, 0, 36, 22, (34, 35, 36), 0)))
    return out


class SegCase:
    """items_stride items for each of the targets; targets[t] is None (skipped) or a dict: BGR (off, w, h, pitch), NV12 (y_off, uv_off, w, h, pitch_y,
    pitch_uv), offsets into the arena `start`; the items lie in the arena too, at items_off"""

    def __init__(self, what, nv12, seed, sizes, stride, make_items, skipped=()):
        rng = np.random.default_rng(seed)
        self.what, self.nv12, self.stride, self.n = what, nv12, stride, len(sizes)
        self.targets, size = [], GUARD
        for t, (w, h) in enumerate(sizes):
            assert w <= 64 and h <= 48
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
                pitch = 3 * w + 1 + 2 * int(rng.integers(0, 3))                     # row padding, and the rows at odd and even addresses in turn
                off = (size | 1) + 2 * int(rng.integers(0, 2))                     # an odd address
                self.targets.append(dict(off=off, w=w, h=h, pitch=pitch))
                size = off + pitch * h + GUARD
        self.items_off = (size + 3) & ~3
        size = self.items_off + 32 * self.n * stride + GUARD
        self.start = rng.integers(0, 256, size, dtype=np.uint8)
        self.items = np.zeros((self.n, stride), ITEM)
        for t, (w, h) in enumerate(sizes):
            self.items[t] = make_items(rng, t, w, h, stride)
        self.start[self.items_off:self.items_off + self.items.nbytes] = self.items.view(np.uint8).reshape(-1)
        self._want = None

    def want(self):
        """the arena after the call, by lineref (computed once)"""
        if self._want is None:
            out = self.start.copy()
            for t, tg in enumerate(self.targets):
                if tg is None:
                    continue
                if self.nv12:
                    lineref.draw_nv12(out, tg["y_off"], tg["uv_off"], tg["w"], tg["h"], tg["pitch_y"], tg["pitch_uv"], self.items[t])
                else:
                    lineref.draw_bgr(out, tg["off"], tg["w"], tg["h"], tg["pitch"], self.items[t])
            self._want = out
        return self._want

    def descs(self, base):
        """the targets as ffcnn_amd.capi takes them, the arena at device address `base`"""
        if self.nv12:
            return [None if g is None else (base + g["y_off"], base + g["uv_off"], g["w"], g["h"], g["pitch_y"], g["pitch_uv"]) for g in self.targets]
        return [None if g is None else (base + g["off"], g["w"], g["h"], g["pitch"]) for g in self.targets]

    def stats(self):
        """per target, by lineref's pixel sets alone: two items write a common pixel with different colours; an item is cut by an edge; (NV12) two
        items write luma pixels of one chroma sample; and, over the items that draw, the octants, thicknesses and dashes, the rounding ties, the items
        wholly outside"""
        st = dict(targets=0, overlap=0, clipped=0, shared_sample=0, octants=set(), thickness=set(), dash=set(), ties=0, used=0, outside=0, empty_unchanged=0,
                  thickness_over=0, dash_over=0)
        want = self.want()
        for t, tg in enumerate(self.targets):
            if tg is None:
                continue
            st["targets"] += 1
            w, h = tg["w"], tg["h"]
            value = np.full((h, w), -1, np.int64)
            owner = np.full(((h + 1) // 2, (w + 1) // 2), -1, np.int64)
            overlap = clipped = shared = False
            for k, it in enumerate(self.items[t]):
                st["thickness_over"] += int(it["thickness"]) > 8
                st["dash_over"] += int(it["dash"]) > 6
                c = lineref.canon(it)
                if c is None:
                    continue
                ym, sm, sn, D, g, T, d = c
                st["used"] += 1
                xs, ys = lineref.pixels(it, w, h)
                if not len(xs):
                    st["outside"] += 1
                    continue
                m = np.arange(0, D + 1, dtype=np.int64)
                clipped |= len(xs) < T * int((((m >> d) & 1) == 0).sum() if d else D + 1)
                st["thickness"].add(T)
                st["dash"].add(d)
                dx, dy = int(it["x1"]) - int(it["x0"]), int(it["y1"]) - int(it["y0"])
                if dx and dy and abs(dx) != abs(dy):
                    st["octants"].add((dx > 0, dy > 0, abs(dx) > abs(dy)))
                ms = (ys if ym else xs) - sm
                st["ties"] += int(g != 0 and D > 0 and bool(((2 * ms * g + D) % (2 * D) == 0).any()))
                col = int(it["color"][0]) | int(it["color"][1]) << 8 | int(it["color"][2]) << 16
                old = value[ys, xs]
                overlap |= bool(((old >= 0) & (old != col)).any())
                value[ys, xs] = col
                shared |= bool(((owner[ys >> 1, xs >> 1] >= 0) & (owner[ys >> 1, xs >> 1] != k)).any())
                owner[ys >> 1, xs >> 1] = k
            st["overlap"] += overlap
            st["clipped"] += clipped
            st["shared_sample"] += shared
            if not self.items[t]["thickness"].any():
                lo, hi = (tg["y_off"], tg["uv_off"] + tg["pitch_uv"] * ((h + 1) // 2)) if self.nv12 else (tg["off"], tg["off"] + tg["pitch"] * h)
                st["empty_unchanged"] += want[lo:hi].tobytes() == self.start[lo:hi].tobytes()
        return st


def _overlap_items(rng, t, w, h, stride):
    return np.array([rand_item(rng, w, h) for _ in range(stride)], ITEM)


def _many_items(rng, t, w, h, stride):
    out = np.array([rand_item(rng, w, h, reach=3) for _ in range(stride)], ITEM)
    out["thickness"][rng.random(stride) < 0.3] = 0                                  # unused slots among the used ones
    if t % 9 == 4:
        out["thickness"] = 0                                                        # a target whose items are all empty
    return out


def _named(rng, t, w, h, stride):
    out = np.zeros(stride, ITEM)
    named = named_items()
    out[:len(named)] = [it for _, it in named]
    return out


def _hostile_items(rng, t, w, h, stride):
    """random bytes; every other item moved to where it can be seen; the corners of the int range"""
    out = np.frombuffer(rng.integers(0, 256, 32 * stride, dtype=np.uint8).tobytes(), ITEM).copy()
    for k in range(0, stride, 2):
        out[k]["x0"], out[k]["x1"] = rng.integers(-40, w + 40, 2)
        out[k]["y0"], out[k]["y1"] = rng.integers(-20, h + 20, 2)
    corners = [(IMIN, IMIN, IMAX, IMAX), (IMAX, IMAX, IMIN, IMIN), (IMIN, 0, IMAX, 0), (0, IMIN, 0, IMAX), (IMAX, 0, 0, 0), (0, 0, 0, IMAX), (IMAX - 3, 2, 2, IMAX - 3),
               (IMIN + 5, 1, 1, 1), (-LIMIT, -LIMIT, LIMIT, LIMIT), (LIMIT, -LIMIT, -LIMIT, LIMIT)]
    for k, c in enumerate(corners[:stride // 2]):
        out[2 * k + 1]["x0"], out[2 * k + 1]["y0"], out[2 * k + 1]["x1"], out[2 * k + 1]["y1"] = c
    out[0]["thickness"], out[0]["dash"] = 200, 99                                    # reads as thickness 8, dash 6
    return out


SIZES = [(37, 21), (64, 32), (51, 47), (33, 48), (64, 17), (1, 1), (2, 3), (29, 45)]
SEG_NAMES = ("overlap", "items 512", "targets 70", "named", "hostile")
NAMED_SIZE = (37, 23)
_SEG = {}


def seg_cases(nv12):
    """the primitive's cases for one surface format, by name"""
    if nv12 not in _SEG:
        seed = 6100 + 50 * int(nv12)
        odd = [(min(w | 1, 63), min(h | 1, 47)) if k % 2 == 0 else (w, h) for k, (w, h) in enumerate(SIZES)]
        small = [(12 + t % 7, 9 + t % 5) for t in range(70)]
        _SEG[nv12] = {
            "overlap": SegCase("overlap", nv12, seed, odd, 64, _overlap_items),
            "items 512": SegCase("items 512", nv12, seed + 1, [(64, 48), (33, 27)], 512, _many_items),
            "targets 70": SegCase("targets 70", nv12, seed + 2, small, 3, _many_items, skipped=(0, 63, 64)),
            "named": SegCase("named", nv12, seed + 3, [NAMED_SIZE, (64, 48)], len(named_items()) + 1, _named),
            "hostile": SegCase("hostile", nv12, seed + 4, odd[:6], 24, _hostile_items),
        }
    return _SEG[nv12]


def check_seg_stats():
    """the conditions of the issue over the case set, per format; returns the totals"""
    out = {}
    for nv12 in (False, True):
        tot = None
        for name, c in seg_cases(nv12).items():
            st = c.stats()
            if name != "hostile":
                assert 2 * st["outside"] <= st["used"], (nv12, name, st)
            if name in ("overlap", "items 512"):                                    # the two cases of many items hold the quarters on their own
                assert 4 * st["overlap"] >= st["targets"] and 4 * st["clipped"] >= st["targets"], (nv12, name, st)
                assert not nv12 or 4 * st["shared_sample"] >= st["targets"], (name, st)
            if tot is None:
                tot = st
            else:
                for k, v in st.items():
                    tot[k] = tot[k] | v if isinstance(v, set) else tot[k] + v
        n = tot["targets"]
        assert 4 * tot["overlap"] >= n and 4 * tot["clipped"] >= n, (nv12, tot)
        assert len(tot["octants"]) == 8 and tot["thickness"] == set(range(1, 9)) and tot["dash"] == set(range(7)), (nv12, tot)
        assert tot["ties"] >= 1 and tot["empty_unchanged"] >= 1 and tot["thickness_over"] >= 1 and tot["dash_over"] >= 1, (nv12, tot)
        if nv12:
            assert 4 * tot["shared_sample"] >= n, tot
        out[nv12] = tot
    return out


# ---------------------------------------------------------------------------------------------------------------- the scene composer
class SceneCase:
    def __init__(self, what, seed, nstreams, capacity, ntargets, S, items_stride, spec):
        rng = np.random.default_rng(seed)
        self.what, self.nstreams, self.capacity, self.n, self.items_stride, self.spec = what, nstreams, capacity, ntargets, items_stride, spec
        self.scenes = np.array([zonecases.rand_scene(rng, s) for s in range(nstreams)], SCENE)
        self.scenes["zone"]["x"][0, 0, 0], self.scenes["zone"]["y"][0, 1, 0], self.scenes["zone"]["x"][0, 2, 1] = 3e9, NAN, -INF
        self.scenes["line"]["bx"][0, 0], self.scenes["line"]["ay"][0, 1] = INF, -3e9
        self.state = rng.integers(0, 256, nstreams * (144 + 64 * capacity), dtype=np.uint8)
        raw = self.state.reshape(nstreams, -1)
        for s in range(nstreams):
            frames = (0, 1, 2 ** 32 - 1, 7, int(rng.integers(0, 2 ** 32)))[s % 5]
            raw[s, :4] = np.frombuffer(np.uint32(frames).tobytes(), np.uint8)
            slots = np.ascontiguousarray(raw[s, 144:]).view(lineref.SLOT_DTYPE)
            for q in range(capacity):
                r = rng.random()
                if r < 0.5:                                                          # seen in the last frame
                    slots[q]["id"] = rng.choice([1, 2, 17, -3, IMAX, IMIN, 300])
                    slots[q]["last"] = np.uint32((frames - 1) % 2 ** 32).astype(np.int32)
                    slots[q]["px"], slots[q]["py"] = rng.uniform(-5, 52, 2)
                    if rng.random() < 0.1:
                        slots[q]["px"] = rng.choice([NAN, INF, -INF, 3e9, -3e9, 2147483520.0])
                elif r < 0.7:                                                        # free, or seen a frame earlier
                    slots[q]["id"] = 0 if r < 0.6 else 5
                    slots[q]["last"] = np.uint32((frames - 2) % 2 ** 32).astype(np.int32) if r >= 0.6 else slots[q]["last"]
            raw[s, 144:] = slots.view(np.uint8)
        self.events_stride = 64 + 2 * S
        self.events = rng.choice([0, 0, 1, 7, 4294967295, 2147483648], (ntargets, self.events_stride)).astype("<u4")
        self.streams = [int(v) for v in rng.integers(-1, nstreams, ntargets)]
        self.streams[:3] = [0, -1, nstreams - 1]
        self.items_off = GUARD
        self.start = rng.integers(0, 256, GUARD + 32 * ntargets * items_stride + GUARD, dtype=np.uint8)
        self.want_items = lineref.outline_scene(self.scenes, self.state, nstreams, capacity, self.events, self.events_stride, self.streams, spec, items_stride)
        self.want = self.start.copy()
        self.want[GUARD:GUARD + self.want_items.nbytes] = self.want_items.view(np.uint8).reshape(-1)


SCENE_NAMES = ("six streams", "targets 520", "stride 512")
_SCENES = {}
ALL = lineref.ZONES | lineref.LINES | lineref.TICKS | lineref.MARKERS | lineref.ALARM


def scene_cases():
    if not _SCENES:
        S = lineref.Spec
        pal = [(k + 1, 2 * k + 1, 255 - k) for k in range(5)]
        _SCENES.update({
            "six streams": SceneCase("six streams", 6200, 6, 3, 12, 9, 80, S(ALL, 3, 2, 4, alarm=(9, 8, 255), palette=pal)),
            "targets 520": SceneCase("targets 520", 6201, 7, 5, 520, 1, 81, S(lineref.ZONES | lineref.MARKERS, 1, 0, 1, color=(200, 100, 50))),
            "stride 512": SceneCase("stride 512", 6202, 2, 128, 3, 40, 512, S(ALL, 8, 6, 32, alarm=(1, 2, 3), palette=pal[:3])),
        })
    return _SCENES
