"""The seeded cases of the preview fuzz (tests/preview/test_gpu_fuzz_input.py).  The cases are made here, on the CPU and before any device call: the
arena of seeded random bytes (sources, destination surfaces and 64 guard bytes around each) and what previewref makes of it -- so
tests/test_preview_abi.py can hold the conditions that keep the fuzz from passing vacuously against previewref alone.  The sources' pixels are the
arena's random bytes unless a case paints them.

NAMES x FORMATS: 1 x 1; 7 x 5 -> 3 x 2; 5 x 3 -> 17 x 11; a copy of 64 x 64; exactly 2 : 1 with an odd result and 4 : 1; 67 x 35 -> 16 x 9 into an odd
byte address with padded pitches; an image of two tiles and a pixel each way from a source 3.7 times as large; FIT with bars above and below, and
with kept bars left and right; the clamp of FIT to one row; a source region at an odd (NV12: even) origin of a larger padded frame; a wall of 2 x 3
panes of six sizes with a skipped pane; 130 panes into 130 slots of one surface.  NV12 only: a Y plane whose sums pass 2^32."""
import functools

import numpy as np

from heat.fuzzcases import GUARD, Arena  # noqa: F401  (GUARD: for the test module)
from preview import previewref

FORMATS = ("bgr", "nv12")
TILE_W, TILE_H = 64, 16                                   # k_preview's tile of destination samples (ffgpu_preview_tile; tests/test_preview_abi.py compares)
NAMES = ("1x1", "7x5 to 3x2", "5x3 to 17x11", "64x64 copy", "130x66 to 65x33", "128x64 to 32x16", "seam 67x35 to 16x9", "wide tile", "fit wide in tall",
         "fit tall in wide keep", "fit clamp", "zoom", "wall", "launch table")
WIDE = "wide sum"


def frame_bytes(fmt, w, h, pad):
    """(pitches, bytes) of a frame: bgr ((pitch,), n); nv12 ((pitch_y, pitch_uv), (n_y, n_uv))"""
    if fmt == "bgr":
        return (3 * w + pad,), ((3 * w + pad) * (h - 1) + 3 * w,)
    py, puv = w + pad, 2 * ((w + 1) // 2) + 2 * (pad // 2)
    return (py, puv), (py * (h - 1) + w, puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2))


class Case:
    """one call.  frames / surfaces: (w, h[, pad[, odd]]) each; panes: (frame index or None, surface index or None, 8-tuple)"""

    def __init__(self, seed, fmt, frames, surfaces, panes, fit=previewref.STRETCH, fill=(7, 77, 177), keep=False, paint=None, what=""):
        rng = np.random.default_rng(seed)
        self.fmt, self.fit, self.fill, self.keep, self.what = fmt, fit, tuple(fill), keep, what
        ar = Arena()

        def place(kind, k, w, h, pad=0, odd=False):
            pitches, sizes = frame_bytes(fmt, w, h, pad)
            if fmt == "bgr":
                return (ar.alloc("%s %d" % (kind, k), sizes[0], 4, odd), w, h, pitches[0])
            oy = ar.alloc("%s %d y" % (kind, k), sizes[0], 4, odd)
            return (oy, ar.alloc("%s %d uv" % (kind, k), sizes[1], 2), w, h, pitches[0], pitches[1])

        self.frames = [place("source", k, *f) for k, f in enumerate(frames)]
        self.surfaces = [place("surface", k, *s) for k, s in enumerate(surfaces)]
        self._regs = ar.regs
        self.start = ar.fill(rng)
        if paint:
            paint(self, rng)
        self.srcs = [None if f is None else self.frames[f] for f, _, _ in panes]
        self.dsts = [None if s is None else self.surfaces[s] for _, s, _ in panes]
        self.panes = [tuple(p) for _, _, p in panes]
        self.n = len(panes)
        self.trace = {}
        self.want = previewref.preview(self.start.copy(), fmt, self.srcs, self.dsts, self.panes, fit, self.fill, keep, self.trace)

    def regions(self):
        return self._regs

    def size(self, d):
        return (d[1], d[2]) if self.fmt == "bgr" else (d[2], d[3])

    def resolved(self, p):
        """(sx, sy, sw, sh, X0, Y0, ow, oh) and the pane (dx, dy, dw, dh) of live pane p"""
        (sw_, sh_), (dw_, dh_) = self.size(self.srcs[p]), self.size(self.dsts[p])
        r = previewref.resolve(sw_, sh_, dw_, dh_, self.panes[p], self.fit, self.fmt == "nv12")
        q = self.panes[p]
        return r, ((q[4], q[5], q[6], q[7]) if q[6] else (0, 0, dw_, dh_))

    def luma_view(self, buf, p, rect):
        """the first plane's bytes (BGR, or Y) of `rect` = (x, y, w, h) of pane p's destination surface in buf"""
        d = self.dsts[p]
        ch, pitch = (3, d[3]) if self.fmt == "bgr" else (1, d[4])
        x, y, w, h = rect
        return previewref.view(buf, d[0] + y * pitch + ch * x, h, ch * w, pitch)

    def live(self):
        return [p for p in range(self.n) if self.srcs[p] is not None and self.dsts[p] is not None]


def slots(fmt, n=130):
    """130 slots of 4 x 3 in a surface of 78 x 40, even origins"""
    return [(6 * (k % 13), 4 * (k // 13), 4, 3) for k in range(n)]


def _cases(fmt):
    nv = fmt == "nv12"
    cases = {}

    def add(name, seed, *a, **kw):
        cases[name] = Case(seed + (500 if nv else 0), fmt, *a, what="%s %s" % (fmt, name), **kw)

    whole = (0,) * 8
    add("1x1", 9101, [(1, 1)], [(1, 1)], [(0, 0, whole)])
    add("7x5 to 3x2", 9102, [(7, 5)], [(3, 2)], [(0, 0, whole)])
    add("5x3 to 17x11", 9103, [(5, 3, 3)], [(17, 11, 2)], [(0, 0, whole)])
    add("64x64 copy", 9104, [(64, 64)], [(64, 64, 4)], [(0, 0, whole)])
    add("130x66 to 65x33", 9105, [(130, 66)], [(65, 33)], [(0, 0, whole)])
    add("128x64 to 32x16", 9106, [(128, 64, 8)], [(32, 16)], [(0, 0, whole)])
    add("seam 67x35 to 16x9", 9107, [(67, 35, 5, True)], [(16, 9, 7, True)], [(0, 0, whole)])
    add("wide tile", 9108, [(477, 122, 3, True)], [(2 * TILE_W + 1, 2 * TILE_H + 1, 1)], [(0, 0, whole)])
    add("fit wide in tall", 9109, [(40, 10, 2)], [(16, 24, 6)], [(0, 0, (0, 0, 0, 0, 2, 2, 12, 20))], fit=previewref.FIT)
    add("fit tall in wide keep", 9110, [(10, 40)], [(34, 14, 2)], [(0, 0, (0, 0, 0, 0, 2, 2, 30, 12))], fit=previewref.FIT, keep=True)
    add("fit clamp", 9111, [(200, 1)], [(8, 8)], [(0, 0, whole)], fit=previewref.FIT)
    add("zoom", 9112, [(50, 40, 6)], [(20, 15, 2)], [(0, 0, (6, 4, 21, 13, 2, 2, 10, 9) if nv else (7, 5, 21, 13, 3, 2, 10, 9))])
    sizes = [(31, 17), (64, 48, 4), (9, 5), (45, 17), (100, 30, 2, True), (23, 41)]
    g = previewref.grid(6, 2, 97, 61, 2, nv)
    add("wall", 9113, sizes, [(97, 61, 3)], [(None if k == 4 else k, 0, (0, 0, 0, 0) + g[k]) for k in range(6)], fit=previewref.FIT, fill=(1, 2, 3))
    add("launch table", 9114, [(9, 7)] * 130, [(78, 40, 2)], [(k, 0, (0, 0, 0, 0) + s) for k, s in enumerate(slots(fmt))])
    return cases


@functools.lru_cache(maxsize=None)
def cases(fmt):
    return _cases(fmt)


def _bright(c, rng):
    """every Y byte 250 or more, nine in ten 255: 255 D passes 2^32 by 0.4 % only, so the mean has to lie above 254.1 for the sums to pass it too"""
    oy, _, w, h, py, _ = c.frames[0]
    y = rng.integers(250, 256, (h, w), dtype=np.uint8)
    y[rng.random((h, w)) < 0.9] = 255
    previewref.view(c.start, oy, h, w, py)[...] = y


@functools.lru_cache(maxsize=None)
def wide_sum():
    """NV12 only, built when asked for: a Y plane of 8192 x 2064 into 3 x 2 -- D = 8192 * 2064, 255 D >= 2^32; its U V plane of 4096 x 1032 stays on
    the narrow path"""
    return Case(9120, "nv12", [(8192, 2064)], [(3, 2)], [(0, 0, (0,) * 8)], paint=_bright, what="nv12 wide sum")


def get(fmt, name):
    return wide_sum() if name == WIDE else cases(fmt)[name]


PARAMS = [(fmt, name) for fmt in FORMATS for name in NAMES] + [("nv12", WIDE)]
