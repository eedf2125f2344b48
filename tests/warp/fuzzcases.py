"""The seeded cases of the warp fuzz (tests/warp/test_gpu_fuzz_input.py).  The cases are made here, on the CPU and before any device call: the arena of
seeded random bytes (sources, destinations, meshes and 64 guard bytes around each) and what warpref makes of it -- so tests/test_warp_abi.py can hold
the conditions that keep the fuzz from passing vacuously against warpref alone.  The sources' pixels are the arena's random bytes.

NAMES x FORMATS: 1 x 1; the identity on exactly one tile and on a tile plus one pixel each way; the 8 orientations of 37 x 23 into odd addresses with
padded pitches; a half-pixel translation of 33 x 9; 7 x 5, where NV12's chroma sizes are (n + 1) / 2; each cell size; random meshes with points inside
and outside the frame at 70 x 40 under FILL and CLAMP with both filters; meshes of extreme int32 values; a rotation by 30 degrees from the homography
builder at 48 x 48; 600 x 200 minified into 64 x 16, whose footprint exceeds any LDS budget; a lens mesh at 96 x 64; two tiles at the staged form's
budget, one that fills it to the byte and one that is a row over it; 130 jobs into 130 panes of one surface with a skipped job."""
import functools
import math

import numpy as np

from heat.fuzzcases import GUARD, Arena  # noqa: F401  (GUARD: for the test module)
from warp import warpref

FORMATS = ("bgr", "nv12")
TILE_W, TILE_H = 64, 16                                   # k_warp's tile of destination pixels (ffgpu_warp_tile; tests/test_warp_abi.py compares)
RANDOM = ("random fill bilinear", "random clamp bilinear", "random fill nearest", "random clamp nearest")
WIDE = tuple("wide " + n for n in RANDOM)                 # the same from a source of 260 x 140: every plane's box is over the staged form's budget
NAMES = ("1x1", "identity 64x16", "identity 65x17", "orientations 37x23", "half pixel 33x9", "7x5", "cells") + RANDOM + WIDE + \
        ("extreme", "rotate 30", "minify 600x200 to 64x16", "lens 96x64", "budget", "launch table")


def frame_bytes(fmt, w, h, pad):
    """(pitches, bytes) of a frame: bgr ((pitch,), (n,)); nv12 ((pitch_y, pitch_uv), (n_y, n_uv))"""
    if fmt == "bgr":
        return (3 * w + pad,), ((3 * w + pad) * (h - 1) + 3 * w,)
    py, puv = w + pad, 2 * ((w + 1) // 2) + 2 * (pad // 2)
    return (py, puv), (py * (h - 1) + w, puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2))


def pane_of(fmt, surface, rect):
    """the frame descriptor of the pane rect = (x, y, w, h) of a surface (NV12: x and y even)"""
    x, y, w, h = rect
    if fmt == "bgr":
        off, _, _, pitch = surface
        return (off + y * pitch + 3 * x, w, h, pitch)
    oy, ouv, _, _, py, puv = surface
    assert not (x | y) & 1
    return (oy + y * py + x, ouv + (y // 2) * puv + x, w, h, py, puv)


class Case:
    """one call.  frames / surfaces: (w, h[, pad[, odd]]) each; jobs: (frame index or None, surface index or (surface index, pane rect) or None,
    (points, cell) or None)"""

    def __init__(self, seed, fmt, frames, surfaces, jobs, filt=warpref.BILINEAR, border=warpref.FILL, fill=(7, 77, 177), what=""):
        rng = np.random.default_rng(seed)
        self.fmt, self.filt, self.border, self.fill, self.what = fmt, filt, border, tuple(fill), what
        ar = Arena()

        def place(kind, k, w, h, pad=0, odd=False):
            pitches, sizes = frame_bytes(fmt, w, h, pad)
            if fmt == "bgr":
                return (ar.alloc("%s %d" % (kind, k), sizes[0], 4, odd), w, h, pitches[0])
            oy = ar.alloc("%s %d y" % (kind, k), sizes[0], 4, odd)
            return (oy, ar.alloc("%s %d uv" % (kind, k), sizes[1], 2), w, h, pitches[0], pitches[1])

        self.frames = [place("source", k, *f) for k, f in enumerate(frames)]
        self.surfaces = [place("surface", k, *s) for k, s in enumerate(surfaces)]
        self.meshes = [m for _, _, m in jobs]
        self.mesh_off = [None if m is None else ar.alloc("mesh %d" % k, m[0].nbytes, 8) for k, m in enumerate(self.meshes)]
        self._regs = ar.regs
        self.start = ar.fill(rng)
        for off, m in zip(self.mesh_off, self.meshes):
            if m is not None:
                assert m[0].dtype == np.int32 and m[0].flags.c_contiguous
                self.start[off:off + m[0].nbytes] = m[0].view(np.uint8).reshape(-1)
        self.srcs = [None if f is None else self.frames[f] for f, _, _ in jobs]
        self.dsts = [None if s is None else self.surfaces[s] if isinstance(s, int) else pane_of(fmt, self.surfaces[s[0]], s[1]) for _, s, _ in jobs]
        self.n = len(jobs)
        self.want = warpref.warp(self.start.copy(), fmt, self.srcs, self.dsts, self.meshes, filt, border, self.fill)

    def regions(self):
        return self._regs

    def size(self, d):
        return (d[1], d[2]) if self.fmt == "bgr" else (d[2], d[3])

    def live(self):
        return [k for k in range(self.n) if self.srcs[k] is not None and self.dsts[k] is not None]

    def luma_view(self, buf, k):
        """the first plane's bytes (BGR, or Y) of job k's destination in buf"""
        d = self.dsts[k]
        w, h = self.size(d)
        ch, pitch = (3, d[3]) if self.fmt == "bgr" else (1, d[4])
        return warpref.view(buf, d[0], h, ch * w, pitch)

    def lds_bytes(self, k):
        """per plane of job k that has a staged form (BGR: one; NV12: none, its planes are always read directly): the bytes of LDS each of its tiles
        would need staged (warpref.tile_lds_bytes)"""
        (sw, sh), (dw, dh) = self.size(self.srcs[k]), self.size(self.dsts[k])
        xy, cell = self.meshes[k]
        return [warpref.tile_lds_bytes(xy, cell, sw, sh, dw, dh, 3)] if self.fmt == "bgr" else []

    def tap_stats(self, k):
        """of job k's luma positions: the shares of destination pixels with all taps inside, with a tap outside, with both fractions non-zero"""
        (sw, sh), (dw, dh) = self.size(self.srcs[k]), self.size(self.dsts[k])
        x5, y5 = warpref.luma_positions(self.meshes[k][0], self.meshes[k][1], dw, dh)
        return tuple(float(a.mean()) for a in warpref.taps(x5, y5, sw, sh, self.filt))


def identity(dw, dh, cell=16):
    return warpref.mesh_orient(dw, dh, 0, cell)[1], cell


def random_mesh(rng, sw, sh, dw, dh, cell, reach=0.3):
    """points drawn evenly from the frame and a margin of `reach` of its size round it"""
    mw, mh = warpref.mesh_size(dw, dh, cell)
    x = rng.integers(int(-reach * sw * 256), int((1 + reach) * sw * 256), (mh, mw))
    y = rng.integers(int(-reach * sh * 256), int((1 + reach) * sh * 256), (mh, mw))
    return np.stack([x, y], axis=-1).astype(np.int32), cell


def extreme_mesh(rng, sw, sh, dw, dh, cell):
    """a third of the points INT32_MIN, INT32_MAX or any int32, the others round the frame"""
    xy, _ = random_mesh(rng, sw, sh, dw, dh, cell)
    wild = rng.integers(-2 ** 31, 2 ** 31, xy.shape).astype(np.int32)
    wild[rng.random(xy.shape) < 0.3] = warpref.INT_MIN
    wild[rng.random(xy.shape) < 0.3] = warpref.INT_MAX
    pick = rng.random(xy.shape) < 0.33
    xy[pick] = wild[pick]
    xy[0, 0] = (warpref.INT_MIN, warpref.INT_MAX)
    xy[-1, -1] = (warpref.INT_MAX, warpref.INT_MIN)
    return np.ascontiguousarray(xy), cell


def corner_mesh(bw, nr):
    """the 2 x 2 points of one tile of 64 x 16 with cells of 64 whose source box is bw columns by nr rows: the plane's corner stretched"""
    return np.array([[[0, 0], [(bw - 2) * 256, 0]], [[0, (nr - 2) * 256], [(bw - 2) * 256, (nr - 2) * 256]]], np.int32), 64


def slots(n=130):
    """130 panes of 4 x 3 in a surface of 78 x 40, even origins"""
    return [(6 * (k % 13), 4 * (k // 13), 4, 3) for k in range(n)]


ROT30 = (math.cos(math.pi / 6), -math.sin(math.pi / 6), 23.5 - 23.5 * math.cos(math.pi / 6) + 23.5 * math.sin(math.pi / 6),
         math.sin(math.pi / 6), math.cos(math.pi / 6), 23.5 - 23.5 * math.sin(math.pi / 6) - 23.5 * math.cos(math.pi / 6), 0.0, 0.0, 1.0)      # round the middle of 48 x 48
LENS = dict(model=warpref.LENS_BROWN, dst=(70.0, 70.0, 47.5, 31.5), src=(70.0, 70.0, 47.5, 31.5), k=(-0.3, 0.05, 0.0, 0.0), p=(0.001, -0.002))


def _cases(fmt):
    nv = fmt == "nv12"
    cases = {}

    def add(name, seed, *a, **kw):
        cases[name] = Case(seed + (500 if nv else 0), fmt, *a, what="%s %s" % (fmt, name), **kw)

    rng = np.random.default_rng(9400)
    add("1x1", 9401, [(1, 1)], [(1, 1)], [(0, 0, identity(1, 1, 8))])
    add("identity 64x16", 9402, [(TILE_W, TILE_H)], [(TILE_W, TILE_H, 4)], [(0, 0, identity(TILE_W, TILE_H))])
    add("identity 65x17", 9403, [(TILE_W + 1, TILE_H + 1, 3, True)], [(TILE_W + 1, TILE_H + 1)], [(0, 0, identity(TILE_W + 1, TILE_H + 1, 64))])
    orient = [warpref.mesh_orient(37, 23, k, (8, 16)[k & 1]) for k in range(8)]
    add("orientations 37x23", 9404, [(37, 23, 5, True)], [(wh[0], wh[1], 3 + k, True) for k, (wh, _) in enumerate(orient)],
        [(0, k, (xy, (8, 16)[k & 1])) for k, (_, xy) in enumerate(orient)])
    half = identity(33, 9, 8)
    add("half pixel 33x9", 9405, [(33, 9, 1)], [(33, 9, 2, True)], [(0, 0, (half[0] + np.int32(128), 8))])
    add("7x5", 9406, [(7, 5, 0, True)], [(7, 5, 1)], [(0, 0, random_mesh(rng, 7, 5, 7, 5, 8, 0.1))])
    add("cells", 9407, [(50, 30, 2), (31, 44)], [(70, 40, k) for k in range(4)], [(k & 1, k, random_mesh(rng, (50, 31)[k & 1], (30, 44)[k & 1], 70, 40, c)) for k, c in enumerate(warpref.CELLS)])
    for n, name in enumerate(RANDOM):
        add(name, 9410 + n, [(70, 40, 3, True)], [(70, 40, 5, True)], [(0, 0, random_mesh(rng, 70, 40, 70, 40, 16))],
            filt=warpref.NEAREST if "nearest" in name else warpref.BILINEAR, border=warpref.CLAMP if "clamp" in name else warpref.FILL)
    for n, name in enumerate(WIDE):
        add(name, 9414 + n, [(260, 140, 1, True)], [(70, 40, 2, True)], [(0, 0, random_mesh(rng, 260, 140, 70, 40, 8))],
            filt=warpref.NEAREST if "nearest" in name else warpref.BILINEAR, border=warpref.CLAMP if "clamp" in name else warpref.FILL)
    add("extreme", 9420, [(40, 24, 1)], [(40, 24), (40, 24, 2, True)], [(0, 0, extreme_mesh(rng, 40, 24, 40, 24, 8)), (0, 1, extreme_mesh(rng, 40, 24, 40, 24, 16))])
    add("rotate 30", 9421, [(48, 48, 4)], [(48, 48)], [(0, 0, (warpref.mesh_homography(48, 48, 16, ROT30), 16))])
    mini = (600 / 64, 0, 0, 0, 200 / 16, 0, 0, 0, 1)
    add("minify 600x200 to 64x16", 9422, [(600, 200)], [(64, 16, 4)], [(0, 0, (warpref.mesh_homography(64, 16, 8, mini), 8))])
    add("lens 96x64", 9423, [(96, 64, 0, True)], [(96, 64)], [(0, 0, (warpref.mesh_lens(96, 64, 32, **LENS), 32))])
    bw = 253 if nv else 84                                # rows of (3 x 84 + 6) >> 2 = (253 + 6) >> 2 = 64 dwords: 64 rows fill the budget of 16384 bytes
    add("budget", 9425, [(256, 70, 1, True)], [(TILE_W, TILE_H), (TILE_W, TILE_H, 3)], [(0, 0, corner_mesh(bw, 64)), (0, 1, corner_mesh(bw, 65))])
    add("launch table", 9424, [(9, 7)] * 130, [(78, 40, 2)], [(None if k == 77 else k, (0, s), random_mesh(rng, 9, 7, 4, 3, 8, 0.1)) for k, s in enumerate(slots())])
    return cases


@functools.lru_cache(maxsize=None)
def cases(fmt):
    return _cases(fmt)


def get(fmt, name):
    return cases(fmt)[name]


PARAMS = [(fmt, name) for fmt in FORMATS for name in NAMES]
