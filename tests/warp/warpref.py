"""The warp contract of include/ffcnn_hip.h restated in numpy: the mesh's size, the builders (orientations, homography, lens), the interpolation rule,
the sampling rule, and a whole call on an arena of bytes.  Integers throughout but the builders' doubles.  tests/test_warp_abi.py pins it to a naive
second implementation; the GPU tests compare the device with it byte for byte."""
import numpy as np

MESH_ONE, SUB, BILINEAR, NEAREST, FILL, CLAMP, MAX_SIDE, MAX_JOBS, LENS_BROWN, LENS_EQUIDISTANT = 256, 32, 0, 1, 0, 1, 8192, 4096, 0, 1
CELLS = (8, 16, 32, 64)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
INVERSE = (0, 3, 2, 1, 4, 5, 6, 7)                                                      # orient k followed by INVERSE[k] is the identity


class Reject(Exception):
    pass


def mesh_size(dw, dh, cell):
    if not (1 <= dw <= MAX_SIDE and 1 <= dh <= MAX_SIDE) or cell not in CELLS:
        raise Reject("mesh size")
    return (dw - 1) // cell + 2, (dh - 1) // cell + 2


def _grid(dw, dh, cell):
    """the destination pixels (i, j) of the mesh's points as int64 arrays of shape (mh, mw)"""
    mw, mh = mesh_size(dw, dh, cell)
    return np.meshgrid(np.arange(mw, dtype=np.int64) * cell, np.arange(mh, dtype=np.int64) * cell)


def fix(v):
    """floor(v * 256 + 0.5) saturated to int32; INT32_MIN where v is not finite"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(v * 256.0 + 0.5)
    out = np.clip(np.where(np.isfinite(v), t, float(INT_MIN)), float(INT_MIN), float(INT_MAX))
    return out.astype(np.int64).astype(np.int32)


def mesh_orient(sw, sh, orient, cell):
    """((dw, dh), points (mh, mw, 2) int32): the table of the header"""
    if not (1 <= sw <= MAX_SIDE and 1 <= sh <= MAX_SIDE) or not 0 <= orient <= 7:
        raise Reject("orient")
    dw, dh = (sh, sw) if orient & 1 else (sw, sh)
    i, j = _grid(dw, dh, cell)
    W1, H1 = sw - 1, sh - 1
    x, y = ((i, j), (j, H1 - i), (W1 - i, H1 - j), (W1 - j, i), (W1 - i, j), (W1 - j, H1 - i), (i, H1 - j), (j, i))[orient]
    return (dw, dh), np.stack([x * MESH_ONE, y * MESH_ONE], axis=-1).astype(np.int32)


def mesh_homography(dw, dh, cell, h):
    h = [float(v) for v in h]
    i, j = (g.astype(np.float64) for g in _grid(dw, dh, cell))
    with np.errstate(all="ignore"):
        den = (h[6] * i + h[7] * j) + h[8]
        x = ((h[0] * i + h[1] * j) + h[2]) / den
        y = ((h[3] * i + h[4] * j) + h[5]) / den
    ok = den > 0
    return np.stack([np.where(ok, fix(x), INT_MIN), np.where(ok, fix(y), INT_MIN)], axis=-1).astype(np.int32)


def mesh_lens(dw, dh, cell, model, dst, src, k=(0, 0, 0, 0), p=(0, 0)):
    if model not in (LENS_BROWN, LENS_EQUIDISTANT) or not (np.isfinite(dst[0]) and np.isfinite(dst[1]) and dst[0] > 0 and dst[1] > 0):
        raise Reject("lens")
    dst, src, k, p = ([float(v) for v in a] for a in (dst, src, k, p))
    i, j = (g.astype(np.float64) for g in _grid(dw, dh, cell))
    with np.errstate(all="ignore"):
        xn, yn = (i - dst[2]) / dst[0], (j - dst[3]) / dst[1]
        r2 = xn * xn + yn * yn
        if model == LENS_BROWN:
            rad = 1.0 + ((k[2] * r2 + k[1]) * r2 + k[0]) * r2
            xd = xn * rad + ((2.0 * p[0]) * (xn * yn) + p[1] * (r2 + (2.0 * xn) * xn))
            yd = yn * rad + (p[0] * (r2 + (2.0 * yn) * yn) + (2.0 * p[1]) * (xn * yn))
        else:
            r = np.sqrt(r2)
            theta = np.arctan(r)
            t2 = theta * theta
            theta_d = theta * (1.0 + ((((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2))
            scale = np.where(r > 0, theta_d / np.where(r > 0, r, 1.0), 1.0)
            xd, yd = xn * scale, yn * scale
        return np.stack([fix(src[0] * xd + src[2]), fix(src[1] * yd + src[3])], axis=-1)


def points(xy, cell, dw, dh, step=1):
    """X8, Y8 (int64 arrays) of the destination pixels (step i, step j) that lie inside dw x dh: the interpolation rule.  step 2: the luma pixels the
    chroma samples take"""
    s = cell.bit_length() - 1
    xy = np.asarray(xy)
    assert xy.shape == (mesh_size(dw, dh, cell)[1], mesh_size(dw, dh, cell)[0], 2) and xy.dtype == np.int32
    P = xy.astype(np.int64)
    i, j = np.meshgrid(np.arange(0, dw, step, dtype=np.int64), np.arange(0, dh, step, dtype=np.int64))
    ci, a, cj, b = i >> s, i & (cell - 1), j >> s, j & (cell - 1)
    out = []
    for ch in (0, 1):
        p = P[:, :, ch]
        S = (cell - b) * ((cell - a) * p[cj, ci] + a * p[cj, ci + 1]) + b * ((cell - a) * p[cj + 1, ci] + a * p[cj + 1, ci + 1])
        out.append((S + (1 << (2 * s - 1))) >> (2 * s))
    return out[0], out[1]


def taps(x5, y5, sw, sh, filt):
    """per destination sample: (all taps inside the frame, some tap outside, both fractions of the position non-zero) as boolean arrays"""
    frac = ((x5 & 31) != 0) & ((y5 & 31) != 0)
    if filt == NEAREST:
        x, y = (x5 + 16) >> 5, (y5 + 16) >> 5
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        return inside, ~inside, frac
    x0, y0 = x5 >> 5, y5 >> 5
    inside = (x0 >= 0) & (x0 + 1 < sw) & (y0 >= 0) & (y0 + 1 < sh)
    return inside, ~inside, frac


def sample(plane, x5, y5, filt, border, fill):
    """plane (sh, sw, ch) of bytes sampled at the positions x5, y5 (int64 arrays of one shape, in 1 / 32 sample): (..., ch) bytes"""
    v = np.asarray(plane).astype(np.int64)
    sh, sw, ch = v.shape
    fill = np.asarray(fill, np.int64).reshape(1, 1, ch)

    def tap(x, y):
        t = v[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]
        if border == CLAMP:
            return t
        return np.where(((x >= 0) & (x < sw) & (y >= 0) & (y < sh))[..., None], t, fill)

    if filt == NEAREST:
        return tap((x5 + 16) >> 5, (y5 + 16) >> 5).astype(np.uint8)
    x0, fx, y0, fy = x5 >> 5, (x5 & 31)[..., None], y5 >> 5, (y5 & 31)[..., None]
    out = ((32 - fy) * ((32 - fx) * tap(x0, y0) + fx * tap(x0 + 1, y0)) + fy * ((32 - fx) * tap(x0, y0 + 1) + fx * tap(x0 + 1, y0 + 1)) + 512) >> 10
    return out.astype(np.uint8)


def luma_positions(xy, cell, dw, dh):
    X8, Y8 = points(xy, cell, dw, dh)
    return (X8 + 4) >> 3, (Y8 + 4) >> 3


def chroma_positions(xy, cell, dw, dh):
    X8, Y8 = points(xy, cell, dw, dh, 2)
    return (X8 + 8) >> 4, (Y8 + 8) >> 4


def warp_plane(plane, xy, cell, dw, dh, filt=BILINEAR, border=FILL, fill=(0, 0, 0)):
    """a BGR (sh, sw, 3) or Y (sh, sw) plane through the mesh into (dh, dw[, 3])"""
    p = np.asarray(plane)
    x5, y5 = luma_positions(xy, cell, dw, dh)
    if p.ndim == 2:
        return sample(p[:, :, None], x5, y5, filt, border, fill[:1])[:, :, 0]
    return sample(p, x5, y5, filt, border, fill)


def warp_chroma(uv, xy, cell, dw, dh, filt=BILINEAR, border=FILL, fill=(0, 0)):
    """the U V plane ((sh + 1) / 2, (sw + 1) / 2, 2) through the mesh of the dw x dh LUMA destination into ((dh + 1) / 2, (dw + 1) / 2, 2)"""
    x5, y5 = chroma_positions(xy, cell, dw, dh)
    return sample(uv, x5, y5, filt, border, fill)


TILE_W, TILE_H, LDS_BYTES = 64, 16, 16384


def tile_lds_bytes(xy, cell, sw, sh, dw, dh, ch, half=0):
    """The staged form's choice restated: for every 64 x 16 tile of a destination plane of dw x dh samples (ch channels; half = 1: the U V plane, whose
    samples take the mesh at luma pixel (2 i, 2 j)) the bytes of LDS its source box needs -- the bounding box of the mesh points of the cells the tile
    touches, as tap coordinates plus one, clipped to the sw x sh plane, rows of (ch columns + 6) >> 2 dwords.  A tile is staged where that is at
    most LDS_BYTES."""
    s = cell.bit_length() - 1
    P = np.asarray(xy).astype(np.int64)
    out = []
    for ty0 in range(0, dh, TILE_H):
        for tx0 in range(0, dw, TILE_W):
            ci0, ci1 = (tx0 << half) >> s, (((min(tx0 + TILE_W, dw) - 1) << half) >> s) + 1
            cj0, cj1 = (ty0 << half) >> s, (((min(ty0 + TILE_H, dh) - 1) << half) >> s) + 1
            box = P[cj0:cj1 + 1, ci0:ci1 + 1]
            span = []
            for k, n in ((0, sw), (1, sh)):
                lo, hi = int(box[:, :, k].min()), int(box[:, :, k].max())
                a, b = ((lo + (4 << half)) >> (3 + half)) >> 5, (((hi + (4 << half)) >> (3 + half)) >> 5) + 1
                span.append(min(max(b, 0), n - 1) - min(max(a, 0), n - 1) + 1)
            out.append(4 * span[1] * ((ch * span[0] + 6) >> 2))
    return out


def view(buf, off, rows, rowbytes, pitch):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, rowbytes), strides=(pitch, 1), writeable=True)


def warp(buf, fmt, srcs, dsts, meshes, filt=BILINEAR, border=FILL, fill=(0, 0, 0)):
    """a whole call on the arena `buf` (changed in place).  srcs / dsts: per job None (skipped) or, with offsets into buf, (off, w, h, pitch) for "bgr"
    and (off_y, off_uv, w, h, pitch_y, pitch_uv) for "nv12"; meshes: per job (points (mh, mw, 2) int32, cell).  Sources are read as the jobs before them
    left them."""
    for s, d, m in zip(srcs, dsts, meshes):
        if s is None or d is None:
            continue
        xy, cell = m
        if fmt == "bgr":
            (so, sw, sh, sp), (do, dw, dh, dp) = s, d
            src = view(buf, so, sh, 3 * sw, sp).reshape(sh, sw, 3).copy()
            view(buf, do, dh, 3 * dw, dp)[...] = warp_plane(src, xy, cell, dw, dh, filt, border, fill).reshape(dh, 3 * dw)
        else:
            (sy, suv, sw, sh, spy, spuv), (dy, duv, dw, dh, dpy, dpuv) = s, d
            y = view(buf, sy, sh, sw, spy).copy()
            uv = view(buf, suv, (sh + 1) // 2, 2 * ((sw + 1) // 2), spuv).reshape((sh + 1) // 2, (sw + 1) // 2, 2).copy()
            view(buf, dy, dh, dw, dpy)[...] = warp_plane(y, xy, cell, dw, dh, filt, border, fill)
            view(buf, duv, (dh + 1) // 2, 2 * ((dw + 1) // 2), dpuv)[...] = warp_chroma(uv, xy, cell, dw, dh, filt, border, fill[1:3]).reshape((dh + 1) // 2, 2 * ((dw + 1) // 2))
    return buf
