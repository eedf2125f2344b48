"""The convert surfaces' contract (include/ffcnn_hip.h) restated in numpy: one function per destination, to_bgr and to_nv12, on a source given as
its planes -- uint8 arrays of (rows, at least the least row bytes), P010's 16-bit samples as their little-endian bytes.  Integers (int64) throughout,
>> arithmetic, clamps last."""
import numpy as np

FORMATS = ("BGR24", "RGB24", "BGRA32", "RGBA32", "GRAY8", "NV12", "NV21", "I420", "YV12", "YUY2", "UYVY", "P010")       # FFGPU_PIX_*, by value
YUV2RGB = ((16, 298, 409, 100, 208, 516), (0, 256, 359, 88, 183, 454), (16, 298, 459, 55, 136, 541), (0, 256, 403, 48, 120, 475))      # FFGPU_YUV_*
RGB2YUV = ((16, 66, 129, 25, -38, -74, 112, 112, -94, -18), (0, 77, 150, 29, -43, -85, 128, 128, -107, -21),
           (16, 47, 157, 16, -26, -86, 112, 112, -102, -10), (0, 54, 183, 19, -29, -99, 128, 128, -116, -12))


def planes(fmt, w, h):
    """[(rows, the least bytes of a row, the alignment of the plane's address and pitch)] of a w x h surface"""
    cw, ch, name = (w + 1) // 2, (h + 1) // 2, FORMATS[fmt]
    if name in ("NV12", "NV21"):
        return [(h, w, 1), (ch, 2 * cw, 2)]
    if name in ("I420", "YV12"):
        return [(h, w, 1), (ch, cw, 1), (ch, cw, 1)]
    if name == "P010":
        return [(h, 2 * w, 2), (ch, 4 * cw, 2)]
    return [(h, {"BGR24": 3 * w, "RGB24": 3 * w, "BGRA32": 4 * w, "RGBA32": 4 * w, "GRAY8": w}.get(name, 4 * cw), 1)]


def _samples(fmt, p, w, h):
    """("rgb", B G R of (h, w, 3)), ("gray", Y) or ("420" / "422", (Y, U, V)) as int64, U before V, P010 reduced"""
    cw, ch, name = (w + 1) // 2, (h + 1) // 2, FORMATS[fmt]
    if name == "P010":
        p = [np.minimum(((np.ascontiguousarray(q[:, :n]).view("<u2").astype(np.int64) >> 6) + 2) >> 2, 255) for q, n in zip(p, (2 * w, 4 * cw))]
    p = [np.asarray(q).astype(np.int64) for q in p]
    if name in ("BGR24", "RGB24", "BGRA32", "RGBA32"):
        n = 3 if name.endswith("24") else 4
        px = p[0][:, :n * w].reshape(h, w, n)[..., :3]
        return "rgb", px[..., ::-1] if name[0] == "R" else px
    if name == "GRAY8":
        return "gray", p[0][:, :w]
    if name in ("NV12", "NV21", "P010"):
        uv = p[1][:, :2 * cw].reshape(ch, cw, 2)
        return "420", (p[0][:, :w], uv[..., int(name == "NV21")], uv[..., int(name != "NV21")])
    if name in ("I420", "YV12"):
        return "420", (p[0][:, :w], p[1 + (name == "YV12")][:, :cw], p[2 - (name == "YV12")][:, :cw])
    g, o = p[0][:, :4 * cw].reshape(h, cw, 4), int(name == "UYVY")
    return "422", (g[..., o::2].reshape(h, 2 * cw)[:, :w], g[..., 1 - o], g[..., 3 - o])


def _clip(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def to_bgr(fmt, p, w, h, matrix=0):
    """the (h, w, 3) uint8 B G R image of the surface"""
    kind, d = _samples(fmt, p, w, h)
    if kind == "rgb":
        return _clip(d)
    if kind == "gray":
        return _clip(np.repeat(d[..., None], 3, 2))
    Y, U, V = d
    yi, xi = np.arange(h)[:, None] >> int(kind == "420"), np.arange(w)[None, :] >> 1      # the nearest chroma sample
    yoff, cy, crv, cgu, cgv, cbu = YUV2RGB[matrix]
    c, dd, e = cy * (Y - yoff) + 128, U[yi, xi] - 128, V[yi, xi] - 128
    return _clip(np.stack([(c + cbu * dd) >> 8, (c - cgu * dd - cgv * e) >> 8, (c + crv * e) >> 8], -1))


def to_nv12(fmt, p, w, h, matrix=0):
    """(Y of (h, w), U V of ((h + 1) / 2, 2 ((w + 1) / 2))) uint8 of the surface"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    kind, d = _samples(fmt, p, w, h)
    if kind == "rgb":
        yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb = RGB2YUV[matrix]
        B, G, R = d[..., 0], d[..., 1], d[..., 2]
        Y = ((yr * R + yg * G + yb * B + 128) >> 8) + yoff
        S = np.zeros((2 * ch, 2 * cw, 4), np.int64)                                   # B G R and the count of the block's pixels inside the frame
        S[:h, :w, :3], S[:h, :w, 3] = d, 1
        S = S.reshape(ch, 2, cw, 2, 4).sum((1, 3))
        n = S[..., 3]
        B, G, R = ((S[..., k] + (n >> 1)) >> (n >> 1) for k in range(3))               # (n = 1, 2, 4: log2 n = n >> 1)
        U, V = ((ur * R + ug * G + ub * B + 128) >> 8) + 128, ((vr * R + vg * G + vb * B + 128) >> 8) + 128
    elif kind == "gray":
        Y, U, V = d, np.full((ch, cw), 128), np.full((ch, cw), 128)
    else:
        Y, U, V = d
        if kind == "422":                                                              # the two rows' mean, or the lone last row
            U, V = (np.concatenate([(c[0:h - 1:2] + c[1::2] + 1) >> 1, c[h - 1:h] if h & 1 else c[:0]]) for c in (U, V))
    return _clip(Y), _clip(np.stack([U, V], -1).reshape(ch, 2 * cw))
