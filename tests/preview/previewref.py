"""The preview contract of include/ffcnn_hip.h restated in numpy: resolve, the grid of a wall, the area-averaging rule, and a whole call on an arena
of bytes.  Integers throughout.  tests/test_preview_abi.py pins it to a naive second implementation; the GPU tests compare the device with it byte
for byte."""
import numpy as np

STRETCH, FIT, KEEP_BARS, MAX_SIDE, MAX_PANES = 0, 1, 1, 8192, 4096


class Reject(Exception):
    pass


def resolve(src_w, src_h, dst_w, dst_h, pane, fit, nv12=False):
    """pane = (sx, sy, sw, sh, dx, dy, dw, dh); returns (sx, sy, sw, sh, X0, Y0, ow, oh) or raises Reject"""
    sx, sy, sw, sh, dx, dy, dw, dh = (int(v) for v in pane)
    if (sw == 0) != (sh == 0) or (dw == 0) != (dh == 0):
        raise Reject("half-defaulted")
    if sw == 0:
        if sx or sy:
            raise Reject("default with an origin")
        sw, sh = src_w, src_h
    if dw == 0:
        if dx or dy:
            raise Reject("default with an origin")
        dw, dh = dst_w, dst_h
    if not (1 <= sw <= MAX_SIDE and 1 <= sh <= MAX_SIDE and 1 <= dw <= MAX_SIDE and 1 <= dh <= MAX_SIDE):
        raise Reject("side")
    if sx < 0 or sy < 0 or sx + sw > src_w or sy + sh > src_h or dx < 0 or dy < 0 or dx + dw > dst_w or dy + dh > dst_h:
        raise Reject("outside")
    if nv12 and (sx | sy | dx | dy) & 1:
        raise Reject("odd")
    ow, oh = dw, dh
    if fit == FIT:
        if sw * dh >= sh * dw:
            oh = min(max((2 * sh * dw + sw) // (2 * sw), 1), dh)
        else:
            ow = min(max((2 * sw * dh + sh) // (2 * sh), 1), dw)
    ox, oy = (dw - ow) >> 1, (dh - oh) >> 1
    if nv12:
        ox, oy = ox & ~1, oy & ~1
    return sx, sy, sw, sh, dx + ox, dy + oy, ow, oh


def grid(npanes, cols, dst_w, dst_h, gap=0, nv12=False):
    """the (dx, dy, dw, dh) of a wall's panes, or raises Reject"""
    if npanes < 1 or cols < 1 or cols > npanes or gap < 0 or (nv12 and gap & 1):
        raise Reject("grid")
    rows = -(-npanes // cols)
    cw, ch = (dst_w - (cols + 1) * gap) // cols, (dst_h - (rows + 1) * gap) // rows
    if nv12:
        cw, ch = cw & ~1, ch & ~1
    if cw < 1 or ch < 1:
        raise Reject("no room")
    return [(gap + (k % cols) * (cw + gap), gap + (k // cols) * (ch + gap), cw, ch) for k in range(npanes)]


def weights(s, o):
    """w[i, x]: the length of [i s, (i + 1) s) cut with [x o, (x + 1) o); every row adds up to s"""
    i, x = np.arange(o, dtype=np.int64)[:, None], np.arange(s, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * s, (x + 1) * o) - np.maximum(i * s, x * o))


def resample(plane, ow, oh):
    """plane (sh, sw[, channels]) of bytes to (oh, ow[, channels]) by the rule, every channel on its own"""
    v = np.asarray(plane).astype(np.int64)
    sh, sw = v.shape[:2]
    wx, wy = weights(sw, ow), weights(sh, oh)
    inner = np.tensordot(v, wx, axes=([1], [1]))                     # (sh, [channels,] ow)
    outer = np.tensordot(wy, inner, axes=([1], [0]))                 # (oh, [channels,] ow)
    if v.ndim == 3:
        outer = outer.transpose(0, 2, 1)
    D = sw * sh
    return ((outer + (D >> 1)) // D).astype(np.uint8)


def view(buf, off, rows, rowbytes, pitch):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, rowbytes), strides=(pitch, 1), writeable=True)


def _plane(buf, src, dst, region, pane, image, ch, fill, keep, trace):
    """one plane of one pane: src / dst = (offset, pitch) in buf; region, pane, image = (x, y, w, h) in samples of ch bytes"""
    (soff, sp), (doff, dp) = src, dst
    sx, sy, sw, sh = region
    px, py, pw, ph = pane
    ix, iy, ow, oh = image
    s = view(buf, soff + sy * sp + ch * sx, sh, ch * sw, sp).reshape(sh, sw, ch).copy()
    out = resample(s, ow, oh)
    d = view(buf, doff + py * dp + ch * px, ph, ch * pw, dp)
    if not keep:
        d[...] = np.tile(np.asarray(fill, np.uint8), pw)[None, :]
    d[iy - py:iy - py + oh, ch * (ix - px):ch * (ix - px + ow)] = out.reshape(oh, ch * ow)
    if trace is not None:
        trace["image_bytes"] = trace.get("image_bytes", 0) + out.size
        trace["bar_bytes"] = trace.get("bar_bytes", 0) + ch * (pw * ph - ow * oh)


def preview(buf, fmt, srcs, dsts, panes, fit=STRETCH, fill=(0, 0, 0), keep=False, trace=None):
    """a whole call on the arena `buf` (changed in place).  srcs / dsts: per pane None (skipped) or, with offsets into buf, (off, w, h, pitch) for
    "bgr" and (off_y, off_uv, w, h, pitch_y, pitch_uv) for "nv12"; panes: 8-tuples.  Sources are read as the panes before them left them."""
    for s, d, p in zip(srcs, dsts, panes):
        if s is None or d is None:
            continue
        if fmt == "bgr":
            r = resolve(s[1], s[2], d[1], d[2], p, fit)
            dw, dh = (p[6], p[7]) if p[6] else (d[1], d[2])
            _plane(buf, (s[0], s[3]), (d[0], d[3]), r[:4], (p[4], p[5], dw, dh), r[4:], 3, fill, keep, trace)
        else:
            r = resolve(s[2], s[3], d[2], d[3], p, fit, True)
            dw, dh = (p[6], p[7]) if p[6] else (d[2], d[3])
            sx, sy, sw, sh, X0, Y0, ow, oh = r
            _plane(buf, (s[0], s[4]), (d[0], d[4]), r[:4], (p[4], p[5], dw, dh), r[4:], 1, fill[:1], keep, trace)
            _plane(buf, (s[1], s[5]), (d[1], d[5]), (sx // 2, sy // 2, (sw + 1) // 2, (sh + 1) // 2), (p[4] // 2, p[5] // 2, (dw + 1) // 2, (dh + 1) // 2),
                   (X0 // 2, Y0 // 2, (ow + 1) // 2, (oh + 1) // 2), 2, fill[1:3], keep, trace)
    return buf
