"""numpy restatement of the drawing contract of include/ffcnn_hip.h (ffgpu_draw_boxes_*_dev, ffgpu_exec_draw_*): the boxes of one target drawn
serially in list order on a uint8 buffer with pitch, each as the reference's bmp_rectangle draws it (bmpfile.c:121-156) -- two loops, four
pixels per step, every pixel dropped when it lies outside the target.  rectangle_literal is those loops word for word; rectangle is the same
pixel set with the loop ranges clipped first and rows / columns written as slices (a box of +-1e30 must not take forever); tests/test_overlay_abi.py
holds the two against each other.  Nothing here knows how the device parallelises."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def f2i(v):
    """(int)v as the contract defines it: toward zero, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    if v >= 2.0 ** 31:
        return INT_MAX
    if v <= -2.0 ** 31:
        return INT_MIN
    return int(v)


def corners(box):
    return f2i(box["x1"]), f2i(box["y1"]), f2i(box["x2"]), f2i(box["y2"])


def colours_of(boxes, color=(0, 255, 0), palette=None):
    """one (c0, c1, c2) per box: palette[type mod len(palette)] (the non-negative remainder), or `color`"""
    if palette is None:
        return [tuple(int(c) for c in color[:3])] * len(boxes)
    return [tuple(int(c) for c in palette[int(t) % len(palette)][:3]) for t in boxes["type"]]


def rectangle_literal(put, x1, y1, x2, y2):
    """bmp_rectangle, bmpfile.c:145-156: put(x, y) is bmp_setpixel with the colour bound"""
    for i in range(x1, x2 + 1):
        put(i, y1)
        put(i, y2)
    for i in range(y1, y2 + 1):
        put(x1, i)
        put(x2, i)


def rectangle(row, col, w, h, x1, y1, x2, y2):
    """the same pixel set through row(y, xa, xb) / col(x, ya, yb) (inclusive ranges inside the target); returns (pixels drawn, pixels of the
    set that the target dropped), both counted per put"""
    xa, xb, ya, yb = max(x1, 0), min(x2, w - 1), max(y1, 0), min(y2, h - 1)
    lh, lv = max(0, xb - xa + 1), max(0, yb - ya + 1)
    drawn = 0
    for y in (y1, y2):
        if 0 <= y < h and lh:
            row(y, xa, xb)
            drawn += lh
    for x in (x1, x2):
        if 0 <= x < w and lv:
            col(x, ya, yb)
            drawn += lv
    return drawn, 2 * max(0, x2 - x1 + 1) + 2 * max(0, y2 - y1 + 1) - drawn


def _stats_box(stats, drawn, dropped):
    if stats is None:
        return
    stats["boxes"] = stats.get("boxes", 0) + 1
    key = "outside" if drawn == 0 else ("clipped" if dropped else "inside")
    stats[key] = stats.get(key, 0) + 1


def _view(buf, base, shape, strides):
    return np.lib.stride_tricks.as_strided(buf[base:], shape=shape, strides=strides, writeable=True)


def draw_bgr(buf, base, w, h, pitch, boxes, colours, thickness=1, stats=None):
    """draws into the flat uint8 array `buf`, whose byte `base` is row 0 of a w x h BGR target with `pitch` bytes between rows.  stats (a dict)
    accumulates: boxes, outside (nothing drawn), inside (nothing dropped), clipped, and overwritten: pixels a later box of another colour took"""
    px = _view(buf, base, (h, w, 3), (pitch, 3, 1))
    owner = np.zeros((h, w), np.int32)                                            # 1 + packed colour of the box that drew the pixel last
    over = 0
    for box, c in zip(boxes, colours):
        a, b, cc, d = corners(box)
        tag = 1 + (c[0] | c[1] << 8 | c[2] << 16)

        def mark(o):
            nonlocal over
            over += int(np.count_nonzero((o != 0) & (o != tag)))
            o[...] = tag

        def row(y, xa, xb):
            px[y, xa:xb + 1] = c
            mark(owner[y, xa:xb + 1])

        def col(x, ya, yb):
            px[ya:yb + 1, x] = c
            mark(owner[ya:yb + 1, x])
        drawn = dropped = 0
        for i in range(thickness):
            n, m = rectangle(row, col, w, h, a + i, b + i, cc - i, d - i)
            drawn, dropped = drawn + n, dropped + m
        _stats_box(stats, drawn, dropped)
    if stats is not None:
        stats["overwritten"] = stats.get("overwritten", 0) + over
    return buf


def draw_nv12(buf, base_y, base_uv, w, h, pitch_y, pitch_uv, boxes, colours, thickness=1, stats=None):
    """the NV12 form: byte base_y of `buf` is row 0 of the Y plane, byte base_uv row 0 of the interleaved U V plane ((h + 1) / 2 rows of
    (w + 1) / 2 pairs); colours are (Y, U, V).  A drawn pixel (x, y) sets Y[y][x] and the pair UV[y >> 1][x >> 1], box after box"""
    Y = _view(buf, base_y, (h, w), (pitch_y, 1))
    UV = _view(buf, base_uv, ((h + 1) // 2, (w + 1) // 2, 2), (pitch_uv, 2, 1))
    owner = np.zeros((h, w), np.int32)
    over = 0
    for box, c in zip(boxes, colours):
        a, b, cc, d = corners(box)
        tag = 1 + (c[0] | c[1] << 8 | c[2] << 16)

        def mark(o):
            nonlocal over
            over += int(np.count_nonzero((o != 0) & (o != tag)))
            o[...] = tag

        def row(y, xa, xb):
            Y[y, xa:xb + 1] = c[0]
            UV[y >> 1, xa >> 1:(xb >> 1) + 1] = c[1:]
            mark(owner[y, xa:xb + 1])

        def col(x, ya, yb):
            Y[ya:yb + 1, x] = c[0]
            UV[ya >> 1:(yb >> 1) + 1, x >> 1] = c[1:]
            mark(owner[ya:yb + 1, x])
        drawn = dropped = 0
        for i in range(thickness):
            n, m = rectangle(row, col, w, h, a + i, b + i, cc - i, d - i)
            drawn, dropped = drawn + n, dropped + m
        _stats_box(stats, drawn, dropped)
    if stats is not None:
        stats["overwritten"] = stats.get("overwritten", 0) + over
    return buf


def bmp_file(rows_top_down, w, h):
    """the 24-bit BMP the demo's image_save writes (54-byte header, rows bottom-up) of an (h, ALIGN(3 w, 4)) uint8 array"""
    pitch = (3 * w + 3) & ~3
    assert rows_top_down.shape == (h, pitch)
    hdr = bytearray(54)
    hdr[0:2] = b"BM"
    nbytes = pitch * h
    for off, val, size in ((2, nbytes + 54, 4), (10, 54, 4), (14, 40, 4), (18, w, 4), (22, h, 4), (26, 1, 2), (28, 24, 2), (34, nbytes, 4)):
        hdr[off:off + size] = int(val).to_bytes(size, "little")
    return bytes(hdr) + np.ascontiguousarray(rows_top_down[::-1]).tobytes()
