"""Drawing the detections into the frames, without a GPU: the style structure's layout in the ctypes mirror, the exported symbols, the contract in
the header, tests/overlay/drawref.py (the numpy restatement of the contract the GPU tests compare with) pinned to the reference program's own
out.bmp, its corner cases, and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLD, ROOT
from overlay import drawref

SYMBOLS = ["ffgpu_draw_boxes_bgr_dev", "ffgpu_draw_boxes_nv12_dev", "ffgpu_exec_draw_bgr", "ffgpu_exec_draw_nv12"]


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def boxes_of(rows):
    b = np.zeros(len(rows), drawref.BOX_DTYPE)
    for k, r in enumerate(rows):
        b[k] = (r[4] if len(r) > 4 else 0, 0.5, r[0], r[1], r[2], r[3])
    return b


def test_draw_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_draw_style_layout(capi):
    S = capi.DrawStyle
    assert C.sizeof(S) == 24
    assert (S.color.offset, S.palette.offset, S.npalette.offset, S.thickness.offset) == (0, 8, 16, 20)
    assert drawref.BOX_DTYPE == capi.BOX_DTYPE and (capi.DRAW_ENTRIES, capi.DRAW_MERGED) == (0, 1)
    st = capi.draw_style()
    assert (bytes(st.color), st.palette, st.npalette, st.thickness) == (b"\x00\xff\x00\x00", None, 0, 1)
    st = capi.draw_style(palette=[(1, 2, 3), (4, 5, 6)], thickness=3)
    assert (st.npalette, st.thickness) == (2, 3) and C.string_at(st.palette, 8) == bytes([1, 2, 3, 0, 4, 5, 6, 0])


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    assert "} ffgpu_draw_style;" in hdr and "serially in list order" in hdr
    assert int(re.search(r"#define FFGPU_DRAW_MERGED\s+(\d+)", hdr).group(1)) == 1
    assert int(re.search(r"#define FFGPU_DRAW_ENTRIES\s+(\d+)", hdr).group(1)) == 0


def test_drawref_is_the_reference_programs_out_bmp(capi):
    """the three rectangles the reference program printed for data/test.bmp (tests/golden/cli.json), green, thickness 1, drawn by drawref and
    written with the demo's 54-byte header: the SHA-256 of the reference's own out.bmp"""
    cli = json.load(open(os.path.join(GOLD, "cli.json")))
    rects = [tuple(int(v) for v in re.search(r"rect: \(\s*(-?\d+)\s+(-?\d+)\s+(-?\d+)\s+(-?\d+)\)", line).groups()) for line in cli["detections"]]
    assert len(rects) == 3
    rows, w, h = capi.load_bmp(os.path.join(capi.DATA, "test.bmp"))
    assert (w, h, rows.shape) == (640, 424, (424, 1920))
    buf = rows.reshape(-1).copy()
    boxes = boxes_of(rects)
    stats = {}
    drawref.draw_bgr(buf, 0, w, h, 1920, boxes, drawref.colours_of(boxes, (0, 255, 0)), 1, stats)
    assert stats["boxes"] == stats["inside"] == 3
    assert hashlib.sha256(drawref.bmp_file(buf.reshape(h, 1920), w, h)).hexdigest() == cli["out_bmp_sha256"]


def literal_bgr(buf, base, w, h, pitch, boxes, colours, thickness):
    """bmp_setpixel + bmp_rectangle word for word (only for boxes whose corners are small)"""
    for box, c in zip(boxes, colours):
        a, b, cc, d = drawref.corners(box)

        def put(x, y):
            if x < 0 or x >= w or y < 0 or y >= h:
                return
            buf[base + 3 * x + y * pitch:base + 3 * x + y * pitch + 3] = c
        for i in range(thickness):
            drawref.rectangle_literal(put, a + i, b + i, cc - i, d - i)
    return buf


def literal_nv12(buf, base_y, base_uv, w, h, pitch_y, pitch_uv, boxes, colours, thickness):
    for box, c in zip(boxes, colours):
        a, b, cc, d = drawref.corners(box)

        def put(x, y):
            if x < 0 or x >= w or y < 0 or y >= h:
                return
            buf[base_y + y * pitch_y + x] = c[0]
            o = base_uv + (y >> 1) * pitch_uv + 2 * (x >> 1)
            buf[o:o + 2] = c[1:]
        for i in range(thickness):
            drawref.rectangle_literal(put, a + i, b + i, cc - i, d - i)
    return buf


def test_drawref_slices_are_the_literal_loops():
    """the clipped, sliced form against the literal loops: small targets, boxes around and across them (inverted ones too), every thickness"""
    rng = np.random.default_rng(517)
    pal = rng.integers(0, 256, (5, 3))
    for case in range(120):
        w, h = int(rng.integers(1, 14)), int(rng.integers(1, 12))
        n, T = int(rng.integers(0, 7)), int(rng.integers(1, 9))
        boxes = boxes_of([tuple(rng.uniform(-6, 18, 4)) + (int(rng.integers(-9, 9)),) for _ in range(n)])
        cols = drawref.colours_of(boxes, palette=pal)
        pitch = 3 * w + int(rng.integers(0, 5))
        start = rng.integers(0, 256, 7 + pitch * h + 9).astype(np.uint8)
        got = drawref.draw_bgr(start.copy(), 7, w, h, pitch, boxes, cols, T)
        assert got.tobytes() == literal_bgr(start.copy(), 7, w, h, pitch, boxes, cols, T).tobytes(), case
        py, puv = w + int(rng.integers(0, 3)), 2 * ((w + 1) // 2) + 2 * int(rng.integers(0, 3))
        base_uv = 5 + py * h + int(rng.integers(0, 4))
        start = rng.integers(0, 256, base_uv + puv * ((h + 1) // 2) + 9).astype(np.uint8)
        got = drawref.draw_nv12(start.copy(), 5, base_uv, w, h, py, puv, boxes, cols, T)
        assert got.tobytes() == literal_nv12(start.copy(), 5, base_uv, w, h, py, puv, boxes, cols, T).tobytes(), case


def drawn_pixels(w, h, rows, T=1, stats=None):
    """the set of pixels a list draws on a black w x h target in white"""
    boxes = boxes_of(rows)
    buf = drawref.draw_bgr(np.zeros(3 * w * h, np.uint8), 0, w, h, 3 * w, boxes, [(255, 255, 255)] * len(boxes), T, stats)
    ys, xs = np.nonzero(buf.reshape(h, w, 3)[:, :, 0])
    return set(zip(xs.tolist(), ys.tolist()))


def test_drawref_properties():
    nan, big = float("nan"), 1e30
    # an inverted box (a > c, b <= d): the two columns and nothing else
    assert drawn_pixels(12, 10, [(8, 2, 3, 5)]) == {(x, y) for x in (8, 3) for y in range(2, 6)}
    # inverted the other way (b > d): the two rows; both ways: nothing
    assert drawn_pixels(12, 10, [(3, 7, 8, 2)]) == {(x, y) for y in (7, 2) for x in range(3, 9)}
    assert drawn_pixels(12, 10, [(8, 7, 3, 2)]) == set()
    # a NaN corner is 0
    assert drawref.corners(boxes_of([(nan, nan, 4.9, -0.9)])[0]) == (0, 0, 4, 0)
    assert drawn_pixels(12, 10, [(nan, 3, 5, nan)]) == drawn_pixels(12, 10, [(0, 3, 5, 0)])
    # +-1e30 saturates and draws only what is inside: here the row y = 4 and nothing of the three edges outside
    assert drawref.corners(boxes_of([(-big, 4, big, big)])[0]) == (drawref.INT_MIN, 4, drawref.INT_MAX, drawref.INT_MAX)
    stats = {}
    assert drawn_pixels(12, 10, [(-big, 4, big, big)], 1, stats) == {(x, 4) for x in range(12)}
    assert drawn_pixels(12, 10, [(-big, -big, big, big)], 8, stats) == set()
    assert (stats["clipped"], stats["outside"]) == (1, 1)
    # thickness: T rectangles, each one pixel further in; a zero-size box is one pixel, then inverted rectangles that draw nothing
    assert drawn_pixels(12, 10, [(2, 1, 9, 8)], 2) == drawn_pixels(12, 10, [(2, 1, 9, 8), (3, 2, 8, 7)])
    assert drawn_pixels(12, 10, [(5, 5, 5, 5)], 8) == {(5, 5)}
    # the palette index of a negative class is the non-negative remainder
    pal = [(1, 1, 1), (2, 2, 2), (3, 3, 3)]
    assert drawref.colours_of(boxes_of([(0, 0, 1, 1, -1), (0, 0, 1, 1, -3), (0, 0, 1, 1, 4), (0, 0, 1, 1, -2 ** 31)]), palette=pal) == [pal[2], pal[0], pal[1], pal[(-2 ** 31) % 3]]
    # a later box overwrites an earlier one, and the statistics see it
    stats = {}
    b = boxes_of([(1, 1, 6, 6, 0), (4, 4, 9, 8, 1)])
    buf = drawref.draw_bgr(np.zeros(3 * 12 * 10, np.uint8), 0, 12, 10, 36, b, drawref.colours_of(b, palette=pal), 1, stats).reshape(10, 12, 3)
    assert tuple(buf[4, 6]) == pal[1] and tuple(buf[6, 4]) == pal[1] and tuple(buf[1, 1]) == pal[0]
    assert stats["overwritten"] == 2 and stats["inside"] == 2
    # NV12: two boxes of different colours share chroma sample (1, 1) through different luma pixels: the later box's U V, each box's own Y
    b = boxes_of([(2, 2, 2, 2, 0), (3, 3, 3, 3, 1)])
    nv = drawref.draw_nv12(np.zeros(8 * 6 + 8 * 3, np.uint8), 0, 48, 8, 6, 8, 8, b, [(10, 20, 30), (40, 50, 60)], 1)
    assert nv[2 * 8 + 2] == 10 and nv[3 * 8 + 3] == 40 and tuple(nv[48 + 8 + 2:48 + 8 + 4]) == (50, 60)


def test_draw_without_device(capi):
    """with no HIP device all four entry points say so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_draw_boxes_bgr_dev(None, None, 0, None, None, 1, None, None),
                 lambda: L.ffgpu_draw_boxes_nv12_dev(None, None, 0, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_draw_bgr(None, 0, None, 1, None, None),
                 lambda: L.ffgpu_exec_draw_nv12(None, 0, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs
