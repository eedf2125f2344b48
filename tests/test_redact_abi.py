"""Redacting the detections in the frames, without a GPU: the spec's layout in the ctypes mirror, the exported symbols, the contract in the header,
tests/redact/redactref.py (the numpy restatement of the contract the GPU tests compare with) against loops that take every pixel against every box
and every cell's mean pixel by pixel, its corner cases, and the device entry points failing the way every entry point of the library does when no
HIP device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from crops import cropref
from overlay import drawref
from redact import redactref

SYMBOLS = ["ffgpu_redact_boxes_bgr_dev", "ffgpu_redact_boxes_nv12_dev", "ffgpu_exec_redact_bgr", "ffgpu_exec_redact_nv12"]
Spec, FILL, MOSAIC = redactref.Spec, redactref.FILL, redactref.MOSAIC


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def boxes_of(rows):
    """rows of (x1, y1, x2, y2[, type[, score]])"""
    b = np.zeros(len(rows), redactref.BOX_DTYPE)
    for k, r in enumerate(rows):
        b[k] = (r[4] if len(r) > 4 else 0, r[5] if len(r) > 5 else 0.5, r[0], r[1], r[2], r[3])
    return b


def test_redact_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_redact_spec_layout(capi):
    S = capi.RedactSpec
    assert C.sizeof(S) == 40
    assert (S.mode.offset, S.cell.offset, S.flags.offset, S.nclasses.offset, S.classes.offset, S.min_score.offset, S.margin_num.offset,
            S.margin_den.offset, S.color.offset) == (0, 4, 8, 12, 16, 24, 28, 32, 36)
    assert (capi.REDACT_FILL, capi.REDACT_MOSAIC, capi.REDACT_OUTSIDE, capi.REDACT_ENTRIES, capi.REDACT_MERGED) == (0, 1, 1, 0, 1)
    assert (redactref.FILL, redactref.MOSAIC) == (capi.REDACT_FILL, capi.REDACT_MOSAIC) and redactref.BOX_DTYPE == capi.BOX_DTYPE
    sp = capi.redact_spec(capi.REDACT_FILL)
    assert (sp.mode, sp.cell, sp.flags, sp.nclasses, sp.classes, sp.min_score, sp.margin_num, sp.margin_den, bytes(sp.color)) == (0, 0, 0, 0, None, 0.0, 0, 1, bytes(4))
    sp = capi.redact_spec(capi.REDACT_MOSAIC, 8, True, 0.25, [0, 1, 1], (1, 4), (1, 2, 3))
    assert (sp.mode, sp.cell, sp.flags, sp.nclasses, sp.min_score, sp.margin_num, sp.margin_den, bytes(sp.color)) == (1, 8, 1, 3, 0.25, 1, 4, bytes([1, 2, 3, 0]))
    assert C.string_at(sp.classes, 3) == bytes([0, 1, 1])


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    assert "} ffgpu_redact_spec;" in hdr
    for name, val in (("FFGPU_REDACT_FILL", 0), ("FFGPU_REDACT_MOSAIC", 1), ("FFGPU_REDACT_OUTSIDE", 1), ("FFGPU_REDACT_ENTRIES", 0), ("FFGPU_REDACT_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    for phrase in ("Covered set S", "anchored at the TARGET's pixel (0, 0)", "m = (sum + n / 2) / n", "ORIGINAL bytes", "Untouched bytes", "exactly one workgroup",
                   "Redact, then draw", "anchors the grid at the TILE", "errs toward redacting"):
        assert phrase in hdr, phrase


def test_redact_without_device(capi):
    """with no HIP device all four entry points say so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_redact_boxes_bgr_dev(None, None, 0, None, None, 1, None, None),
                 lambda: L.ffgpu_redact_boxes_nv12_dev(None, None, 0, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_redact_bgr(None, 0, None, 1, None, None),
                 lambda: L.ffgpu_exec_redact_nv12(None, 0, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


# ---------------------------------------------------------------------------------------------------------------- redactref against literal loops
def literal_covered(x, y, w, h, boxes, spec):
    """is pixel (x, y) of a w x h target in S: every box, one after the other, by the header's sentences"""
    inside = False
    for box in boxes:
        score, t = np.float32(box["score"]), int(box["type"])
        if not (score >= np.float32(spec.min_score)):
            continue
        if spec.classes is not None and not (0 <= t < len(spec.classes) and spec.classes[t]):
            continue
        a, b, c, d = drawref.corners(box)
        if a > c or b > d:
            continue
        mx, my = (c - a + 1) * spec.num // spec.den, (d - b + 1) * spec.num // spec.den
        X0, X1, Y0, Y1 = max(a - mx, 0), min(c + mx, w - 1), max(b - my, 0), min(d + my, h - 1)
        if X0 <= x <= X1 and Y0 <= y <= Y1:
            inside = True
    return inside != spec.outside


def literal_mean(get, x, y, w, h, s):
    """the mean of the cell of side s that holds (x, y) in a w x h plane, get(x, y) one value at a time"""
    i, j = x // s, y // s
    total = n = 0
    for yy in range(j * s, min((j + 1) * s, h)):
        for xx in range(i * s, min((i + 1) * s, w)):
            total += int(get(xx, yy))
            n += 1
    return (total + n // 2) // n


def literal_bgr(start, base, w, h, pitch, boxes, spec):
    out = start.copy()
    for y in range(h):
        for x in range(w):
            if not literal_covered(x, y, w, h, boxes, spec):
                continue
            for c in range(3):
                o = base + y * pitch + 3 * x + c
                out[o] = spec.color[c] if spec.mode == FILL else literal_mean(lambda xx, yy: start[base + yy * pitch + 3 * xx + c], x, y, w, h, spec.cell)
    return out


def literal_nv12(start, base_y, base_uv, w, h, py, puv, boxes, spec):
    out = start.copy()
    for y in range(h):
        for x in range(w):
            if literal_covered(x, y, w, h, boxes, spec):
                out[base_y + y * py + x] = spec.color[0] if spec.mode == FILL else literal_mean(lambda xx, yy: start[base_y + yy * py + xx], x, y, w, h, spec.cell)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    for j in range(ch):
        for i in range(cw):
            if not any(literal_covered(x, y, w, h, boxes, spec) for x in (2 * i, 2 * i + 1) for y in (2 * j, 2 * j + 1) if x < w and y < h):
                continue
            for c in range(2):
                o = base_uv + j * puv + 2 * i + c
                out[o] = spec.color[1 + c] if spec.mode == FILL else literal_mean(lambda xx, yy: start[base_uv + yy * puv + 2 * xx + c], i, j, cw, ch, spec.cell // 2)
    return out


def test_redactref_is_the_literal_loops():
    """small targets with pitch padding and guard bytes, boxes around and across them (inverted ones too), both modes, with and without OUTSIDE,
    cells 2, 3, 4 and 64 (NV12: 2, 4, 64), class tables and score thresholds"""
    rng = np.random.default_rng(522)
    seen = set()
    for case in range(104):
        w, h = int(rng.integers(1, 15)), int(rng.integers(1, 13))
        n = int(rng.integers(0, 6))
        boxes = boxes_of([tuple(rng.uniform(-6, 18, 4)) + (int(rng.integers(-2, 5)), float(rng.uniform(0, 1))) for _ in range(n)])
        mode, outside = (FILL, MOSAIC)[case & 1], bool(case & 2)
        cell = (2, 3, 4, 64)[(case >> 2) & 3] if mode == MOSAIC else 0
        classes = None if rng.random() < 0.5 else [int(v) for v in rng.integers(0, 2, 4)]
        margin = ((0, 1), (1, 3), (4, 1))[int(rng.integers(0, 3))]
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        spec = Spec(mode, cell, outside, float(rng.uniform(0, 0.6)), classes, margin, color)
        seen.add((mode, outside, cell))
        pitch = 3 * w + int(rng.integers(0, 5))
        start = rng.integers(0, 256, 7 + pitch * h + 9).astype(np.uint8)
        got = redactref.redact_bgr(start.copy(), 7, w, h, pitch, boxes, spec)
        assert got.tobytes() == literal_bgr(start, 7, w, h, pitch, boxes, spec).tobytes(), case
        if cell & 1:
            spec = Spec(mode, cell + 1, outside, spec.min_score, classes, margin, color)
        py, puv = w + int(rng.integers(0, 3)), 2 * ((w + 1) // 2) + 2 * int(rng.integers(0, 3))
        base_uv = 5 + py * h + int(rng.integers(0, 4))
        start = rng.integers(0, 256, base_uv + puv * ((h + 1) // 2) + 9).astype(np.uint8)
        got = redactref.redact_nv12(start.copy(), 5, base_uv, w, h, py, puv, boxes, spec)
        assert got.tobytes() == literal_nv12(start, 5, base_uv, w, h, py, puv, boxes, spec).tobytes(), case
    assert len(seen) == 2 * (1 + 4)


def covered_set(w, h, rows, stats=None, **kw):
    S = redactref.covered(w, h, boxes_of(rows), Spec(FILL, **kw), stats)
    ys, xs = np.nonzero(S)
    return set(zip(xs.tolist(), ys.tolist()))


def rect(x0, y0, x1, y1):
    return {(x, y) for x in range(x0, x1 + 1) for y in range(y0, y1 + 1)}


def test_redactref_properties():
    nan, big = float("nan"), 1e30
    # the region of a box is its truncated corners, inclusive; NaN corners are 0; +-1e30 saturates and is clipped to the target
    assert covered_set(12, 10, [(2.9, 1.2, 5.1, 3.99)]) == rect(2, 1, 5, 3)
    assert covered_set(12, 10, [(nan, nan, 4.5, 2.5)]) == rect(0, 0, 4, 2)
    assert covered_set(12, 10, [(-big, 4, big, big)]) == rect(0, 4, 11, 9)
    assert covered_set(12, 10, [(big, big, big, big)]) == set()
    # inverted either way: nothing (the draw contract would still outline it); a box wholly outside: nothing; both count as empty
    stats = {}
    assert covered_set(12, 10, [(8, 2, 3, 5), (3, 7, 8, 2), (20, 20, 30, 30), (-9, -9, -1, -1)], stats) == set()
    assert (stats["qualifying"], stats["empty"], stats["covered"], stats["pixels"]) == (4, 4, 0, 120)
    # a NaN score never qualifies, a NaN min_score lets nothing qualify; a negative class against a table is not allowed
    stats = {}
    assert covered_set(12, 10, [(1, 1, 2, 2, 0, nan), (4, 4, 5, 5, 0, 0.0)], stats) == rect(4, 4, 5, 5) and stats["rejected_score"] == 1
    assert covered_set(12, 10, [(1, 1, 2, 2, 0, 0.9)], min_score=nan) == set()
    stats = {}
    assert covered_set(12, 10, [(1, 1, 2, 2, -1), (4, 4, 5, 5, 1), (7, 7, 8, 8, 0), (9, 1, 9, 1, 2)], stats, classes=[0, 1]) == rect(4, 4, 5, 5)
    assert stats["rejected_class"] == 3
    # margins: 0 is the box, 4 / 1 grows it by four times its size each way, clipped
    assert covered_set(40, 30, [(20, 10, 21, 12)], margin=(0, 1)) == rect(20, 10, 21, 12)
    assert covered_set(40, 30, [(20, 10, 21, 12)], margin=(4, 1)) == rect(12, 0, 29, 24)
    assert covered_set(40, 30, [(20, 10, 21, 12)], margin=(1, 3)) == rect(20, 9, 21, 13)
    # OUTSIDE: the complement inside w x h; an empty list then covers the whole target
    assert covered_set(12, 10, [(2, 1, 5, 3)], outside=True) == rect(0, 0, 11, 9) - rect(2, 1, 5, 3)
    assert covered_set(12, 10, [], outside=True) == rect(0, 0, 11, 9) and covered_set(12, 10, []) == set()
    # overlapping boxes: the union, in either order
    rng = np.random.default_rng(523)
    start = rng.integers(0, 256, 36 * 10).astype(np.uint8)
    two = [(1, 1, 6, 6), (4, 4, 9, 8)]
    for spec in (Spec(FILL, color=(9, 8, 7)), Spec(MOSAIC, 4), Spec(MOSAIC, 3, outside=True)):
        a = redactref.redact_bgr(start.copy(), 0, 12, 10, 36, boxes_of(two), spec)
        b = redactref.redact_bgr(start.copy(), 0, 12, 10, 36, boxes_of(two[::-1]), spec)
        assert a.tobytes() == b.tobytes() != start.tobytes()
    assert covered_set(12, 10, two) == rect(1, 1, 6, 6) | rect(4, 4, 9, 8)
    # MOSAIC of a constant frame leaves it unchanged; of any frame: a covered pixel holds its cell's rounded mean over ALL the cell's pixels
    const = np.full(36 * 10, 77, np.uint8)
    assert redactref.redact_bgr(const.copy(), 0, 12, 10, 36, boxes_of(two), Spec(MOSAIC, 5)).tobytes() == const.tobytes()
    nv = np.full(12 * 10 + 12 * 5, 200, np.uint8)
    assert redactref.redact_nv12(nv.copy(), 0, 120, 12, 10, 12, 12, boxes_of(two), Spec(MOSAIC, 4, outside=True)).tobytes() == nv.tobytes()
    img = np.arange(8 * 4 * 3, dtype=np.uint8)
    out = redactref.redact_bgr(img.copy(), 0, 8, 4, 24, boxes_of([(1, 1, 1, 1)]), Spec(MOSAIC, 4)).reshape(4, 8, 3)
    cellmean = (int(img.reshape(4, 8, 3)[:4, :4, 0].sum()) + 8) // 16
    assert out[1, 1, 0] == cellmean and np.count_nonzero(out != img.reshape(4, 8, 3)) == 3
    # the cells' statistics on 3 x 3 cells (the last column 2 wide, the last row 1 high): cell (0, 0) and the clipped cell (2, 2) fully covered, three
    # neighbours of the first and cell (2, 1) partly; (2, 1) and (2, 2) are cut by the right edge, (2, 2) by the bottom edge
    stats = {}
    redactref.redact_bgr(np.zeros(30 * 9, np.uint8), 0, 10, 9, 30, boxes_of([(0, 0, 5, 5), (8, 7, 9, 8)]), Spec(MOSAIC, 4), stats)
    assert (stats["cells_full"], stats["cells_partial"], stats["cells_cut_right"], stats["cells_cut_bottom"]) == (2, 4, 2, 1)
    # NV12 FILL: a single luma pixel takes its whole chroma sample with it (mixed coverage), odd sizes have half-empty samples at the edges
    stats = {}
    nv = redactref.redact_nv12(np.zeros(7 * 5 + 8 * 3, np.uint8), 0, 35, 7, 5, 7, 8, boxes_of([(3, 3, 3, 3), (6, 4, 6, 4)]), Spec(FILL, color=(10, 20, 30)), stats)
    assert np.count_nonzero(nv[:35]) == 2 and nv[3 * 7 + 3] == 10 and nv[4 * 7 + 6] == 10
    assert tuple(nv[35 + 8 + 2:35 + 8 + 4]) == (20, 30) and tuple(nv[35 + 16 + 6:35 + 16 + 8]) == (20, 30) and np.count_nonzero(nv[35:]) == 4
    assert stats["chroma_mixed"] == 1
    assert cropref.corners(boxes_of([(1.5, 2.5, 3.5, 4.5)])[0]) == drawref.corners(boxes_of([(1.5, 2.5, 3.5, 4.5)])[0])


def test_fuzz_seeds_meet_the_conditions_on_the_reference_alone():
    """the seeded cases of the GPU fuzz (tests/redact/fuzzcases.py) through redactref on zero frames, no device: every parametrisation has its partly
    covered cells, cut cells, mixed chroma samples, empty and rejected boxes, and more than a quarter of the pixels on either side"""
    from redact import fuzzcases
    for nv12 in (False, True):
        for mode in (FILL, MOSAIC):
            for outside in (False, True):
                total, lengths = {}, set()
                for cell, specs, lists, sp in fuzzcases.fuzz_cases(nv12, mode, outside):
                    assert sp.cell == (cell if mode == MOSAIC else 0)
                    lengths |= {len(b) for b in lists}
                    for s, b in zip(specs, lists):
                        if nv12:
                            redactref.redact_nv12(np.zeros(s[2] * s[1] + s[3] * ((s[1] + 1) // 2), np.uint8), 0, s[2] * s[1], s[0], s[1], s[2], s[3], b, sp, total)
                        else:
                            redactref.redact_bgr(np.zeros(s[2] * s[1], np.uint8), 0, s[0], s[1], s[2], b, sp, total)
                print(nv12, mode, outside, total)
                assert {0, 7} <= lengths <= set(range(8)), lengths
                fuzzcases.check_stats(total, nv12, mode)
