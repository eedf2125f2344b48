"""Blurring the detections in the frames, without a GPU: the spec's layout in the ctypes mirror, the exported symbols, the contract in the header,
tests/blur/blurref.py (the numpy restatement of the contract the GPU tests compare with) against loops that visit every pixel, every pixel of its
window and every box, p passes against p calls of one pass, the conditions that keep the GPU fuzz from passing vacuously on the reference alone,
and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from blur import blurref, fuzzcases
from conftest import ROOT
from overlay import drawref

SYMBOLS = ["ffgpu_blur_boxes_bgr_dev", "ffgpu_blur_boxes_nv12_dev", "ffgpu_exec_blur_bgr", "ffgpu_exec_blur_nv12"]
Spec = blurref.Spec


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def boxes_of(rows):
    """rows of (x1, y1, x2, y2[, type[, score]])"""
    b = np.zeros(len(rows), blurref.BOX_DTYPE)
    for k, r in enumerate(rows):
        b[k] = (r[4] if len(r) > 4 else 0, r[5] if len(r) > 5 else 0.5, r[0], r[1], r[2], r[3])
    return b


def test_blur_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_blur_spec_layout(capi):
    S = capi.BlurSpec
    assert C.sizeof(S) == 40
    assert (S.radius.offset, S.passes.offset, S.flags.offset, S.nclasses.offset, S.classes.offset, S.min_score.offset, S.margin_num.offset,
            S.margin_den.offset, S.reserved.offset) == (0, 4, 8, 12, 16, 24, 28, 32, 36)
    assert (capi.BLUR_OUTSIDE, capi.BLUR_ENTRIES, capi.BLUR_MERGED) == (1, 0, 1) and blurref.BOX_DTYPE == capi.BOX_DTYPE
    sp = capi.blur_spec(5)
    assert (sp.radius, sp.passes, sp.flags, sp.nclasses, sp.classes, sp.min_score, sp.margin_num, sp.margin_den, sp.reserved) == (5, 1, 0, 0, None, 0.0, 0, 1, 0)
    sp = capi.blur_spec(31, 3, True, 0.25, [0, 1, 1], (1, 4))
    assert (sp.radius, sp.passes, sp.flags, sp.nclasses, sp.min_score, sp.margin_num, sp.margin_den, sp.reserved) == (31, 3, 1, 3, 0.25, 1, 4, 0)
    assert C.string_at(sp.classes, 3) == bytes([0, 1, 1])


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    assert "} ffgpu_blur_spec;" in hdr
    for name, val in (("FFGPU_BLUR_OUTSIDE", 1), ("FFGPU_BLUR_ENTRIES", 0), ("FFGPU_BLUR_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    for phrase in ("the redact contract's, word for word", "(sum of O over W + n / 2) / n", "clipped to the target's w x h, not padded", "blur mixes, it does not mask",
                   "Every byte outside\n * S stays", "rc = (r + 1) / 2", "No evenness is required of r", "NULL exactly where the target is NULL",
                   "with both indices in the message", "every other scratch byte is unchanged", "stream order between the two is the barrier",
                   "Blur, then draw, outline and caption", "FFGPU_BLUR_MERGED on the whole picture"):
        assert phrase in hdr, phrase


def test_blur_without_device(capi):
    """with no HIP device all four entry points say so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_blur_boxes_bgr_dev(None, None, 0, None, None, None, 1, None, None),
                 lambda: L.ffgpu_blur_boxes_nv12_dev(None, None, 0, None, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_blur_bgr(None, 0, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_blur_nv12(None, 0, None, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


# ---------------------------------------------------------------------------------------------------------------- blurref against literal loops
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


def literal_mean(get, x, y, w, h, r):
    """the rounded mean over the clipped window of (x, y) in a w x h plane, get(x, y) one value at a time"""
    total = n = 0
    for yy in range(max(y - r, 0), min(y + r, h - 1) + 1):
        for xx in range(max(x - r, 0), min(x + r, w - 1) + 1):
            total += int(get(xx, yy))
            n += 1
    return (total + n // 2) // n


def literal_bgr(start, base, sbase, w, h, pitch, spitch, boxes, spec):
    out = start.copy()
    for _ in range(spec.passes):
        old = out.copy()
        for y in range(h):
            for x in range(w):
                if not literal_covered(x, y, w, h, boxes, spec):
                    continue
                for c in range(3):
                    m = literal_mean(lambda xx, yy: old[base + yy * pitch + 3 * xx + c], x, y, w, h, spec.radius)
                    out[base + y * pitch + 3 * x + c] = out[sbase + y * spitch + 3 * x + c] = m
    return out


def literal_nv12(start, base_y, base_uv, sbase_y, sbase_uv, w, h, py, puv, spy, spuv, boxes, spec):
    out = start.copy()
    cw, ch, rc = (w + 1) // 2, (h + 1) // 2, (spec.radius + 1) // 2
    for _ in range(spec.passes):
        old = out.copy()
        for y in range(h):
            for x in range(w):
                if literal_covered(x, y, w, h, boxes, spec):
                    out[base_y + y * py + x] = out[sbase_y + y * spy + x] = literal_mean(lambda xx, yy: old[base_y + yy * py + xx], x, y, w, h, spec.radius)
        for j in range(ch):
            for i in range(cw):
                if not any(literal_covered(x, y, w, h, boxes, spec) for x in (2 * i, 2 * i + 1) for y in (2 * j, 2 * j + 1) if x < w and y < h):
                    continue
                for c in range(2):
                    m = literal_mean(lambda xx, yy: old[base_uv + yy * puv + 2 * xx + c], i, j, cw, ch, rc)
                    out[base_uv + j * puv + 2 * i + c] = out[sbase_uv + j * spuv + 2 * i + c] = m
    return out


def small_case(rng, case, w, h):
    n = int(rng.integers(0, 5))
    boxes = boxes_of([tuple(rng.uniform(-6, 24, 4)) + (int(rng.integers(-2, 5)), float(rng.uniform(0, 1))) for _ in range(n)])
    classes = None if rng.random() < 0.5 else [int(v) for v in rng.integers(0, 2, 4)]
    margin = ((0, 1), (1, 3), (4, 1))[int(rng.integers(0, 3))]
    radius = (1, 2, 3, 7, 16, 31)[case % 6]
    return boxes, Spec(radius, 1 + (case // 6) % 3, bool((case // 3 + case // 18) & 1), float(rng.uniform(0, 0.6)), classes, margin)


def test_blurref_is_the_literal_loops():
    """small targets (up to 20 x 17) with pitch padding and guard bytes, a scratch surface of another pitch, boxes around and across them (inverted
    ones too), with and without OUTSIDE, radii from 1 to 31 (windows inside the target, clipped, and larger than it), 1 to 3 passes"""
    rng = np.random.default_rng(540)
    seen = set()
    for case in range(36):
        w, h = (20, 17) if case == 5 else (int(rng.integers(1, 15)), int(rng.integers(1, 12)))
        boxes, spec = small_case(rng, case, w, h)
        seen.add((spec.radius, spec.passes, spec.outside))
        pitch, spitch = 3 * w + int(rng.integers(0, 5)), 3 * w + int(rng.integers(0, 7))
        sbase = 7 + pitch * h + 3
        start = rng.integers(0, 256, sbase + spitch * h + 9).astype(np.uint8)
        got = blurref.blur_bgr(start.copy(), 7, sbase, w, h, pitch, spitch, boxes, spec)
        assert got.tobytes() == literal_bgr(start, 7, sbase, w, h, pitch, spitch, boxes, spec).tobytes(), case
        py, puv = w + int(rng.integers(0, 3)), 2 * ((w + 1) // 2) + 2 * int(rng.integers(0, 3))
        spy, spuv = w + int(rng.integers(0, 4)), 2 * ((w + 1) // 2) + 2 * int(rng.integers(0, 2))
        base_uv = 5 + py * h + int(rng.integers(0, 4))
        sbase_y = base_uv + puv * ((h + 1) // 2) + 3
        sbase_uv = sbase_y + spy * h + 1
        start = rng.integers(0, 256, sbase_uv + spuv * ((h + 1) // 2) + 9).astype(np.uint8)
        got = blurref.blur_nv12(start.copy(), 5, base_uv, sbase_y, sbase_uv, w, h, py, puv, spy, spuv, boxes, spec)
        assert got.tobytes() == literal_nv12(start, 5, base_uv, sbase_y, sbase_uv, w, h, py, puv, spy, spuv, boxes, spec).tobytes(), case
    assert len(seen) == 36 and {s[0] for s in seen} == {1, 2, 3, 7, 16, 31} and {s[1] for s in seen} == {1, 2, 3}


def test_blurref_passes_are_repeated_calls():
    """passes = p is p calls with passes = 1 on the same surfaces: the target AND the scratch end up the same"""
    rng = np.random.default_rng(541)
    for case in range(12):
        w, h = int(rng.integers(3, 90)), int(rng.integers(3, 80))
        boxes = boxes_of([tuple(rng.uniform(-6, 90, 4)) + (0, 0.9) for _ in range(3)] + [(1, 1, w // 2, h - 2)])
        p, r, outside = 2 + case % 2, (1, 4, 16, 31)[case % 4], bool(case & 4)
        pitch, spitch = 3 * w + 2, 3 * w + 5
        sbase = 7 + pitch * h
        start = rng.integers(0, 256, sbase + spitch * h + 9).astype(np.uint8)
        once = blurref.blur_bgr(start.copy(), 7, sbase, w, h, pitch, spitch, boxes, Spec(r, p, outside))
        step = start.copy()
        for _ in range(p):
            blurref.blur_bgr(step, 7, sbase, w, h, pitch, spitch, boxes, Spec(r, 1, outside))
        assert once.tobytes() == step.tobytes() != start.tobytes(), case
        py, puv, spy, spuv = w + 1, 2 * ((w + 1) // 2) + 2, w, 2 * ((w + 1) // 2)
        base_uv, sbase_y = 4 + py * h, 4 + py * h + puv * ((h + 1) // 2) + 3
        sbase_uv = sbase_y + spy * h
        start = rng.integers(0, 256, sbase_uv + spuv * ((h + 1) // 2) + 9).astype(np.uint8)
        once = blurref.blur_nv12(start.copy(), 4, base_uv, sbase_y, sbase_uv, w, h, py, puv, spy, spuv, boxes, Spec(r, p, outside))
        step = start.copy()
        for _ in range(p):
            blurref.blur_nv12(step, 4, base_uv, sbase_y, sbase_uv, w, h, py, puv, spy, spuv, boxes, Spec(r, 1, outside))
        assert once.tobytes() == step.tobytes() != start.tobytes(), case


def test_blurref_properties():
    # a constant frame stays what it is, whatever the radius and the clipping; the scratch receives the same constant at the positions of S only
    buf = np.concatenate([np.full(36 * 10, 77, np.uint8), np.full(40 * 10, 1, np.uint8)])
    out = blurref.blur_bgr(buf.copy(), 0, 360, 12, 10, 36, 40, boxes_of([(2, 1, 5, 3)]), Spec(31, 3))
    assert out[:360].tobytes() == buf[:360].tobytes()
    sc = out[360:].reshape(10, 40)
    assert np.all(sc[1:4, 6:18] == 77) and np.count_nonzero(sc == 77) == 3 * 12
    # one bright pixel, r = 1: the covered pixels around it take 255 / n rounded, n = 9 inside, 6 at an edge, 4 in a corner; the uncovered stay
    img = np.zeros((5, 6, 3), np.uint8)
    img[0, 0] = 255
    buf = np.concatenate([img.reshape(-1), np.zeros(90, np.uint8)])
    out = blurref.blur_bgr(buf.copy(), 0, 90, 6, 5, 18, 18, boxes_of([(0, 0, 1, 4)]), Spec(1))[:90].reshape(5, 6, 3)
    assert out[0, 0, 0] == (255 + 2) // 4 and out[0, 1, 0] == (255 + 3) // 6 and out[1, 1, 0] == (255 + 4) // 9 and out[1, 0, 0] == (255 + 3) // 6
    assert out[2, 0, 0] == 0 and np.all(out[:, 2:] == 0)
    # blur mixes, it does not mask: a covered pixel next to an uncovered bright one takes part of it
    img = np.zeros((3, 8, 3), np.uint8)
    img[:, 4:] = 200
    buf = np.concatenate([img.reshape(-1), np.zeros(72, np.uint8)])
    out = blurref.blur_bgr(buf.copy(), 0, 72, 8, 3, 24, 24, boxes_of([(0, 0, 3, 2)]), Spec(1))[:72].reshape(3, 8, 3)
    assert out[1, 3, 0] == (200 * 3 + 4) // 9 and out[0, 3, 0] == (200 * 2 + 3) // 6 and np.all(out[:, 4:] == 200) and np.all(out[:, :3] == 0)
    # NV12: chroma uses (r + 1) / 2 on the half-size plane and is written where the FILL rule says, a single luma pixel taking its sample with it
    w, h = 7, 5
    Y, UV = np.zeros((h, w), np.uint8), np.zeros((3, 4, 2), np.uint8)
    UV[1, 1] = (90, 180)
    buf = np.concatenate([Y.reshape(-1), UV.reshape(-1), np.zeros(35 + 24, np.uint8)])
    stats = {}
    out = blurref.blur_nv12(buf.copy(), 0, 35, 59, 94, w, h, 7, 8, 7, 8, boxes_of([(3, 3, 3, 3)]), Spec(2), stats)
    uv = out[35:59].reshape(3, 4, 2)
    assert tuple(uv[1, 1]) == ((90 + 4) // 9, (180 + 4) // 9) and np.count_nonzero(uv) == 2 and stats["chroma_mixed"] == 1
    assert tuple(out[94:118].reshape(3, 4, 2)[1, 1]) == tuple(uv[1, 1])
    # the statistics of the windows: 150 x 140, r = 31: all three pixels' windows are clipped; (80, 10) reaches columns 49 .. 111 (two blocks), (0, 0)
    # stays in its block, (140, 100) reaches columns 109 .. 149 and rows 69 .. 131 (four blocks); r = 31 on 5 x 4 is larger than the whole target
    stats = {}
    blurref.blur_bgr(np.zeros(2 * 450 * 140, np.uint8), 0, 450 * 140, 150, 140, 450, 450, boxes_of([(80, 10, 80, 10), (0, 0, 0, 0), (140, 100, 140, 100)]), Spec(31), stats)
    assert (stats["covered"], stats["win_clipped"], stats["win_neighbour"], stats["win_three_blocks"], stats["win_whole"]) == (3, 3, 2, 1, 0)
    stats = {}
    blurref.blur_bgr(np.zeros(2 * 15 * 4, np.uint8), 0, 60, 5, 4, 15, 15, boxes_of([(0, 0, 4, 3)]), Spec(31), stats)
    assert (stats["covered"], stats["win_clipped"], stats["win_whole"]) == (20, 20, 20)


def host_stats(nv12, outside, seed=None):
    """one parametrisation's cases through blurref on a host array, no device: (cases, one statistics dict per target)"""
    cases = fuzzcases.fuzz_cases(nv12, outside, seed)
    per_target = []
    for c in cases:
        size, offs = fuzzcases.host_layout(nv12, c["specs"] + c["sspecs"])
        n = len(c["specs"])
        buf = np.random.default_rng(7).integers(0, 256, size, dtype=np.uint8)
        for s, o, img in zip(c["specs"], offs[:n], c["images"]):
            fuzzcases.write_image(buf, nv12, s, o, img)
        fuzzcases.reference(buf, nv12, c["specs"], c["sspecs"], offs[:n], offs[n:], c["lists"], c["spec"], per_target)
    return cases, per_target


def test_fuzz_seeds_meet_the_conditions_on_the_reference_alone():
    """the seeded cases of the GPU fuzz (tests/blur/fuzzcases.py) through blurref, no device: every parametrisation has every radius and pass count,
    covered pixels with clipped windows, windows into neighbouring blocks, across three blocks and larger than the target, enough non-empty S and
    results that differ from the input"""
    for nv12 in (False, True):
        for outside in (False, True):
            cases, per_target = host_stats(nv12, outside)
            lengths = {len(b) for c in cases for b in c["lists"]}
            assert {0, 7} <= lengths <= set(range(8)), lengths
            assert all(c["spec"].radius == c["radius"] and c["spec"].passes == c["passes"] and c["spec"].outside == outside for c in cases)
            fuzzcases.check_stats(cases, per_target, outside)
