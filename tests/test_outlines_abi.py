"""Outlines, without a GPU: the exported symbols, the layout of the item and spec structs in the ctypes mirror and the constants in the header, the
host glue under ASan + UBSan (san/lines_driver.cc, run as a child process: every rejection with its message), tests/outlines/lineref.py (the numpy
restatement of the contract the GPU tests compare with) pinned three ways -- to a per-pixel evaluation of the contract's inequality over the whole
surface, to the literal column loop with Python's floor division, and to the stated properties -- and on the named cases, the composer's slot layout,
ticks, alarm switch, SEEN rule and marker cut, the seeded cases of the GPU fuzz held to the conditions that keep it from passing vacuously, and the
device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from outlines import fuzzcases, lineref
from zones import zoneref

SYMBOLS = ["ffgpu_draw_segments_bgr_dev", "ffgpu_draw_segments_nv12_dev", "ffgpu_outline_spec_check", "ffgpu_outline_scene_dev"]
NAN, INF = float("nan"), float("inf")
ITEM = lineref.ITEM_DTYPE
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
LIMIT, IMIN, IMAX = 1 << 20, -2 ** 31, 2 ** 31 - 1
seg = fuzzcases.seg


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module", autouse=True)
def feature(capi):
    """every test of this file is a test of the feature, those that pin lineref and the fuzz's seeds too: a reference is worth what the library it restates
    carries, so each of them needs the built library to export the family and its item layout to be lineref's"""
    missing = [s for s in SYMBOLS if s not in capi.EXPORTS or not hasattr(capi.lib(), s)]
    assert not missing, "libffcnn_hip.so lacks %s" % missing
    assert capi.SEG_ITEM_DTYPE == ITEM and C.sizeof(capi.SegItem) == ITEM.itemsize


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_outlines_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_outlines_struct_layout(capi):
    T, P = capi.SegItem, capi.OutlineSpec
    assert (C.sizeof(T), C.sizeof(P)) == (32, 40)
    assert [getattr(T, f).offset for f in ("x0", "y0", "x1", "y1", "color", "thickness", "dash", "flags", "reserved", "reserved2")] == [0, 4, 8, 12, 16, 20, 21, 22, 23, 24]
    assert [getattr(P, f).offset for f in ("flags", "thickness", "line_dash", "marker", "color", "alarm", "palette", "npalette", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 32, 36]
    assert capi.SEG_ITEM_DTYPE == ITEM and ITEM.itemsize == 32 and [ITEM.fields[f[0]][1] for f in T._fields_] == [getattr(T, f[0]).offset for f in T._fields_]
    assert (capi.SEG_ITEMS, capi.SEG_LIMIT, capi.OUTLINE_FIXED) == (512, 1048576, 80) == (lineref.SEG_ITEMS, lineref.SEG_LIMIT, lineref.FIXED)
    assert (capi.OUTLINE_ZONES, capi.OUTLINE_LINES, capi.OUTLINE_TICKS, capi.OUTLINE_MARKERS, capi.OUTLINE_ALARM) == (1, 2, 4, 8, 16) == \
        (lineref.ZONES, lineref.LINES, lineref.TICKS, lineref.MARKERS, lineref.ALARM)
    sp = capi.outline_spec(zones=True, lines=False, ticks=False, markers=True, alarm_on=True, thickness=3, line_dash=2, marker=7, color=(4, 5, 6), alarm=(1, 2, 3),
                           palette=[(7, 8, 9), (10, 11, 12)])
    assert (sp.flags, sp.thickness, sp.line_dash, sp.marker, list(sp.color), list(sp.alarm), sp.npalette, sp.reserved) == (25, 3, 2, 7, [4, 5, 6, 0], [1, 2, 3, 0], 2, 0)
    assert bytes((C.c_ubyte * 8).from_address(sp.palette)) == bytes([7, 8, 9, 0, 10, 11, 12, 0])
    capi.outline_spec_check(sp)
    its = capi.seg_items([(3, -4, 5, 6), (1, 2, 3, 4, (9, 8, 7), 5, 2)], 4)
    want = np.zeros(4, ITEM)
    want[0], want[1] = lineref.make_item(3, -4, 5, 6, (255, 255, 255), 1), lineref.make_item(1, 2, 3, 4, (9, 8, 7), 5, 2)
    assert its.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        capi.seg_items([(0, 0, 1, 1)] * 3, 2)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    for phrase in ("} ffgpu_seg_item;", "} ffgpu_outline_spec;", "32 bytes: x0 0, y0 4, x1 8, y1 12, color 16, thickness 20, dash 21, flags 22, reserved 23, reserved2 24",
                   "40 bytes: flags 0, thickness 4, line_dash 8, marker 12, color 16, alarm 20, palette 24, npalette 32, reserved 36",
                   "the item is X-MAJOR when |dx| >= |dy|", "S is the end point with the smaller major coordinate", "lo = (T - 1) / 2, hi = T / 2",
                   "0 <= m <= D,  and  d == 0 or ((m >> d) & 1) == 0", "if D == 0:  -lo <= r <= hi", "with e = 2 m g + D:  2 D (r - hi) <= e < 2 D (r + lo + 1)",
                   "S.y + floor((2 m g + D) / (2 D))", "the floor taken toward", "the set does not depend on the", "A solid item contains both of its",
                   "a later item overwrites an earlier one", "takes bytes 1, 2 of the LAST item in slot order that writes any of the sample's up to",
                   "The segment kernel is total over any item bytes", "Every byte of d_items for the call's targets is written", "THE STATE'S VALUES ARE THE STATE'S",
                   "Slot 8 z + i", "Slot 64 + 2 l,", "Slot 64 + 2 l + 1", "Slots 80 + 2 k and 80 + 2 k + 1", "M + (-(by - ay) / 8, (bx - ax) / 8)",
                   "id != 0 and last == frames - 1", "It is written while 80 + 2 k + 1 < items_stride", "int 16 + 4 z + 3 of event row t",
                   "computed in 64 bits and saturated to int", "Redact, then draw, then outline, then caption", "tests/outlines/lineref.py",
                   "Outlines of the zones' polygons and lines are not part of it"):
        assert phrase in hdr, phrase
    assert hdr.index("Outlines of the zones' polygons and lines are not part of it") < hdr.index("---- outlines:")     # the captions sentence stays where it was
    for name, val in (("FFGPU_SEG_ITEMS", 512), ("FFGPU_SEG_LIMIT", 1048576), ("FFGPU_OUTLINE_FIXED", 80), ("FFGPU_OUTLINE_ZONES", 1), ("FFGPU_OUTLINE_LINES", 2),
                      ("FFGPU_OUTLINE_TICKS", 4), ("FFGPU_OUTLINE_MARKERS", 8), ("FFGPU_OUTLINE_ALARM", 16)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_lines.inc"' in inc and inc.index('#include "ffgpu_text.inc"') < inc.index('#include "ffgpu_lines.inc"')
    host = open(os.path.join(CSRC, "ffgpu_lines_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    kern = open(os.path.join(CSRC, "ffgpu_lines.inc")).read()
    assert "atomic" not in kern and "printf" not in kern and "asm" not in kern


# ------------------------------------------------------------------------------------------------- the pixel set, three ways
def contract_hit(it, px, py):
    """the contract's sentence for one pixel of one item, in Python integers"""
    x0, y0, x1, y1 = (int(it[f]) for f in ("x0", "y0", "x1", "y1"))
    T, d = min(int(it["thickness"]), 8), min(int(it["dash"]), 6)
    if T == 0 or any(abs(v) > LIMIT for v in (x0, y0, x1, y1)):
        return False
    dx, dy = x1 - x0, y1 - y0
    if abs(dx) < abs(dy):                                                              # y-major: x and y exchange their roles
        x0, y0, x1, y1, px, py = y0, x0, y1, x1, py, px
    (sx, sy), (ex, ey) = ((x0, y0), (x1, y1)) if x0 <= x1 else ((x1, y1), (x0, y0))
    D, g, lo, hi = ex - sx, ey - sy, (T - 1) // 2, T // 2
    m, r = px - sx, py - sy
    if not 0 <= m <= D or (d and (m >> d) & 1):
        return False
    if D == 0:
        return -lo <= r <= hi
    e = 2 * m * g + D
    return 2 * D * (r - hi) <= e < 2 * D * (r + lo + 1)


def inequality_set(it, w, h):
    return {(x, y) for y in range(h) for x in range(w) if contract_hit(it, x, y)}


def column_loop_set(it, w, h):
    """the literal DDA: every major step from S to E, its column by Python's floor division, lo pixels before and hi behind"""
    x0, y0, x1, y1 = (int(it[f]) for f in ("x0", "y0", "x1", "y1"))
    T, d = min(int(it["thickness"]), 8), min(int(it["dash"]), 6)
    out = set()
    if T == 0 or any(abs(v) > LIMIT for v in (x0, y0, x1, y1)):
        return out
    ym = abs(x1 - x0) < abs(y1 - y0)
    a, b = ((y0, x0), (y1, x1)) if ym else ((x0, y0), (x1, y1))
    if b[0] < a[0]:
        a, b = b, a
    D, g = b[0] - a[0], b[1] - a[1]
    for m in range(D + 1):
        if d and (m >> d) & 1:
            continue
        col = a[1] + ((2 * m * g + D) // (2 * D) if D else 0)
        for n in range(col - (T - 1) // 2, col + T // 2 + 1):
            x, y = (n, a[0] + m) if ym else (a[0] + m, n)
            if 0 <= x < w and 0 <= y < h:
                out.add((x, y))
    return out


def ref_set(it, w, h):
    xs, ys = lineref.pixels(it, w, h)
    s = set(zip(xs.tolist(), ys.tolist()))
    assert len(s) == len(xs)                                                           # every pixel once
    return s


def test_pixel_set_three_ways_on_seeded_items():
    rng = np.random.default_rng(6150)
    for case in range(400):
        w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        it = fuzzcases.rand_item(rng, w, h, reach=12)
        if case % 7 == 0:
            it["thickness"] = int(rng.integers(9, 256))
        if case % 11 == 0:
            it["dash"] = int(rng.integers(7, 256))
        got = ref_set(it, w, h)
        assert got == inequality_set(it, w, h), (case, it)
        assert got == column_loop_set(it, w, h), (case, it)


def test_pixel_set_properties_on_seeded_items():
    """direction symmetry; both end points present when solid; exactly T pixels per drawn major step; the column changes by at most 1 per step; dash d
    skips exactly the steps with bit d of m set -- on a surface that holds the whole item"""
    rng = np.random.default_rng(6151)
    W = 80
    for case in range(600):
        it = fuzzcases.rand_item(rng, W - 24, W - 24, reach=0)
        it["x0"], it["x1"], it["y0"], it["y1"] = int(it["x0"]) + 12, int(it["x1"]) + 12, int(it["y0"]) + 12, int(it["y1"]) + 12
        back = it.copy()
        back["x0"], back["y0"], back["x1"], back["y1"] = it["x1"], it["y1"], it["x0"], it["y0"]
        got = ref_set(it, W, W)
        assert got == ref_set(back, W, W), case
        ym, sm, sn, D, g, T, d = lineref.canon(it)
        if d == 0:
            assert (int(it["x0"]), int(it["y0"])) in got and (int(it["x1"]), int(it["y1"])) in got, case
        per_step = {}
        for x, y in got:
            M, N = (y, x) if ym else (x, y)
            per_step.setdefault(M - sm, []).append(N)
        assert sorted(per_step) == [m for m in range(D + 1) if not (d and (m >> d) & 1)], case
        cols = {}
        for m, ns in per_step.items():
            assert len(ns) == T and max(ns) - min(ns) == T - 1, case
            cols[m] = min(ns) + (T - 1) // 2
        solid = it.copy()
        solid["dash"] = 0
        full = {}
        for x, y in ref_set(solid, W, W):
            M, N = (y, x) if ym else (x, y)
            full.setdefault(M - sm, []).append(N)
        assert all(abs(min(full[m + 1]) - min(full[m])) <= 1 for m in range(D)), case
        assert all(cols[m] == min(full[m]) + (T - 1) // 2 for m in cols), case


def test_named_cases():
    w, h = fuzzcases.NAMED_SIZE
    named = dict(fuzzcases.named_items())
    octants = set()
    for name, it in named.items():
        got = ref_set(it, w, h)
        if name != "long" and not name.startswith("at the limit"):
            assert got == inequality_set(it, w, h) == column_loop_set(it, w, h), name
        dx, dy = int(it["x1"]) - int(it["x0"]), int(it["y1"]) - int(it["y0"])
        if name.startswith("octant"):
            octants.add((dx > 0, dy > 0, abs(dx) > abs(dy), name.endswith("back")))
            assert len(got) == max(abs(dx), abs(dy)) + 1, name
    assert len(octants) == 16
    assert ref_set(named["point"], w, h) == {(5, y) for y in range(4, 9)}              # D == 0, T = 5: lo 2, hi 2 along y (a point is x-major)
    assert ref_set(seg(2, 3, 14, 15), w, h) == {(2 + k, 3 + k) for k in range(13)}     # |dx| == |dy|: x-major
    assert ref_set(named["tie"], w, h) == {(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)}     # m = 1: 2 + 4 = 6 / 8 -> 0 ... the middle column (m = 2) lies at y = 1
    assert ref_set(seg(4, 2, 0, 0), w, h) == ref_set(named["tie"], w, h)
    assert ref_set(seg(0, 0, 2, 1), w, h) == {(0, 0), (1, 1), (2, 1)}                  # the tie itself: m g / D = 1 / 2 rounds up
    assert ref_set(seg(0, 1, 2, 0), w, h) == {(0, 1), (1, 1), (2, 0)}                  # and up in the canonical direction, whichever way the segment runs
    for T in range(1, 10):                                                             # (on a surface wide enough to hold them all)
        got = ref_set(named["thickness %d" % T], 64, 48)
        rows = {y: sorted(x for x, yy in got if yy == y) for y in range(1, 22)}
        assert all(len(r) == min(T, 8) for r in rows.values()), T
        assert rows[1][0] == 1 + 4 * T - (min(T, 8) - 1) // 2, T
    assert ref_set(named["thickness 9"], 64, 48) == ref_set(seg(37, 1, 39, 21, thickness=8), 64, 48)
    d7, d6 = ref_set(named["dash 7"], w, h), ref_set(seg(-3, 20, 40, 18, dash=6), w, h)
    assert d7 == d6 and {x for x, _ in d7} == {x for x in range(w) if not ((x + 3) >> 6) & 1}
    assert {x for x, _ in ref_set(named["dash 1"], w, h)} == {x for x in range(w) if not (x >> 1) & 1}
    assert ref_set(named["at the limit x"], w, h) == {(x, 5) for x in range(w)}        # a coordinate at +-2^20 is drawn
    assert ref_set(named["at the limit y"], w, h) == {(x, y) for x in (3, 4) for y in range(h)}    # (y-major, T = 2: lo 0, hi 1 along x)
    for k in range(8):
        assert not ref_set(named["beyond the limit %d" % k], w, h), k                  # +-(2^20 + 1) and the int limits are not
    assert not ref_set(named["thickness 0"], w, h)
    # the long segment, as 64-bit arithmetic: (-2^20, -2^20 + 3) -> (2^20, 2^20) is x-major, D = 2^21, g = 2^21 - 3; pixel by pixel with Python integers
    long_ = named["long"]
    assert lineref.canon(long_) == (False, -LIMIT, -LIMIT + 3, 2 * LIMIT, 2 * LIMIT - 3, 2, 0)
    want = set()
    for x in range(w):
        m = x + LIMIT
        col = -LIMIT + 3 + (2 * m * (2 * LIMIT - 3) + 2 * LIMIT) // (4 * LIMIT)
        want |= {(x, y) for y in (col, col + 1) if 0 <= y < h}
    assert ref_set(long_, w, h) == want == inequality_set(long_, w, h) and len(want) > 30
    assert 2 * (w + LIMIT) * (2 * LIMIT - 3) > 2 ** 42                                 # (products a 32-bit int cannot hold)


def test_drawing_is_serial_in_slot_order_and_nv12_chroma_follows_the_last_writer_of_the_sample():
    rng = np.random.default_rng(6152)
    for case in range(6):
        w, h = int(rng.integers(9, 40)) | 1, int(rng.integers(7, 30)) | 1
        items = np.array([fuzzcases.rand_item(rng, w, h) for _ in range(9)], ITEM)
        pitch = 3 * w + 5
        start = rng.integers(0, 256, 16 + pitch * h + 16, dtype=np.uint8)
        a, b = start.copy(), start.copy()
        lineref.draw_bgr(a, 16, w, h, pitch, items)
        for it in items:
            for (x, y) in inequality_set(it, w, h):
                b[16 + y * pitch + 3 * x:16 + y * pitch + 3 * x + 3] = it["color"][:3]
        assert a.tobytes() == b.tobytes() and (a != start).any(), case
        assert a[16:16 + pitch * h].reshape(h, pitch)[:, 3 * w:].tobytes() == start[16:16 + pitch * h].reshape(h, pitch)[:, 3 * w:].tobytes() and a[:16].tobytes() == start[:16].tobytes()
        pitch_y, pitch_uv = w + 3, w + 1 + 4
        uv_off = 16 + pitch_y * h + 16
        start = rng.integers(0, 256, uv_off + pitch_uv * ((h + 1) // 2) + 16, dtype=np.uint8)
        a, b = start.copy(), start.copy()
        lineref.draw_nv12(a, 16, uv_off, w, h, pitch_y, pitch_uv, items)
        for it in items:
            for (x, y) in inequality_set(it, w, h):
                b[16 + y * pitch_y + x] = it["color"][0]
                b[uv_off + (y >> 1) * pitch_uv + 2 * (x >> 1)], b[uv_off + (y >> 1) * pitch_uv + 2 * (x >> 1) + 1] = it["color"][1], it["color"][2]
        assert a.tobytes() == b.tobytes() and (a != start).any(), case


# ------------------------------------------------------------------------------------------------- the composer
def one_scene(zones=(), lines=(), nzones=None, nlines=None):
    sc = zoneref.make_scene(zones, lines)
    if nzones is not None:
        sc["nzones"] = nzones
    if nlines is not None:
        sc["nlines"] = nlines
    return np.array([sc], zoneref.SCENE_DTYPE)


def compose(scenes, spec, stride=80, state=None, events=None, capacity=4, streams=(0,)):
    state = zoneref.State(1, capacity) if state is None else state
    events = np.zeros((len(streams), 64), "<u4") if events is None else events
    return lineref.outline_scene(scenes, np.frombuffer(state.tobytes(), np.uint8), 1, capacity, events, events.shape[1], list(streams), spec, stride)


def ends(it):
    return tuple(int(it[f]) for f in ("x0", "y0", "x1", "y1"))


SQUARE = [(1.9, 2.9), (10.2, 2), (10, 12), (-1.5, 12.7)]


def test_composer_slot_layout_and_colours():
    sc = one_scene([(SQUARE,), ([(0, 0), (5, 0), (0, 5)],)], [((1, 2), (30, 4)), ((7.9, -0.9), (7, 40))])
    pal = [(k, k + 1, k + 2) for k in range(0, 30, 3)]
    sp = lineref.Spec(lineref.ZONES | lineref.LINES | lineref.TICKS, 3, 2, palette=pal)
    it = compose(sc, sp)[0]
    assert [ends(it[k]) for k in range(4)] == [(1, 2, 10, 2), (10, 2, 10, 12), (10, 12, -1, 12), (-1, 12, 1, 2)]       # toward zero; the last edge closes the polygon
    assert [ends(it[8 + k]) for k in range(3)] == [(0, 0, 5, 0), (5, 0, 0, 5), (0, 5, 0, 0)]
    used = it["thickness"] > 0
    assert [int(k) for k in np.nonzero(used)[0]] == [0, 1, 2, 3, 8, 9, 10, 64, 65, 66, 67]
    assert not it[~used].view(np.uint8).any()
    assert all(int(it[k]["thickness"]) == 3 and int(it[k]["dash"]) == 0 for k in (0, 3, 8, 10))
    assert (int(it[64]["thickness"]), int(it[64]["dash"]), int(it[65]["thickness"]), int(it[65]["dash"])) == (3, 2, 1, 0)
    assert ends(it[64]) == (1, 2, 30, 4) and ends(it[66]) == (7, 0, 7, 40)
    assert [list(it[k]["color"]) for k in (0, 8, 64, 65, 66)] == [[0, 1, 2, 0], [3, 4, 5, 0], [24, 25, 26, 0], [24, 25, 26, 0], [27, 28, 29, 0]]
    assert not it["flags"].any() and not it["reserved"].any() and not it["reserved2"].any()
    one = compose(sc, lineref.Spec(lineref.ZONES | lineref.LINES, 1, color=(7, 8, 9)))[0]
    assert {tuple(c) for c in one["color"][one["thickness"] > 0]} == {(7, 8, 9, 0)} and (one["thickness"] > 0).sum() == 9
    assert list(compose(sc, lineref.Spec(lineref.ZONES, 1, palette=pal[:2]))[0][8]["color"]) == [3, 4, 5, 0]
    assert not compose(sc, sp, streams=(-1,)).view(np.uint8).any()                      # an entry of -1: all-zero items
    # the counts are clamped as the zones kernel clamps them
    assert (compose(one_scene([(SQUARE,)] * 8, nzones=11), lineref.Spec(lineref.ZONES))[0]["thickness"] > 0).sum() == 32
    assert not compose(one_scene([(SQUARE,)] * 8, nzones=-3), lineref.Spec(lineref.ZONES)).view(np.uint8).any()
    assert (compose(one_scene([], [((0, 0), (1, 1))] * 8, nlines=12), lineref.Spec(lineref.LINES))[0]["thickness"] > 0).sum() == 8


def test_tick_end_points_point_to_the_forward_side():
    for (ax, ay), (bx, by), want in (((0, 0), (16, 0), (8, 0, 8, 2)), ((0, 0), (0, 16), (0, 8, -2, 8)), ((16, 16), (0, 0), (8, 8, 10, 6)), ((0, 16), (16, 0), (8, 8, 10, 10)),
                                     ((1, 2), (30, 5), (15, 3, 15, 6)), ((-1, -2), (-30, -5), (-16, -4, -16, -7)), ((3, 4), (-12, 27), (-5, 15, -7, 14)),
                                     ((3, 4), (12, -27), (7, -12, 10, -11))):
        assert lineref.tick_ends(ax, ay, bx, by) == want, (ax, ay, bx, by)
        it = compose(one_scene([], [((ax, ay), (bx, by))]), lineref.Spec(lineref.LINES | lineref.TICKS))[0]
        assert ends(it[65]) == want
        mx, my, ex, ey = want
        if (ex, ey) != (mx, my):                                                       # the zones contract's side(P) is true at the tick's far end
            assert zoneref.side(ax, ay, bx, by, ex, ey) and not zoneref.side(ax, ay, bx, by, 2 * mx - ex, 2 * my - ey)
    # odd sums: the shifts are arithmetic (floor), the divisions go toward zero
    assert lineref.tick_ends(-3, -3, 0, 0) == (-2, -2, -2, -2) and lineref.tick_ends(0, 0, -15, 15) == (-8, 7, -9, 6) and lineref.tick_ends(0, 0, 15, -15) == (7, -8, 8, -7)
    # far-off ends: computed in 64 bits, saturated to int; the primitive drops such an item
    it = compose(one_scene([], [((-3e9, 0), (3e9, 7))]), lineref.Spec(lineref.LINES | lineref.TICKS))[0]
    assert ends(it[64]) == (IMIN, 0, IMAX, 7) and ends(it[65]) == (-1, 3, -1, 3 + (2 ** 32 - 1) // 8)
    it = compose(one_scene([], [((0, -3e9), (8, 3e9))]), lineref.Spec(lineref.LINES | lineref.TICKS))[0]
    assert ends(it[65]) == (4, -1, 4 - (2 ** 32 - 1) // 8, 0) and not len(lineref.pixels(it[65], 64, 48)[0]) and not len(lineref.pixels(it[64], 64, 48)[0])
    it = compose(one_scene([], [((INF, -INF), (NAN, 5))]), lineref.Spec(lineref.LINES))[0]
    assert ends(it[64]) == (IMAX, IMIN, 0, 5)


def test_alarm_switch():
    sc = one_scene([(SQUARE,), (SQUARE,)])
    ev = np.zeros((1, 70), "<u4")
    ev[0, 16 + 4 * 1 + 3] = 2
    ev[0, 16:19] = 5                                                                   # occupancy, entered, left of zone 0: not the loitering count
    on = compose(sc, lineref.Spec(lineref.ZONES | lineref.ALARM, color=(1, 1, 1), alarm=(9, 8, 7)), events=ev)[0]
    assert list(on[0]["color"]) == [1, 1, 1, 0] and list(on[8]["color"]) == [9, 8, 7, 0] and list(on[11]["color"]) == [9, 8, 7, 0]
    off = compose(sc, lineref.Spec(lineref.ZONES, color=(1, 1, 1), alarm=(9, 8, 7)), events=ev)[0]
    assert list(off[8]["color"]) == [1, 1, 1, 0]


def planted(frames, slots):
    """a state of one stream: header frames, slots = [(id, last, px, py)]"""
    st = zoneref.State(1, len(slots))
    st.hdr[0, 0] = frames % 2 ** 32
    for q, (id_, last, px, py) in enumerate(slots):
        st.slots[0, q]["id"], st.slots[0, q]["last"], st.slots[0, q]["px"], st.slots[0, q]["py"] = id_, np.uint32(last % 2 ** 32).astype(np.int32), px, py
    return st


def test_seen_rule_and_markers():
    sp = lineref.Spec(lineref.MARKERS, marker=3, palette=[(1, 1, 1), (2, 2, 2), (3, 3, 3)])
    sc = one_scene()
    slots = [(5, 6, 10.9, 20.2), (0, 6, 1, 1), (7, 5, 2, 2), (-4, 6, -7.9, 3), (9, 7, 3, 3)]
    it = compose(sc, sp, 96, planted(7, slots), capacity=5)[0]                          # seen: last == frames - 1 = 6 and id != 0: slots 0 and 3, in slot order
    assert [ends(it[k]) for k in range(80, 84)] == [(7, 20, 13, 20), (10, 17, 10, 23), (-10, 3, -4, 3), (-7, 0, -7, 6)]
    assert [list(it[k]["color"]) for k in (80, 81, 82)] == [[3, 3, 3, 0], [3, 3, 3, 0], [3, 3, 3, 0]]           # 5 mod 3 = 2; -4 mod 3 = 2, the non-negative remainder
    assert not it[84:].view(np.uint8).any() and not it[:80].view(np.uint8).any()
    assert all(int(it[k]["thickness"]) == 1 and int(it[k]["dash"]) == 0 for k in range(80, 84))
    # frames = 0: frames - 1 is 2^32 - 1; frames = 1: last == 0; the wrap at 2^32
    assert (compose(sc, sp, 96, planted(0, [(1, -1, 1, 1), (2, 0, 1, 1)]), capacity=2)[0]["thickness"] > 0).sum() == 2
    assert ends(compose(sc, sp, 96, planted(0, [(1, 0, 1, 1), (2, 2 ** 32 - 1, 5, 5)]), capacity=2)[0][80]) == (2, 5, 8, 5)
    assert ends(compose(sc, sp, 96, planted(1, [(1, 1, 1, 1), (2, 0, 5, 5)]), capacity=2)[0][80]) == (2, 5, 8, 5)
    assert ends(compose(sc, sp, 96, planted(2 ** 32, [(1, 2 ** 32 - 1, 9, 9)]), capacity=1)[0][80]) == (6, 9, 12, 9)
    assert not compose(sc, sp, 96, planted(2 ** 32 - 1, [(1, 2 ** 32 - 1, 9, 9)]), capacity=1).view(np.uint8).any()
    # the cut: written while 80 + 2 k + 1 < items_stride
    many = planted(3, [(q + 1, 2, q, q) for q in range(128)])
    for stride, n in ((80, 0), (81, 0), (82, 1), (83, 1), (84, 2), (512, 128)):
        got = compose(sc, sp, stride, many, capacity=128)[0]
        assert (got["thickness"] > 0).sum() == 2 * n and (n == 0 or ends(got[80 + 2 * n - 1]) == (n - 1, n - 4, n - 1, n + 2)), stride
    # a far-off anchor: saturated, and dropped by the primitive; NaN -> 0
    it = compose(sc, sp, 96, planted(1, [(1, 0, 3e9, NAN)]), capacity=1)[0]
    assert ends(it[80]) == (IMAX - 3, 0, IMAX, 0) and ends(it[81]) == (IMAX, -3, IMAX, 3) and not len(lineref.pixels(it[80], 64, 48)[0])


def test_zones_that_contain_nothing_draw_nothing_and_inf_vertices_saturate():
    tri = [(1, 1), (9, 1), (1, 9)]
    sp = lineref.Spec(lineref.ZONES)
    assert not compose(one_scene([(tri[:2],)]), sp).view(np.uint8).any()                # nverts 2
    nine = one_scene([(SQUARE + SQUARE,)])
    nine["zone"]["nverts"][0, 0] = 9
    assert not compose(nine, sp).view(np.uint8).any()                                  # nverts 9
    nan = one_scene([(tri,), (tri,)])
    nan["zone"]["y"][0, 0, 2] = NAN
    got = compose(nan, sp)[0]
    assert not got[:8].view(np.uint8).any() and (got[8:16]["thickness"] > 0).sum() == 3      # a NaN among the used vertices: that zone alone
    unused = one_scene([(tri,)])
    unused["zone"]["x"][0, 0, 5] = NAN
    assert (compose(unused, sp)[0]["thickness"] > 0).sum() == 3                         # a NaN behind nverts does not count
    inf = one_scene([([(INF, 1), (9, -INF), (-3e9, 2147483520.0)],)])
    got = compose(inf, sp)[0]
    assert [ends(got[k]) for k in range(3)] == [(IMAX, 1, 9, IMIN), (9, IMIN, IMIN, 2147483520), (IMIN, 2147483520, IMAX, 1)]
    assert all(not len(lineref.pixels(got[k], 64, 48)[0]) for k in range(3))


def test_every_flag_combination(capi):
    for f in range(64):
        sp = capi.outline_spec(thickness=2, marker=3)
        sp.flags = f
        legal = f < 32 and bool(f & 11) and (not f & 4 or bool(f & 2)) and (not f & 16 or bool(f & 1))
        assert (capi.lib().ffgpu_outline_spec_check(sp) == 0) == legal, f
        if legal:                                                                      # and lineref writes only the parts named
            st = planted(1, [(1, 0, 5, 5)])
            ev = np.ones((1, 64), "<u4")
            it = compose(one_scene([(SQUARE,)], [((0, 0), (9, 9))]), lineref.Spec(f, 2, 0, 3), 96, st, ev, capacity=1)[0]
            used = it["thickness"] > 0
            assert (bool(used[:64].any()), bool(used[64]), bool(used[65]), bool(used[80:].any())) == (bool(f & 1), bool(f & 2), bool(f & 4), bool(f & 8)), f
    assert capi.lib().ffgpu_outline_spec_check(None) < 0 and "NULL spec" in capi.last_error()


# ------------------------------------------------------------------------------------------------- the GPU fuzz's seeds
def test_fuzz_seeds_meet_the_conditions_on_the_reference_alone():
    """the seeded cases of the GPU fuzz (tests/outlines/fuzzcases.py) through lineref, no device -- a condition on the inputs: per surface format at
    least a quarter of the targets have two items that write a common pixel with different colours, a quarter an item cut by an edge, (NV12) a quarter a
    chroma sample two items share; every octant, every thickness 1..8 and every dash 0..6 occurs; a rounding tie occurs; outside the hostile case at
    most half of a case's used items fall wholly outside their target"""
    tot = fuzzcases.check_seg_stats()
    print(tot)
    for nv12 in (False, True):
        cs = fuzzcases.seg_cases(nv12)
        assert sorted(cs) == sorted(fuzzcases.SEG_NAMES)
        assert {c.stride for c in cs.values()} >= {3, 64, 512} and max(c.n for c in cs.values()) > 64
        assert any(t is None for c in cs.values() for t in c.targets)
        assert any(int(it["x0"]) in (IMIN, IMAX) for it in cs["hostile"].items.reshape(-1))
        assert all(g["w"] <= 64 and g["h"] <= 48 for c in cs.values() for g in c.targets if g is not None)
        for c in cs.values():
            assert (c.want() != c.start).any(), c.what
        named = cs["named"]
        assert fuzzcases.NAMED_SIZE == (named.targets[0]["w"], named.targets[0]["h"]) == (37, 23)
        assert any(ends(it) == (-LIMIT, -LIMIT + 3, LIMIT, LIMIT) for it in named.items[0])
    bgr = [g for c in fuzzcases.seg_cases(False).values() for g in c.targets if g is not None]
    assert all(g["off"] % 2 == 1 and g["pitch"] > 3 * g["w"] for g in bgr) and any(g["pitch"] % 2 for g in bgr)
    odd = [g for c in fuzzcases.seg_cases(True).values() for g in c.targets if g is not None]
    assert any(g["w"] % 2 and g["h"] % 2 for g in odd) and any(g["w"] % 2 == 0 for g in odd)
    ss = fuzzcases.scene_cases()
    assert sorted(ss) == sorted(fuzzcases.SCENE_NAMES) and max(c.n for c in ss.values()) > 512 and {c.items_stride for c in ss.values()} >= {80, 512}
    assert any(-1 in c.streams for c in ss.values())
    for c in ss.values():
        used = c.want_items["thickness"] > 0
        assert used[:, :64].any() and not used[:, :64].all(), c.what
        if c.spec.flags & lineref.MARKERS and c.items_stride > 81:
            assert used[:, 80:].any(), c.what
    six, big = ss["six streams"], ss["stride 512"]
    used = six.want_items["thickness"] > 0
    assert used[:, 64:80:2].any() and used[:, 65:80:2].any() and not used[:, 80:].any()
    assert any(tuple(it["color"][:3]) == six.spec.alarm for it in six.want_items[:, :64].reshape(-1)) and (big.want_items["thickness"][:, 80:] > 0).sum(axis=1).max() > 64
    assert {int(s["nzones"]) for c in ss.values() for s in c.scenes} >= {0, 8, 11} and {int(z["nverts"]) for c in ss.values() for s in c.scenes for z in s["zone"]} >= {2, 3, 8, 9}
    coords = np.concatenate([c.want_items[f].reshape(-1) for c in ss.values() for f in ("x0", "y0", "x1", "y1")])
    assert (coords == IMAX).any() and (coords == IMIN).any()


# ------------------------------------------------------------------------------------------------- without a device; the host glue
def test_outlines_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_draw_segments_bgr_dev(None, 1, None, 1, None),
                 lambda: L.ffgpu_draw_segments_nv12_dev(None, 1, None, 1, None),
                 lambda: L.ffgpu_outline_scene_dev(None, None, 1, 1, None, 64, None, 1, None, None, 80, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


def test_host_glue_under_the_sanitizers():
    """san/lines_driver.cc: the outline spec's plan and every argument check of ffgpu_lines_host.hpp on the CPU under ASan + UBSan, as a child process;
    the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "lines"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_lines_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"lines_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 60, out[-1]
    assert not any("WRONG" in ln for ln in out)
    for ln in ("plan.color_values holds", "plan.palette_values holds", "spec.every_flag_combination holds", "plan.null_spec -1 op: NULL spec",
               "spec.flags_0 -1 op: flags 0x0 name no part (FFGPU_OUTLINE_ZONES | _LINES | _MARKERS)", "spec.flags_32 -1 op: unknown flags 0x21",
               "spec.ticks_without_lines -1 op: FFGPU_OUTLINE_TICKS without FFGPU_OUTLINE_LINES", "spec.alarm_without_zones -1 op: FFGPU_OUTLINE_ALARM without FFGPU_OUTLINE_ZONES",
               "spec.thickness_0 -1 op: thickness 0 is outside 1..8", "spec.thickness_9 -1 op: thickness 9 is outside 1..8", "spec.dash_7 -1 op: line_dash 7 is outside 0..6",
               "spec.marker_33 -1 op: marker 33 is outside 0..32", "spec.marker_0_with_markers -1 op: marker 0 with FFGPU_OUTLINE_MARKERS (at least 1)",
               "spec.npalette_without_palette -1 op: npalette 3 (0 with a NULL palette, else 1..256)", "spec.reserved -1 op: reserved must be 0",
               "scene.null_scenes -1 op: NULL scenes", "scene.null_items -1 op: NULL items", "scene.stride_79 -1 op: items_stride 79 is outside 80..512",
               "scene.stride_513 -1 op: items_stride 513 is outside 80..512", "scene.events_stride_63 -1 op: events_stride 63 is below FFGPU_ZONES_ROW = 64",
               "scene.stream_high -1 op: target 1: stream 2 is outside -1 .. 1", "scene.capacity_129 -1 op: capacity 129 is outside 1..128",
               "segments.null_targets -1 op: NULL targets", "segments.ntargets_0 -1 op: 0 targets (ntargets >= 1)", "segments.stride_0 -1 op: items_stride 0 is outside 1..512",
               "segments.stride_513 -1 op: items_stride 513 is outside 1..512", "segments.items_unaligned -1 op: the items must be 4-byte aligned"):
        assert ln in out, ln
