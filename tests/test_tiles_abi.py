"""Tiled detection without a GPU: the tile structure's layout in the ctypes mirror, the exported symbols, tests/tiles/mergeref.py (the numpy
restatement of the merge contract the GPU tests compare with) pinned to the oracle's NMS on tie-free lists, the planner's properties, and the
device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C

import numpy as np
import pytest

from tiles import mergeref

SYMBOLS = ["ffgpu_merge_tiles_scratch_bytes", "ffgpu_merge_tiles_dev", "ffgpu_exec_merge_tiles", "ffgpu_exec_merged_dev", "ffgpu_exec_read_merged",
           "ffgpu_exec_read_merged_boxes", "ffgpu_tile_plan"]


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_tile_struct_layout(capi):
    T = capi.Tile
    assert C.sizeof(T) == 16
    assert (T.image.offset, T.x0.offset, T.y0.offset, T.reserved.offset) == (0, 4, 8, 12)
    assert mergeref.BOX_DTYPE == capi.BOX_DTYPE and mergeref.DETS_DTYPE == capi.DETS_DTYPE and mergeref.MAX_DET == capi.FFGPU.MAX_DET


def test_tile_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_header_states_the_contract():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffcnn_hip.h")).read()
    assert "} ffgpu_tile;" in hdr and "TWO-STAGE NMS" in hdr
    assert int(re.search(r"#define FFGPU_MERGE_LDS_SLOTS\s+(\d+)", hdr).group(1)) == 1024


def overlapping_list(rng, n, tight=False):
    """n boxes of classes 0-3 crowded into a small area (both outcomes of the suppression test occur), distinct scores in (0, 1); tight: similar
    boxes around three centres, so that intersection / union passes 0.5 often enough too"""
    b = np.zeros(n, mergeref.BOX_DTYPE)
    b["type"] = rng.integers(0, 4, n)
    b["score"] = rng.permutation(np.arange(1, 4001))[:n].astype(np.float32) / np.float32(4001)
    cx, cy = rng.uniform(0, 200, n), rng.uniform(0, 200, n)
    w, h = rng.uniform(20, 140, n), rng.uniform(20, 140, n)
    if tight:
        c = rng.integers(0, 3, n)
        cx, cy = 150.0 * c + rng.uniform(-25, 25, n), 90.0 * c + rng.uniform(-25, 25, n)
        w, h = rng.uniform(70, 130, n), rng.uniform(70, 130, n)
    b["x1"], b["y1"], b["x2"], b["y2"] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    return b


@pytest.mark.parametrize("use_min", [1, 0])
def test_mergeref_is_the_oracles_nms(orc, use_min):
    """200 seeded tie-free lists of 0-300 boxes: one tile at (0, 0) through mergeref is orc.nms(..., 0.5, use_min, 1, 1) byte for byte; and
    at least a tenth of the examined same-class pairs are suppressed, at least a tenth kept"""
    rng = np.random.default_rng(20260 + use_min)
    stats = {}
    for case in range(200):
        n = int(rng.integers(0, 301)) if case > 2 else (0, 1, 300)[case]
        b = overlapping_list(rng, n, tight=not use_min)
        assert len(np.unique(b["score"])) == n
        got = mergeref.merge([b], [(0, 0)], 0.5, use_min, stats)
        want = orc.nms(b, 0.5, use_min, 1, 1)
        assert got.tobytes() == want.tobytes(), "case %d (%d boxes): %d vs %d survivors" % (case, n, len(got), len(want))
    total = stats["suppressed"] + stats["kept"]
    assert stats["suppressed"] * 10 >= total and stats["kept"] * 10 >= total, stats


def test_mergeref_translation_order_and_record():
    """what orc.nms cannot pin: the translation, the tie order (tile position, then index) and the record's fields"""
    a = np.zeros(2, mergeref.BOX_DTYPE)
    a["type"], a["score"] = 1, (0.9, 0.5)
    a["x1"], a["y1"], a["x2"], a["y2"] = (0, 100), (0, 100), (10, 110), (10, 110)
    far = mergeref.merge([a, a], [(1000, 0), (0, 2000)])                       # disjoint after translation: all four, ties in table order
    assert [(float(b["x1"]), float(b["y1"])) for b in far] == [(1000, 0), (0, 2000), (1100, 100), (100, 2100)]
    same = mergeref.merge([a, a], [(7, 9), (7, 9)])                            # a tile listed twice: the first listing's boxes survive
    assert same.tobytes() == mergeref.merge([a], [(7, 9)]).tobytes()
    recs = np.zeros(2, mergeref.DETS_DTYPE)
    recs["ncand"], recs["overflow"] = (5, 7), (2, 5)
    r = mergeref.record(far, recs)
    assert (int(r["count"]), int(r["nfull"]), int(r["ncand"]), int(r["overflow"])) == (4, 4, 12, 1)
    assert r["box"][:4].tobytes() == far.tobytes() and not r["box"][4:].tobytes().strip(b"\0")
    many = np.zeros(130, mergeref.BOX_DTYPE)
    many["score"] = 0.5
    many["type"] = np.arange(130)
    r = mergeref.record(many, recs[:1])
    assert (int(r["count"]), int(r["nfull"]), int(r["overflow"])) == (128, 130, 4)
    assert len(mergeref.merge([], [])) == 0 and len(mergeref.merge([a[:0]], [(3, 4)])) == 0


def check_plan(capi, W, H, tw, th, ox, oy, align):
    plan = capi.tile_plan(W, H, tw, th, ox, oy, align)
    assert plan == capi.tile_plan(W, H, tw, th, ox, oy, align)                  # deterministic
    assert len({(w, h) for _, _, w, h in plan}) == 1
    w, h = plan[0][2:]
    assert min(tw, W) <= w <= min(tw, W) + (align - 1) and min(th, H) <= h <= min(th, H) + (align - 1)
    xs, ys = sorted({p[0] for p in plan}), sorted({p[1] for p in plan})
    assert plan == [(x, y, w, h) for y in ys for x in xs]                       # a grid, rows first
    for org, size, length, ov in ((xs, w, W, ox), (ys, h, H, oy)):
        assert org[0] == 0 and org[-1] + size == length                         # first at 0, last ends at the edge: contained
        assert all(o % align == 0 for o in org)
        covered = np.zeros(length, bool)
        for o in org:
            assert 0 <= o and o + size <= length
            covered[o:o + size] = True
        assert covered.all()
        for a, b in zip(org, org[1:]):
            assert a < b and a + size - b >= ov - (align - 1), (org, size, ov)
    short = (capi.TileRect * 1)()
    assert capi.lib().ffgpu_tile_plan(W, H, tw, th, ox, oy, align, short, 1) == len(plan)      # the count, also when cap is short
    assert (short[0].x0, short[0].y0, short[0].w, short[0].h) == plan[0]
    return plan


def test_planner_fixed_cases(capi):
    assert len(check_plan(capi, 1920, 1080, 640, 640, 64, 64, 1)) == 4 * 2
    assert len(check_plan(capi, 3840, 2160, 640, 640, 128, 128, 2)) == 8 * 4
    assert check_plan(capi, 640, 424, 640, 640, 0, 0, 1) == [(0, 0, 640, 424)]
    assert check_plan(capi, 100, 50, 320, 320, 16, 16, 2) == [(0, 0, 100, 50)]          # a picture smaller than the tile
    assert check_plan(capi, 1280, 848, 800, 600, 200, 200, 1) == [(0, 0, 800, 600), (480, 0, 800, 600), (0, 248, 800, 600), (480, 248, 800, 600)]
    assert check_plan(capi, 1280, 848, 640, 424, 0, 0, 2) == [(0, 0, 640, 424), (640, 0, 640, 424), (0, 424, 640, 424), (640, 424, 640, 424)]
    assert check_plan(capi, 7, 1, 2, 1, 0, 0, 2)[0][2:] == (3, 1)                        # align 2: 7 - 2 is odd, the tile grows by one


def test_planner_sweep(capi):
    rng = np.random.default_rng(5160)
    n = 0
    for case in range(1500):
        align = 1 + case % 2
        W, H = int(rng.integers(1, 4001)), int(rng.integers(1, 4001))
        if case % 5 == 0:                                                       # small pictures and tiles, where the edge cases live
            W, H = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        tw, th = int(rng.integers(1, 1001)), int(rng.integers(1, 1001))
        if case % 5 < 2:
            tw, th = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        ox, oy = int(rng.integers(0, tw)), int(rng.integers(0, th))
        if case % 7 == 0:
            ox, oy = tw - 1, th - 1
        if align == 2 and ((tw < 2 and W > tw) or (th < 2 and H > th)):         # even origins of 1-pixel tiles cannot cover a picture
            with pytest.raises(RuntimeError, match="at least 2 pixels"):
                capi.tile_plan(W, H, tw, th, ox, oy, align)
            continue
        check_plan(capi, W, 1, tw, 1, ox, 0, align)                               # each axis on its own (up to 4000 tiles) ...
        check_plan(capi, 1, H, 1, th, 0, oy, align)
        if (-(-W // max(1, tw - ox))) * (-(-H // max(1, th - oy))) <= 20000:     # ... and the grid where it is not millions of tiles
            check_plan(capi, W, H, tw, th, ox, oy, align)
        n += 1
    assert n > 1000


def test_planner_rejects(capi):
    L = capi.lib()
    out = (capi.TileRect * 4)()
    for args, msg in (((100, 100, 50, 50, 50, 0, 1), "overlap"), ((100, 100, 50, 50, 0, 77, 1), "overlap"), ((100, 100, 50, 50, -1, 0, 1), "overlap"),
                      ((100, 100, 50, 50, 0, 0, 0), "align"), ((100, 100, 50, 50, 0, 0, 3), "align"), ((100, 100, 50, 50, 0, 0, 4), "align"),
                      ((0, 100, 50, 50, 0, 0, 1), "sizes"), ((100, 100, 50, 0, 0, 0, 1), "sizes"), ((5, 5, 1, 3, 0, 0, 2), "at least 2 pixels")):
        assert L.ffgpu_tile_plan(*args, out, 4) < 0, args
        assert msg in capi.last_error(), (args, capi.last_error())
    assert L.ffgpu_tile_plan(100, 100, 50, 50, 0, 0, 1, None, 4) < 0 and "NULL" in capi.last_error()
    assert L.ffgpu_tile_plan(100, 100, 50, 50, 0, 0, 1, None, 0) == 4            # the count alone


def test_tile_helpers(capi):
    arr = capi.tile_table([(0, 0, 0), (-1, 0, 0), (1, 640, 424)])
    assert [(t.image, t.x0, t.y0, t.reserved) for t in arr] == [(0, 0, 0, 0), (-1, 0, 0, 0), (1, 640, 424, 0)]
    assert capi.tile_table(arr) is arr
    assert capi.merge_tiles_scratch_bytes(4, 128) >= 36 * 2 * 4 * 128 and capi.merge_tiles_scratch_bytes(0, 128) == 0


def test_merge_tiles_without_device(capi):
    """with no HIP device both device entry points say so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    tiles = capi.tile_table([(0, 0, 0)])
    rc1 = capi.lib().ffgpu_exec_merge_tiles(None, tiles, 1, 1, None)
    e1 = capi.last_error()
    rc2 = capi.lib().ffgpu_merge_tiles_dev(None, None, 0, tiles, 1, 1, 0.5, 1, None, None, None, 0, None)
    e2 = capi.last_error()
    assert rc1 < 0 and rc2 < 0
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert want in e1 and want in e2, (e1, e2)
