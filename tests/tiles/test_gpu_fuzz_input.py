"""Tiled detection on the device: ffgpu_merge_tiles_dev (the operator, on synthetic records and lists) and ffgpu_exec_merge_tiles (behind a
forward of the real net) against tests/tiles/mergeref.py, the numpy restatement of the contract in include/ffcnn_hip.h, byte for byte --
records and full lists.  mergeref, not orc.nms directly: a tiled picture produces exact score ties from identical pixels, which the
reference's qsort orders as it likes; tests/test_tiles_abi.py pins mergeref to orc.nms on tie-free lists.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from test_gpu_parity import boxes_match
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)
from tiles import mergeref

pytestmark = pytest.mark.gpu
BOX, DETS = mergeref.BOX_DTYPE, mergeref.DETS_DTYPE
COUNTS = (0, 1, 2, 127, 128, 129, 300)


def rand_list(rng, n):
    """n boxes of classes 0-3 in score order, crowded into 200 x 200 pixels so that the suppression test goes both ways"""
    b = np.zeros(n, BOX)
    b["type"] = rng.integers(0, 4, n)
    b["score"] = np.sort(rng.uniform(0.05, 1.0, n).astype(np.float32))[::-1]
    cx, cy = rng.uniform(0, 200, n), rng.uniform(0, 200, n)
    w, h = rng.uniform(20, 140, n), rng.uniform(20, 140, n)
    b["x1"], b["y1"], b["x2"], b["y2"] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    return b


def spread_list(rng, n):
    """n boxes that never suppress each other: one class each"""
    b = rand_list(rng, n)
    b["type"] = np.arange(n)
    return b


def records_of(rng, lists):
    """the records k_nms would leave beside these full lists"""
    r = np.zeros(len(lists), DETS)
    for t, b in enumerate(lists):
        n = len(b)
        r[t]["count"], r[t]["nfull"] = min(n, 128), n
        r[t]["ncand"] = n + int(rng.integers(0, 50))
        r[t]["overflow"] = int(rng.integers(0, 2)) | (4 if n > 128 else 0)
        r[t]["box"][:min(n, 128)] = b[:128]
    return r


def run_op(F, recs, lists, tiles, nimages, stride=None, scratch=True, thresh=0.5, use_min=1):
    """ffgpu_merge_tiles_dev on device copies; returns (records, [full list per picture]).  lists None: the records' own boxes.  The output
    buffers start as 0xA5 bytes: whatever is compared was written by the kernel."""
    import torch
    ntiles = len(tiles)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    d_lists = None
    if lists is not None:
        stride = stride or max(1, max(len(b) for b in lists))
        flat = np.zeros((ntiles, stride), BOX)
        flat.view(np.uint8)[:] = 0x3C                                           # (slots behind a list hold junk: never read)
        for t, b in enumerate(lists):
            flat[t, :len(b)] = b
        d_lists = torch.from_numpy(flat.view(np.uint8).reshape(-1)).cuda()
    S = stride if lists is not None else F.FFGPU.MAX_DET
    off = np.concatenate([[0], np.cumsum([sum(1 for e in tiles if e[0] == g) for g in range(nimages)])])
    out_recs = torch.full((nimages * DETS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    out_lists = torch.full((max(1, int(off[-1]) * S) * BOX.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    nbytes = F.merge_tiles_scratch_bytes(ntiles, S)
    d_scr = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if scratch else None
    F.merge_tiles_dev(d_recs.data_ptr(), d_lists.data_ptr() if d_lists is not None else None, stride or 0, tiles, nimages,
                      out_recs.data_ptr(), out_lists.data_ptr(), thresh, use_min, d_scr.data_ptr() if scratch else None, nbytes if scratch else 0)
    torch.cuda.synchronize()
    got_r = np.frombuffer(out_recs.cpu().numpy().tobytes(), DETS)
    ol = np.frombuffer(out_lists.cpu().numpy().tobytes(), BOX)
    return got_r, [ol[S * int(off[g]):S * int(off[g]) + max(0, int(got_r[g]["nfull"]))] for g in range(nimages)]


def check_op(F, recs, lists, tiles, nimages, what, **kw):
    got_r, got_l = run_op(F, recs, lists, tiles, nimages, **kw)
    want_r, want_l = mergeref.merge_table(recs, lists, tiles, nimages, kw.get("thresh", 0.5), kw.get("use_min", 1))
    for g in range(nimages):
        for f in ("count", "ncand", "overflow", "nfull"):
            assert int(got_r[g][f]) == int(want_r[g][f]), "%s picture %d: %s %d, want %d" % (what, g, f, got_r[g][f], want_r[g][f])
        assert got_r[g].tobytes() == want_r[g].tobytes(), "%s picture %d: record" % (what, g)
        assert got_l[g].tobytes() == want_l[g].tobytes(), "%s picture %d: full list" % (what, g)
    return got_r, got_l


@pytest.mark.parametrize("seed", range(4))
def test_operator_fuzz(F, seed):
    """1-6 tiles in 1-3 pictures, entries that are no tile, the tiles of a picture scattered over the table, per-tile counts from COUNTS,
    origins 0-4000, both metrics"""
    rng = np.random.default_rng(7700 + seed)
    some_suppressed = some_kept = 0
    for case in range(8):
        nimages = int(rng.integers(1, 4))
        ntiles = int(rng.integers(max(1, nimages), 7))
        images = list(rng.integers(0, nimages, ntiles))                         # any picture at any table position: rows of the CSR are not contiguous
        for t in range(ntiles):
            if rng.random() < 0.2 and ntiles > nimages:
                images[t] = -1
        tiles = [(int(g), int(rng.integers(0, 4001)), int(rng.integers(0, 4001))) for g in images]
        if case % 2:                                                            # near origins: the tiles' boxes meet across tiles
            tiles = [(g, int(rng.integers(0, 60)), int(rng.integers(0, 60))) for g, _, _ in tiles]
        lists = [rand_list(rng, int(rng.choice(COUNTS))) for _ in range(ntiles)]
        recs = records_of(rng, lists)
        use_min = int(case % 4 != 3)
        got_r, _ = check_op(F, recs, lists, tiles, nimages, "seed %d case %d" % (seed, case), stride=300 + int(rng.integers(0, 9)), use_min=use_min)
        union = sum(len(lists[t]) for t in range(ntiles) if tiles[t][0] >= 0)
        kept = sum(int(r["nfull"]) for r in got_r)
        some_suppressed += union - kept
        some_kept += kept
    assert some_suppressed > 100 and some_kept > 100


@pytest.mark.parametrize("union", [255, 256, 257])
def test_operator_union_sizes_around_a_power_of_two(F, union):
    rng = np.random.default_rng(union)
    lists = [rand_list(rng, 127), rand_list(rng, union - 127 - 2), rand_list(rng, 0), rand_list(rng, 2)]
    tiles = [(0, 0, 0), (0, 31, 7), (0, 5, 5), (0, 100, 90)]
    check_op(F, records_of(rng, lists), lists, tiles, 1, "union %d" % union)
    one = [spread_list(rng, union)]
    check_op(F, records_of(rng, one), one, [(0, 9, 9)], 1, "one tile of %d" % union)


def test_operator_picture_without_tiles_and_without_boxes(F):
    rng = np.random.default_rng(5)
    lists = [rand_list(rng, 40), rand_list(rng, 0), rand_list(rng, 0), rand_list(rng, 3)]
    recs = records_of(rng, lists)
    tiles = [(0, 10, 10), (2, 500, 500), (2, 0, 0), (-1, 0, 0)]                    # picture 1: no tiles; picture 2: tiles without boxes
    got_r, got_l = check_op(F, recs, lists, tiles, 3, "empty pictures")
    assert not got_r[1]["box"].tobytes().strip(b"\0") and int(got_r[1]["count"]) == int(got_r[1]["nfull"]) == int(got_r[1]["ncand"]) == int(got_r[1]["overflow"]) == 0
    assert int(got_r[2]["nfull"]) == 0 and int(got_r[2]["ncand"]) == int(recs[1]["ncand"]) + int(recs[2]["ncand"])
    assert not got_r[2]["box"].tobytes().strip(b"\0")


def test_operator_score_ties_across_tiles(F):
    """the same list under two origins (what identical pixels under two tiles give): far apart every box survives twice, in table order; 3
    pixels apart the earlier table entry's box wins every tie"""
    rng = np.random.default_rng(11)
    b = rand_list(rng, 60)
    recs = records_of(rng, [b, b, b])
    got_r, got_l = check_op(F, recs, [b, b, b], [(0, 3000, 0), (1, 0, 0), (0, 0, 3000)], 2, "ties, far")
    alone = got_l[1]
    assert len(got_l[0]) == 2 * len(alone) and np.array_equal(got_l[0]["score"][0::2], got_l[0]["score"][1::2])
    assert np.all(got_l[0]["x1"][0::2] > 2000) and np.all(got_l[0]["y1"][1::2] > 2000)                # table order within a tie
    got_r, got_l = check_op(F, recs, [b, b, b], [(0, 103, 100), (1, 0, 0), (0, 100, 100)], 2, "ties, near")
    first = mergeref.merge([b], [(103, 100)])
    assert len(got_l[0]) < 2 * len(alone) and got_l[0][0].tobytes() == first[0].tobytes()


def test_operator_records_own_boxes(F):
    """d_lists == NULL: a tile's boxes are box[0 .. count) of its record, whatever nfull says"""
    rng = np.random.default_rng(12)
    lists = [rand_list(rng, n) for n in (128, 300, 0, 17, 128)]
    recs = records_of(rng, lists)
    tiles = [(1, 20, 0), (0, 0, 0), (0, 7, 7), (1, 0, 30), (0, 4000, 4000)]
    check_op(F, recs, None, tiles, 2, "records' own boxes")
    check_op(F, recs, None, tiles, 2, "records' own boxes, IoU", use_min=0)


def test_operator_global_scratch_path(F):
    """a union one box over the LDS slots is merged in the scratch buffer and equals mergeref; without the buffer the same call fails, with
    a message, before anything is launched -- and a union that cannot exceed the slots needs no buffer"""
    import torch
    rng = np.random.default_rng(13)
    slots = F.FFGPU.MERGE_LDS_SLOTS
    sizes = (300, slots + 1 - 300 - 299, 299)
    lists = [rand_list(rng, n) for n in sizes]
    assert sum(len(b) for b in lists) == slots + 1
    recs = records_of(rng, lists)
    tiles = [(0, 0, 0), (0, 50, 20), (0, 10, 60)]
    check_op(F, recs, lists, tiles, 1, "scratch path")
    fits = [b[:-1] if k == 2 else b for k, b in enumerate(lists)]              # (their own records: a tile's nfull is its list's length)
    assert sum(len(b) for b in fits) == slots
    check_op(F, records_of(rng, fits), fits, tiles, 1, "exactly the LDS slots")
    out = torch.full((DETS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="scratch buffer"):
        run_op(F, recs, lists, tiles, 1, scratch=False)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    d_lists = torch.zeros(3 * 600 * BOX.itemsize, dtype=torch.uint8, device="cuda")
    assert F.lib().ffgpu_merge_tiles_dev(d_recs.data_ptr(), d_lists.data_ptr(), 600, F.tile_table(tiles), 3, 1, 0.5, 1, out.data_ptr(), None, None, 0, None) < 0
    assert "scratch buffer" in F.last_error() and "bytes" in F.last_error()
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy().tobytes()) == b"\xa5" * DETS.itemsize        # nothing was launched
    small = [rand_list(rng, n) for n in (300, 300, 300)]                       # 3 x 341 <= 1024 slots: no buffer needed
    check_op(F, records_of(rng, small), small, tiles, 1, "no scratch needed", stride=341, scratch=False)


def test_operator_properties(F):
    rng = np.random.default_rng(14)
    for n in (0, 5, 128, 129, 300):                                            # a single tile at (0, 0): its own record, byte for byte
        b = spread_list(rng, n)
        recs = records_of(rng, [b])
        got_r, got_l = run_op(F, recs, [b], [(0, 0, 0)], 1)
        want = recs[0].copy()
        want["overflow"] &= 5
        assert got_r[0].tobytes() == want.tobytes() and got_l[0].tobytes() == b.tobytes(), n
    lists = [rand_list(rng, 129), rand_list(rng, 80), rand_list(rng, 2)]
    recs = records_of(rng, lists)
    tiles = [(0, 0, 0), (0, 64, 64), (0, 20, 90)]
    once_r, once_l = check_op(F, recs, lists, tiles, 1, "once")
    twice_r, twice_l = check_op(F, recs[[0, 1, 2, 1, 0]], [lists[k] for k in (0, 1, 2, 1, 0)], [tiles[k] for k in (0, 1, 2, 1, 0)], 1, "tiles listed twice")
    assert twice_l[0].tobytes() == once_l[0].tobytes() and twice_r[0]["box"].tobytes() == once_r[0]["box"].tobytes()
    assert int(twice_r[0]["nfull"]) == int(once_r[0]["nfull"]) and int(twice_r[0]["count"]) == int(once_r[0]["count"])
    many = [spread_list(rng, 100), spread_list(rng, 100)]                      # merged nfull > 128: bit 2, count 128
    many[1]["type"] += 1000
    got_r, got_l = check_op(F, records_of(rng, many), many, [(0, 0, 0), (0, 5, 5)], 1, "overflow")
    assert int(got_r[0]["nfull"]) == 200 and int(got_r[0]["count"]) == 128 and int(got_r[0]["overflow"]) & 4


def test_operator_rejects(F):
    import torch
    rng = np.random.default_rng(15)
    lists = [rand_list(rng, 4) for _ in range(3)]
    recs = records_of(rng, lists)
    d = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.zeros(3 * DETS.itemsize, dtype=torch.uint8, device="cuda")
    L = F.lib()

    def call(tiles, ntiles=3, nimages=2, null_table=False):
        arr = F.tile_table(tiles)
        return L.ffgpu_merge_tiles_dev(d.data_ptr(), None, 0, None if null_table else arr, ntiles, nimages, 0.5, 1, out.data_ptr(), None, None, 0, None)
    good = [(0, 0, 0), (1, 5, 5), (-1, 0, 0)]
    for k, bad, msg in ((1, (2, 0, 0), "image"), (2, (-2, 0, 0), "image"), (0, (0, -1, 0), "negative origin"), (1, (1, 0, -7), "negative origin")):
        assert call(good[:k] + [bad] + good[k + 1:]) < 0
        assert "tile %d:" % k in F.last_error() and msg in F.last_error(), F.last_error()
    arr = F.tile_table(good)
    arr[2].reserved = 1
    assert call(arr) < 0 and "tile 2:" in F.last_error() and "reserved" in F.last_error()
    assert call(good, nimages=0) < 0 and "nimages" in F.last_error()
    assert call(good, nimages=4) < 0 and "nimages" in F.last_error()
    assert call(good, null_table=True) < 0 and "NULL" in F.last_error()
    assert call(good) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the real net
ORIGINS = [(0, 0), (640, 0), (0, 424), (640, 424)]


@pytest.fixture(scope="module")
def canvas(test_image):
    """1280 x 848 u8 BGR on the device: 2 x 2 copies of data/test.bmp (640 x 424); and the picture itself"""
    import torch
    bgr, w, h = test_image
    assert (w, h) == (640, 424)
    src = np.frombuffer(bgr, np.uint8).reshape(h, (3 * w + 3) & ~3)[:, :3 * w].reshape(h, w, 3)
    return torch.from_numpy(np.ascontiguousarray(np.tile(src, (2, 2, 1)))).cuda(), src


@pytest.fixture(scope="module")
def gold12():
    """the merged picture of the four copies: the golden boxes plus each origin, in the merge's order (score, then tile)"""
    gold = json.load(open(os.path.join(GOLD, "boxes.json")))["net_320x320_v0"]["boxes"]
    want = np.zeros(12, BOX)
    for k, g in enumerate(gold):
        assert 82 <= g["x1"] and g["x2"] <= 594 and 99 <= g["y1"] and g["y2"] <= 372      # no box crosses a copy
        for t, (x0, y0) in enumerate(ORIGINS):
            want[4 * k + t] = (g["type"], g["score"], g["x1"] + x0, g["y1"] + y0, g["x2"] + x0, g["y2"] + y0)
    return want


def mergeref_of(ex, tiles, nimages):
    """mergeref of the executor's own per-entry records and full lists"""
    dets = ex.read_dets()
    return mergeref.merge_table(dets, [ex.read_boxes(t) for t in range(len(tiles))], tiles, nimages)


def check_exec(ex, tiles, nimages, what):
    want_r, want_l = mergeref_of(ex, tiles, nimages)
    got = ex.read_merged(nimages)
    assert len(got) == nimages
    for g in range(nimages):
        assert got[g].tobytes() == want_r[g].tobytes(), "%s picture %d: record" % (what, g)
        assert ex.read_merged_boxes(g).tobytes() == want_l[g].tobytes(), "%s picture %d: full list" % (what, g)
    return got


@pytest.mark.parametrize("flags", [0, 32])
def test_net_batch4_four_copies(F, net, canvas, gold12, flags):
    """four 640 x 424 tiles at the copies' origins, one picture (flags 32: an FFGPU_SPLIT2 executor): the 12 golden boxes, and exactly
    mergeref of the four read_boxes lists; the per-entry records are what they were before the merge"""
    img, _ = canvas
    frames, tiles = F.tiles_of(img, [(x0, y0, 640, 424) for x0, y0 in ORIGINS])
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        before = ex.read_dets().tobytes()
        ex.merge_tiles(tiles, 1)
        got = check_exec(ex, tiles, 1, "flags %d" % flags)
        assert ex.read_dets().tobytes() == before
        assert int(got[0]["count"]) == int(got[0]["nfull"]) == 12 and int(got[0]["overflow"]) == 0
        boxes_match(ex.read_merged_boxes(0), gold12, "four copies, flags %d" % flags)
        ptr, nbytes = ex.merged_dev()
        assert ptr and nbytes == DETS.itemsize


def test_net_batch8(F, net, canvas, gold12):
    """batch 8: the four tiles each listed twice give the same 12 boxes; a 4-tile overlapped plan (the other four entries no tiles) and two
    pictures at once equal mergeref of their own lists"""
    img, _ = canvas
    frames, tiles = F.tiles_of(img, [(x0, y0, 640, 424) for x0, y0 in ORIGINS])
    with net.executor(8) as ex:
        ex.forward_bgr_frames_dev(frames + frames)
        ex.merge_tiles(tiles + tiles, 1)
        check_exec(ex, tiles + tiles, 1, "listed twice")
        boxes_match(ex.read_merged_boxes(0), gold12, "listed twice")
        ex.merge_tiles(tiles + [(1, x0, y0) for _, x0, y0 in tiles], 2)        # the same forward as two pictures
        got = check_exec(ex, tiles + [(1, x0, y0) for _, x0, y0 in tiles], 2, "two pictures")
        assert got[0].tobytes() == got[1].tobytes()
        plan = F.tile_plan(1280, 848, 800, 600, 200, 200, 1)
        assert len(plan) == 4
        pframes, ptiles = F.tiles_of(img, plan)
        ex.forward_bgr_frames_dev(pframes + frames)
        ptiles = ptiles + [(-1, 0, 0)] * 4
        ex.merge_tiles(ptiles, 1)
        check_exec(ex, ptiles, 1, "overlapped plan")


def test_net_batch8_nv12_tiles(F, net, canvas):
    """NV12 tiles of one surface (align 2: even origins keep the chroma phase), origins (0, 0) and (640, 424), against mergeref of their
    own per-tile lists"""
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    _, src = canvas
    Y, UV = bgr_to_nv12(np.ascontiguousarray(np.tile(src, (2, 2, 1))))
    dY, dUV = torch.from_numpy(Y).cuda(), torch.from_numpy(UV).cuda()
    plan = F.tile_plan(1280, 848, 640, 424, 0, 0, 2)
    assert [(p[0], p[1]) for p in plan] == ORIGINS
    two = [plan[0], plan[3]]
    frames = [(dY[y0:y0 + h, x0:x0 + w], dUV[y0 // 2:(y0 + h + 1) // 2, x0:x0 + 2 * ((w + 1) // 2)]) for x0, y0, w, h in two]
    tiles = [(0, x0, y0) for x0, y0, w, h in two] + [(-1, 0, 0)] * 6
    with net.executor(8) as ex:
        ex.forward_nv12_frames_dev(frames * 4)
        ex.merge_tiles(tiles, 1)
        got = check_exec(ex, tiles, 1, "nv12 tiles")
        assert int(got[0]["nfull"]) == len(ex.read_boxes(0)) + len(ex.read_boxes(1)) > 0      # the two tiles' boxes are 424 rows apart: all survive


def test_stream_order_and_reuse(F, net, canvas):
    """forward A, merge, forward B (other frames), merge, no sync between: the second result; the table is sent once (the second merge
    adds one launch), no graph is captured, the per-entry records are untouched"""
    import torch
    img, _ = canvas
    frames, tiles = F.tiles_of(img, [(x0, y0, 640, 424) for x0, y0 in ORIGINS])
    other = torch.flip(img, dims=(1,)).contiguous()                             # mirrored: other boxes
    oframes, _ = F.tiles_of(other, [(x0, y0, 640, 424) for x0, y0 in ORIGINS])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with net.executor(4) as ex:
        ex.forward_bgr_frames_dev(oframes, stream=st.cuda_stream)
        ex.merge_tiles(tiles, 1, stream=st.cuda_stream)
        want_b = check_exec(ex, tiles, 1, "B alone")[0].tobytes()
        ex.forward_bgr_frames_dev(frames, stream=st.cuda_stream)
        ex.merge_tiles(tiles, 1, stream=st.cuda_stream)
        want_a = check_exec(ex, tiles, 1, "A alone")[0].tobytes()
        assert want_a != want_b
        for _ in range(3):
            ex.forward_bgr_frames_dev(frames, stream=st.cuda_stream)
            ex.merge_tiles(tiles, 1, stream=st.cuda_stream)
            ex.forward_bgr_frames_dev(oframes, stream=st.cuda_stream)
            ex.merge_tiles(tiles, 1, stream=st.cuda_stream)
        assert ex.read_merged(1)[0].tobytes() == want_b
        check_exec(ex, tiles, 1, "A, merge, B, merge")
        assert ex.graph_captures == 1
        with pytest.raises(RuntimeError, match="stream of the forward"):
            ex.merge_tiles(tiles, 1)                                            # the executor's own stream is not the forward's


def test_exec_rejects(F, net, canvas):
    """every rejected argument, the entry's index in the message; the executor still runs a good call afterwards"""
    img, _ = canvas
    frames, tiles = F.tiles_of(img, [(x0, y0, 640, 424) for x0, y0 in ORIGINS])
    L = F.lib()
    with net.executor(4) as ex:
        with pytest.raises(RuntimeError, match="no ffgpu_exec_merge_tiles has run"):
            ex.read_merged(1)
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 1)
        good = ex.read_merged(1)[0].tobytes()
        for k, bad, msg in ((1, (1, 0, 0), "image"), (3, (-2, 0, 0), "image"), (0, (0, -1, 0), "negative origin"), (2, (0, 0, -1), "negative origin")):
            with pytest.raises(RuntimeError, match="tile %d: .*%s" % (k, msg)):
                ex.merge_tiles(tiles[:k] + [bad] + tiles[k + 1:], 1)
        arr = F.tile_table(tiles)
        arr[3].reserved = 9
        assert L.ffgpu_exec_merge_tiles(ex.h, arr, 4, 1, None) < 0 and "tile 3:" in F.last_error() and "reserved" in F.last_error()
        arr[3].reserved = 0
        assert L.ffgpu_exec_merge_tiles(ex.h, arr, 3, 1, None) < 0 and "tiles for an executor of batch" in F.last_error()
        assert L.ffgpu_exec_merge_tiles(ex.h, arr, 4, 0, None) < 0 and "nimages" in F.last_error()
        assert L.ffgpu_exec_merge_tiles(ex.h, arr, 4, 5, None) < 0 and "nimages" in F.last_error()
        assert L.ffgpu_exec_merge_tiles(ex.h, None, 4, 1, None) < 0 and "NULL" in F.last_error()
        assert L.ffgpu_exec_read_merged_boxes(ex.h, 1, None, 0) < 0
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 1)
        assert ex.read_merged(1)[0].tobytes() == good
