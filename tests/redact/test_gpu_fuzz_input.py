"""The detections redacted in the frames on the device: ffgpu_redact_boxes_bgr_dev / _nv12_dev (the operators, on synthetic records and lists) and
ffgpu_exec_redact_bgr / _nv12 (behind a forward or a merge of the real net) against tests/redact/redactref.py, the numpy restatement of the contract
in include/ffcnn_hip.h.  Every comparison is byte for byte over the WHOLE allocation: the targets lie in one arena of seeded random bytes with 64
guard bytes in front of and behind each, so a byte that should have stayed and did not is a failure like a wrong pixel.  No tolerance anywhere.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import re

import numpy as np
import pytest

from overlay import drawref
from overlay.test_gpu_fuzz_input import (Arena, bgr_arena, bgr_bytes, explain, fill_bgr, flat_lists, four_frames, picture,  # noqa: F401
                                         records_of, to_dev)
from redact import redactref
from redact.fuzzcases import check_stats, fuzz_cases, rand_boxes, targets_of
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX = redactref.BOX_DTYPE
Spec, FILL, MOSAIC = redactref.Spec, redactref.FILL, redactref.MOSAIC


def c_spec(F, sp):
    return F.redact_spec(sp.mode, sp.cell, sp.outside, sp.min_score, sp.classes, (sp.num, sp.den), sp.color)


def nv12_sizes(s):
    w, h, py, puv = s[:4]
    return py * (h - 1) + w, puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2)


def place(rng, nv12, specs):
    """the targets in one arena.  specs: BGR (w, h, pitch), NV12 (w, h, pitch_y, pitch_uv, separate uv plane), None: a skipped target.  Returns
    (arena, offsets, frames as capi takes them); offsets: BGR o, NV12 (oy, ouv)"""
    ar = Arena(rng)
    offs = []
    for s in specs:
        if s is None:
            offs.append(None)
        elif not nv12:
            offs.append(ar.alloc(bgr_bytes(*s), parity=1))
        else:
            ny, nuv = nv12_sizes(s)
            if s[4]:
                offs.append((ar.alloc(ny, parity=1), ar.alloc(nuv, parity=0)))
            else:                                                              # one surface: uv = y + pitch_y h, which must come out even
                oy = ar.alloc(s[2] * s[1] + nuv, parity=(s[2] * s[1]) & 1)
                offs.append((oy, oy + s[2] * s[1]))
    base = ar.upload()
    frames = []
    for s, o in zip(specs, offs):
        if s is None:
            frames.append(None)
        elif not nv12:
            frames.append((base + o, s[0], s[1], s[2]))
        else:
            frames.append((base + o[0], base + o[1] if s[4] else 0, s[0], s[1], s[2], s[3]))
    return ar, offs, frames


def reference(want, nv12, specs, offs, lists, sp, stats=None):
    """redactref on every target of the arena's bytes; returns the regions for explain"""
    regions = []
    for t, (s, o) in enumerate(zip(specs, offs)):
        if s is None:
            continue
        if nv12:
            redactref.redact_nv12(want, o[0], o[1], s[0], s[1], s[2], s[3], lists[t], sp, stats)
            ny, nuv = nv12_sizes(s)
            regions += [("target %d Y (%d x %d, %d boxes)" % (t, s[0], s[1], len(lists[t])), o[0], o[0] + ny), ("target %d UV" % t, o[1], o[1] + nuv)]
        else:
            redactref.redact_bgr(want, o, s[0], s[1], s[2], lists[t], sp, stats)
            regions.append(("target %d (%d x %d, pitch %d, %d boxes)" % (t, s[0], s[1], s[2], len(lists[t])), o, o + bgr_bytes(*s)))
    return regions


def run(F, rng, nv12, specs, lists, sp, what, stats=None, use_records=False, first_given=False):
    """redacts on the device and with redactref; compares the whole arena; returns the device's bytes"""
    ar, offs, frames = place(rng, nv12, specs)
    d_recs = to_dev(records_of(F, lists))
    stride = max(1, max(len(b) for b in lists)) + 3
    order = list(rng.permutation(len(lists))) if first_given else list(range(len(lists)))     # list t lies in slot order[t]
    slots = [None] * len(lists)
    for t, s in enumerate(order):
        slots[s] = lists[t]
    d_lists = None if use_records else to_dev(flat_lists(slots, stride))
    first = [int(s) * stride for s in order] if first_given else None
    fn = F.redact_boxes_nv12_dev if nv12 else F.redact_boxes_bgr_dev
    fn(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride, frames, c_spec(F, sp), first)
    got = ar.download()
    want = ar.start.copy()
    regions = reference(want, nv12, specs, offs, [b[:128] for b in lists] if use_records else lists, sp, stats)
    explain(got, want, regions, what)
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. the seeded fuzz
@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("mode", [FILL, MOSAIC])
@pytest.mark.parametrize("nv12", [False, True])
def test_operator_fuzz(F, nv12, mode, outside):
    """the seeded cases of tests/redact/fuzzcases.py: every size of SIZES as one target each per call, odd base addresses, row padding, lists of 0 to
    7 boxes with the degenerate boxes of the draw fuzz mixed in, one call per cell (FILL: as many calls with cell 0).  check_stats asserts the
    conditions that keep the fuzz from passing vacuously on redactref's statistics (tests/test_redact_abi.py: they hold on the reference alone)."""
    rng = np.random.default_rng(5300 + 4 * nv12 + 2 * mode + outside)
    total = {}
    for cell, specs, lists, sp in fuzz_cases(nv12, mode, outside):
        stats = {}
        run(F, rng, nv12, specs, lists, sp, "nv12 %s, mode %d, cell %d, outside %s" % (nv12, mode, cell, outside), stats)
        print("nv12 %s mode %d cell %d outside %s: %s" % (nv12, mode, cell, outside, stats))
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    check_stats(total, nv12, mode)


# ---------------------------------------------------------------------------------------------------------------- 2. counts, list starts, launches
@pytest.mark.parametrize("nv12", [False, True])
def test_operator_records_own_boxes(F, nv12):
    """d_lists == NULL: box[0 .. count) of each record, whatever nfull says; a list longer than the record keeps its first 128"""
    rng = np.random.default_rng(5240 + nv12)
    specs = targets_of(rng, nv12, [(64, 48), (40, 30), (70, 45), (33, 17)])
    lists = [rand_boxes(rng, n, s[0], s[1]) for n, s in zip((0, 5, 129, 300), specs)]
    run(F, rng, nv12, specs, lists, Spec(MOSAIC, 4, False, 0.2), "records' own boxes", use_records=True)
    run(F, rng, nv12, specs, lists, Spec(FILL, 0, True, 0.2, color=(1, 2, 3)), "records' own boxes, outside", use_records=True)


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_list_first_and_a_skipped_target(F, nv12):
    """the lists in scattered slots named by list_first, against the uniform stride of a NULL list_first; a NULL-address target in the middle stays
    untouched"""
    rng = np.random.default_rng(5242 + nv12)
    specs = targets_of(rng, nv12, [(64, 48), (7, 5), (150, 140), (13, 9), (1, 1)])
    specs[1] = specs[3] = None
    lists = [rand_boxes(rng, n, 64, 48) for n in (7, 5, 6, 3, 1)]
    for outside in (False, True):
        run(F, rng, nv12, specs, lists, Spec(MOSAIC, 6, outside, 0.1), "list_first given", first_given=True)
        run(F, rng, nv12, specs, lists, Spec(MOSAIC, 6, outside, 0.1), "list_first NULL")


def test_operator_counts_are_clamped(F):
    """records whose count / nfull is negative or beyond the stride redact by the clamped number of boxes and touch nothing else"""
    rng = np.random.default_rng(5244)
    w, h, pitch, stride = 40, 30, 131, 9
    sp = Spec(MOSAIC, 5, False, 0.0)
    for use_records in (False, True):
        cap = 128 if use_records else stride
        lists = [rand_boxes(rng, cap, w, h) for _ in range(4)]
        for b in lists:                                                            # (small boxes: 128 of them must not cover everything)
            b["x2"], b["y2"] = np.minimum(b["x2"], b["x1"] + 3), np.minimum(b["y2"], b["y1"] + 2)
        recs = records_of(F, lists)
        claimed = (-1, -2 ** 31, cap + 1, 2 ** 31 - 1)
        for t, c in enumerate(claimed):
            recs[t]["count" if use_records else "nfull"] = c
            recs[t]["nfull" if use_records else "count"] = 2                     # (the other field is not the one that is read)
        specs = [(w, h, pitch)] * 4
        ar, offs, frames = place(rng, False, specs)
        d_recs = to_dev(recs)
        d_lists = None if use_records else to_dev(flat_lists(lists, stride))
        F.redact_boxes_bgr_dev(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride, frames, c_spec(F, sp))
        got = ar.download()
        want = ar.start.copy()
        regions = reference(want, False, specs, offs, [b[:0] if c < 0 else b for b, c in zip(lists, claimed)], sp)
        explain(got, want, regions, "clamped counts, records %s" % use_records)
        assert want.tobytes() != ar.start.tobytes()
        assert d_recs.cpu().numpy().tobytes() == recs.tobytes()


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_a_list_past_the_staging_chunk(F, nv12):
    """300 boxes on a 40 x 30 target: the list is staged 256 boxes at a time; small boxes, so covered and uncovered pixels both remain"""
    rng = np.random.default_rng(5246 + nv12)
    specs = targets_of(rng, nv12, [(40, 30)])
    b = rand_boxes(rng, 300, 40, 30)
    b["x2"], b["y2"] = np.minimum(b["x2"], b["x1"] + 2), np.minimum(b["y2"], b["y1"] + 2)
    only_late = b.copy()
    only_late["score"][:256] = 0.0                                                 # only the boxes of the second trip qualify
    for boxes in (b, only_late):
        for sp in (Spec(MOSAIC, 4, False, 0.3), Spec(FILL, 0, True, 0.3, color=(200, 100, 50))):
            stats = {}
            run(F, rng, nv12, specs, [boxes], sp, "300 boxes", stats)
            assert 0 < stats["covered"] < stats["pixels"] and stats["qualifying"] > 0, stats


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_more_targets_than_one_launch(F, nv12):
    """65 tiny targets of different sizes in one call (a launch's arguments hold 64), the grid sized by the largest of each launch: the one target of
    several blocks is the last of the first launch, the second launch holds a single small one"""
    rng = np.random.default_rng(5248 + nv12)
    sizes = [(1 + (t * 7) % 23, 1 + (t * 5) % 17) for t in range(65)]
    sizes[63] = (130, 70)
    specs = targets_of(rng, nv12, sizes)
    lists = [rand_boxes(rng, int(rng.integers(0, 6)), s[0], s[1]) for s in specs]
    for sp in (Spec(MOSAIC, 2, False, 0.1), Spec(MOSAIC, 64, True, 0.1), Spec(FILL, 0, False, 0.1, color=(5, 6, 7))):
        run(F, rng, nv12, specs, lists, sp, "65 targets", first_given=True)


def test_operator_nv12_odd_sizes(F):
    """odd w and h: the last column and row of luma have half-empty chroma samples; a box on the last pixel alone, OUTSIDE of nothing"""
    rng = np.random.default_rng(5250)
    specs = targets_of(rng, True, [(63, 47), (65, 65), (1, 1), (3, 1), (1, 3), (129, 5)])
    corner = []
    for s in specs:
        b = np.zeros(2, BOX)
        b[0] = (0, 0.9, s[0] - 1, s[1] - 1, s[0] - 1, s[1] - 1)
        b[1] = (0, 0.9, 0, 0, 0, 0)
        corner.append(b)
    for sp in (Spec(FILL, 0, False, 0.5, color=(9, 99, 199)), Spec(MOSAIC, 2, False, 0.5), Spec(MOSAIC, 64, False, 0.5), Spec(MOSAIC, 6, True, 0.5)):
        stats = {}
        run(F, rng, True, specs, corner, sp, "nv12 odd sizes, corners", stats)
        assert stats["chroma_mixed"] > 0
        run(F, rng, True, specs, [rand_boxes(rng, 4, s[0], s[1]) for s in specs], sp, "nv12 odd sizes")
    run(F, rng, True, specs, [b[:0] for b in corner], Spec(MOSAIC, 4, True), "nv12 odd sizes, an empty list with OUTSIDE")


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_nan_scores(F, nv12):
    """a NaN score never qualifies and a NaN min_score lets nothing qualify: without OUTSIDE nothing is written, with it the whole target"""
    rng = np.random.default_rng(5251 + nv12)
    specs = targets_of(rng, nv12, [(70, 45), (13, 9)])
    lists = [rand_boxes(rng, 6, s[0], s[1]) for s in specs]
    for b in lists:
        b["score"][::2] = float("nan")
    for min_score in (0.0, float("nan")):
        for outside in (False, True):
            stats = {}
            run(F, rng, nv12, specs, lists, Spec(MOSAIC, 4, outside, min_score), "NaN scores, min_score %s" % min_score, stats)
            assert stats["rejected_score"] == (12 if min_score != min_score else 6), stats
            if min_score != min_score:
                assert stats["covered"] == (stats["pixels"] if outside else 0), stats


def test_same_call_twice_gives_the_same_bytes(F):
    """the same call on two fresh copies of the same start bytes: identical bytes (and both equal redactref)"""
    for nv12 in (False, True):
        outs = []
        for _ in range(2):
            rng = np.random.default_rng(5252)
            specs = targets_of(rng, nv12, [(150, 140), (64, 48)])
            lists = [rand_boxes(rng, 7, 150, 140), rand_boxes(rng, 7, 30, 30)]
            outs.append(run(F, rng, nv12, specs, lists, Spec(MOSAIC, 6, False, 0.1, None, (1, 2)), "run twice").tobytes())
        assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------------------------- the real net
def nv12_arena(rng, imgs):
    """the pictures as NV12 surfaces in one arena; returns (arena, [(oy, ouv, w, h, py, puv)], frames)"""
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    ar = Arena(rng)
    where = []
    for im in imgs:
        h, w = im.shape[:2]
        py, puv = w + 3, 2 * ((w + 1) // 2) + 4
        where.append((ar.alloc(py * (h - 1) + w, parity=1), ar.alloc(puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2), parity=0), w, h, py, puv))
    base = ar.upload()
    for (oy, ouv, w, h, py, puv), im in zip(where, imgs):
        Y, UV = bgr_to_nv12(im)
        np.lib.stride_tricks.as_strided(ar.start[oy:], shape=(h, w), strides=(py, 1), writeable=True)[...] = Y
        np.lib.stride_tricks.as_strided(ar.start[ouv:], shape=UV.shape, strides=(puv, 1), writeable=True)[...] = UV
    ar.dev.copy_(torch.from_numpy(ar.start))
    return ar, where, [(base + oy, base + ouv, w, h, py, puv) for oy, ouv, w, h, py, puv in where]


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_redact_entries_bgr(F, net, picture, flags):
    """batch 4 (flags 32: FFGPU_SPLIT2): the very array handed to the forward is redacted frame by frame, MOSAIC 8; the records, the full lists and
    the one captured graph are what they were"""
    rng = np.random.default_rng(5260)
    imgs = four_frames(picture)
    ar, where = bgr_arena(rng, imgs)
    base = ar.upload()
    fill_bgr(ar, where, imgs)
    frames = [(base + o, w, h, p) for o, w, h, p in where]
    sp = Spec(MOSAIC, 8, False, 0.0, None, (1, 8))
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)], ex.graph_captures
        assert caps == 1 and all(len(b) > 0 for b in boxes)
        ex.redact_bgr(frames, c_spec(F, sp), F.REDACT_ENTRIES)
        got = ar.download()
        want = ar.start.copy()
        stats = {}
        for (o, w, h, p), b in zip(where, boxes):
            redactref.redact_bgr(want, o, w, h, p, b, sp, stats)
        explain(got, want, [("frame %d" % t, o, o + bgr_bytes(w, h, p)) for t, (o, w, h, p) in enumerate(where)], "exec entries, flags %d" % flags)
        assert got.tobytes() != ar.start.tobytes() and stats["cells_partial"] > 0 and stats["cells_full"] > 0
        assert ex.read_dets().tobytes() == dets and ex.graph_captures == 1
        assert all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(4))


def test_exec_redact_entries_nv12(F, net, picture):
    rng = np.random.default_rng(5261)
    ar, where, frames = nv12_arena(rng, four_frames(picture))
    sp = Spec(MOSAIC, 8, False, 0.0)
    with net.executor(4) as ex:
        ex.forward_nv12_frames_dev(frames)
        dets, boxes = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)]
        assert sum(len(b) for b in boxes) > 0
        ex.redact_nv12(frames, c_spec(F, sp), F.REDACT_ENTRIES)
        got = ar.download()
        want = ar.start.copy()
        for (oy, ouv, w, h, py, puv), b in zip(where, boxes):
            redactref.redact_nv12(want, oy, ouv, w, h, py, puv, b, sp)
        explain(got, want, [("frame %d Y" % t, x[0], x[0] + x[4] * (x[3] - 1) + x[2]) for t, x in enumerate(where)], "exec entries, nv12")
        assert got.tobytes() != ar.start.tobytes()
        assert ex.read_dets().tobytes() == dets and ex.graph_captures == 1


def test_exec_redact_merged_then_draw(F, net, picture):
    """2 pictures x 2 tiles: plan, forward, merge, redact the merged lists in the two pictures (everything BUT the boxes filled), then draw them:
    redactref followed by drawref -- the outlines lie on top; the merged records stay what they were"""
    rng = np.random.default_rng(5262)
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    pics = [wide, np.ascontiguousarray(wide[::-1])]
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    assert len(plan) == 2
    ar, where = bgr_arena(rng, pics, pad=7)
    base = ar.upload()
    fill_bgr(ar, where, pics)
    frames, tiles = [], []
    for g, (o, w, h, p) in enumerate(where):
        for x0, y0, tw, th in plan:
            frames.append((base + o + y0 * p + 3 * x0, tw, th, p))
            tiles.append((g, x0, y0))
    whole = [(base + o, w, h, p) for o, w, h, p in where]
    sp = Spec(FILL, 0, True, 0.0, None, (1, 4), (30, 30, 30))
    with net.executor(4) as ex:
        with pytest.raises(RuntimeError, match="no ffgpu_exec_merge_tiles has run"):
            ex.redact_bgr(whole, c_spec(F, sp), F.REDACT_MERGED)
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 2)
        merged, lists = ex.read_merged(2).tobytes(), [ex.read_merged_boxes(g) for g in range(2)]
        assert all(len(b) > 0 for b in lists)
        ex.redact_bgr(whole, c_spec(F, sp), F.REDACT_MERGED)
        ex.draw_bgr(whole, F.DRAW_MERGED, color=(255, 0, 255), thickness=2)
        got = ar.download()
        want = ar.start.copy()
        for (o, w, h, p), b in zip(where, lists):
            redactref.redact_bgr(want, o, w, h, p, b, sp)
        only_redacted = want.copy()
        for (o, w, h, p), b in zip(where, lists):
            drawref.draw_bgr(want, o, w, h, p, b, drawref.colours_of(b, (255, 0, 255)), 2)
        explain(got, want, [("picture %d" % g, o, o + bgr_bytes(w, h, p)) for g, (o, w, h, p) in enumerate(where)], "exec merged, then draw")
        assert want.tobytes() != only_redacted.tobytes() != ar.start.tobytes()
        assert ex.read_merged(2).tobytes() == merged and ex.graph_captures == 1


def test_rejections(F, net, picture):
    """every rejected argument with its message, the target's index where there is one; nothing is written by a rejected call, and the next valid
    call on the same executor equals redactref"""
    import ctypes as C
    import torch
    rng = np.random.default_rng(5270)
    imgs = four_frames(picture)
    ar, where = bgr_arena(rng, imgs)
    base = ar.upload()
    fill_bgr(ar, where, imgs)
    frames = [(base + o, w, h, p) for o, w, h, p in where]
    L = F.lib()
    good = F.redact_spec(F.REDACT_MOSAIC, 8)
    cls = (C.c_ubyte * 8)()

    def spec(mode=1, cell=8, flags=0, nclasses=0, classes=False, margin=(0, 1)):
        s = F.RedactSpec()
        s.mode, s.cell, s.flags, s.nclasses, s.classes = mode, cell, flags, nclasses, (C.addressof(cls) if classes else None)
        s.margin_num, s.margin_den = margin
        return s
    with net.executor(4) as ex:
        ex.forward_bgr_frames_dev(frames)
        boxes = [ex.read_boxes(t) for t in range(4)]
        tab = F.bgr_frame_table(frames)
        nv = F.nv12_frame_table([(base + where[t][0] + 1, 0, 64, 48) for t in range(4)])     # (an even address: a valid 64 x 48 surface inside frame t)
        d_recs, _ = ex.dets_dev()

        def both(args, msg, nv12_too=True, bgr_too=True):
            """the executor form and the operator, BGR (and NV12 with the same spec / counts)"""
            which, t, n, s = args
            calls = []
            if bgr_too:
                calls.append(lambda: L.ffgpu_exec_redact_bgr(ex.h, which, t, n, s, None))
                if which == 0:
                    calls.append(lambda: L.ffgpu_redact_boxes_bgr_dev(d_recs, None, 0, None, t, n, s, None))
            if nv12_too:
                calls.append(lambda: L.ffgpu_exec_redact_nv12(ex.h, which, None if t is None else nv, n, s, None))
                if which == 0:
                    calls.append(lambda: L.ffgpu_redact_boxes_nv12_dev(d_recs, None, 0, None, None if t is None else nv, n, s, None))
            for c in calls:
                assert c() < 0
                assert re.search(msg, F.last_error()), (msg, F.last_error())
        both((0, None, 4, good), "NULL targets")
        both((0, tab, 4, None), "NULL spec")
        both((0, tab, 4, spec(mode=2)), "mode 2")
        both((0, tab, 4, spec(mode=-1)), "mode -1")
        both((0, tab, 4, spec(flags=2)), "unknown flags 0x2")
        both((0, tab, 4, spec(flags=-1)), "unknown flags")
        both((0, tab, 4, spec(cell=1)), "cell 1 ")
        both((0, tab, 4, spec(cell=0)), "cell 0 ")
        both((0, tab, 4, spec(cell=65)), "cell 65 ")
        both((0, tab, 4, spec(cell=66)), "cell 66 ")
        both((0, tab, 4, spec(mode=0, cell=2)), "cell 2 ")
        both((0, tab, 4, spec(cell=7)), "cell 7 is odd", bgr_too=False)
        both((0, tab, 4, spec(classes=True, nclasses=0)), "nclasses 0")
        both((0, tab, 4, spec(classes=True, nclasses=257)), "nclasses 257")
        both((0, tab, 4, spec(classes=False, nclasses=2)), "nclasses 2")
        both((0, tab, 4, spec(margin=(1, 0))), "margin 1 / 0")
        both((0, tab, 4, spec(margin=(-1, 4))), "margin -1 / 4")
        both((0, tab, 4, spec(margin=(17, 4))), "margin 17 / 4")
        both((0, tab, 4, spec(margin=(1, 1025))), "margin 1 / 1025")
        both((2, tab, 4, good), "which = 2")
        both((-1, tab, 4, good), "which = -1")
        both((1, tab, 4, good), "no ffgpu_exec_merge_tiles has run")
        assert L.ffgpu_exec_redact_bgr(ex.h, 0, tab, 3, good, None) < 0 and "3 targets for an executor of batch 4" in F.last_error()
        assert L.ffgpu_exec_redact_nv12(ex.h, 0, nv, 5, good, None) < 0 and "5 targets for an executor of batch 4" in F.last_error()
        assert L.ffgpu_redact_boxes_bgr_dev(d_recs, None, 0, None, tab, 0, good, None) < 0 and "ntargets" in F.last_error()
        assert L.ffgpu_redact_boxes_bgr_dev(None, None, 0, None, tab, 4, good, None) < 0 and "NULL records" in F.last_error()
        assert L.ffgpu_redact_boxes_bgr_dev(d_recs, d_recs, 0, None, tab, 4, good, None) < 0 and "list_stride" in F.last_error()
        first = (C.c_int * 4)(0, 0, -5, 0)
        assert L.ffgpu_redact_boxes_bgr_dev(d_recs, d_recs, 8, first, tab, 4, good, None) < 0 and "target 2: negative list start" in F.last_error()
        st = torch.cuda.Stream()
        assert L.ffgpu_exec_redact_bgr(ex.h, 0, tab, 4, good, st.cuda_stream) < 0 and "stream of the forward" in F.last_error()
        for k, field, val, msg in ((1, "w", 0, "bad size"), (2, "h", -3, "bad size"), (3, "reserved", 1, "reserved"), (0, "pitch", 5, "pitch")):
            bad = F.bgr_frame_table(frames)
            setattr(bad[k], field, val)
            both((0, bad, 4, good), "target %d: .*%s" % (k, msg), nv12_too=False)
        for k, field, val, msg in ((1, "w", 0, "bad size"), (2, "matrix", 4, "matrix"), (3, "reserved", 1, "reserved"), (0, "pitch_y", 5, "pitch_y"),
                                   (2, "pitch_uv", 63, "pitch_uv"), (1, "uv", base + 1, "odd")):
            bad = F.nv12_frame_table([(base + where[t][0] + 1, 0, 64, 48) for t in range(4)])
            setattr(bad[k], field, val)
            assert L.ffgpu_exec_redact_nv12(ex.h, 0, bad, 4, good, None) < 0
            assert re.search("target %d: .*%s" % (k, msg), F.last_error()), F.last_error()
            assert L.ffgpu_redact_boxes_nv12_dev(d_recs, None, 0, None, bad, 4, good, None) < 0
            assert re.search("target %d: .*%s" % (k, msg), F.last_error()), F.last_error()
        huge = F.nv12_frame_table([(base + where[t][0] + 1, 0, 64, 48) for t in range(4)])       # 2^24 x 2^24 blocks of 64 x 64: never launched
        huge[3].w = huge[3].h = (1 << 30) - 1
        huge[3].pitch_y = huge[3].pitch_uv = 1 << 30
        assert L.ffgpu_exec_redact_nv12(ex.h, 0, huge, 4, good, None) < 0 and re.search("target 3: .*more than 2\\^23 blocks", F.last_error()), F.last_error()
        assert ar.download().tobytes() == ar.start.tobytes()                    # nothing was launched
        sp = Spec(MOSAIC, 8)
        ex.redact_bgr(frames[:2] + [None] + frames[3:], c_spec(F, sp))          # the executor is still usable; a NULL address is a skipped target
        got = ar.download()
        want = ar.start.copy()
        for t, ((o, w, h, p), b) in enumerate(zip(where, boxes)):
            if t != 2:
                redactref.redact_bgr(want, o, w, h, p, b, sp)
        explain(got, want, [("frame %d" % t, o, o + bgr_bytes(w, h, p)) for t, (o, w, h, p) in enumerate(where)], "after the rejections")
        assert got.tobytes() != ar.start.tobytes()
