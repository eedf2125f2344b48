"""The detections blurred in the frames on the device: ffgpu_blur_boxes_bgr_dev / _nv12_dev (the operators, on synthetic records and lists) and
ffgpu_exec_blur_bgr / _nv12 (behind a forward or a merge of the real net) against tests/blur/blurref.py, the numpy restatement of the contract in
include/ffcnn_hip.h.  Every comparison is byte for byte over the WHOLE allocation: the targets AND their scratch surfaces lie in one arena of seeded
random bytes with 64 guard bytes in front of and behind each, so a byte that should have stayed and did not -- in a target, in a scratch surface,
in the padding of a row -- is a failure like a wrong pixel.  No tolerance anywhere.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import re

import numpy as np
import pytest

from blur import blurref, fuzzcases
from blur.fuzzcases import border_boxes, check_stats, fuzz_cases, image_of, nv12_sizes, scratch_of, write_image
from overlay import drawref
from overlay.test_gpu_fuzz_input import (Arena, bgr_arena, bgr_bytes, explain, fill_bgr, flat_lists, four_frames, picture,  # noqa: F401
                                         records_of, to_dev)
from redact import redactref
from redact.fuzzcases import rand_boxes, targets_of
from redact.test_gpu_fuzz_input import place
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX = blurref.BOX_DTYPE
Spec = blurref.Spec


def c_spec(F, sp):
    return F.blur_spec(sp.radius, sp.passes, sp.outside, sp.min_score, sp.classes, (sp.num, sp.den))


def regions_of(nv12, specs, sspecs, offs, soffs):
    out = []
    for kind, ss, oo in (("target", specs, offs), ("scratch", sspecs, soffs)):
        for t, (s, o) in enumerate(zip(ss, oo)):
            if s is None:
                continue
            if nv12:
                ny, nuv = nv12_sizes(s)
                out += [("%s %d Y (%d x %d)" % (kind, t, s[0], s[1]), o[0], o[0] + ny), ("%s %d UV" % (kind, t), o[1], o[1] + nuv)]
            else:
                out.append(("%s %d (%d x %d, pitch %d)" % (kind, t, s[0], s[1], s[2]), o, o + bgr_bytes(*s)))
    return out


def run(F, rng, nv12, specs, lists, sp, what, images=None, stats=None, use_records=False, first_given=False, calls=1, sspecs=None, after=None):
    """blurs on the device and with blurref (`calls` times each); compares the whole arena, targets and scratch; returns the device's bytes.
    after(ar, frames, want, offs): further device calls on the same frames and their reference, before the comparison"""
    import torch
    n = len(specs)
    sspecs = scratch_of(specs, nv12) if sspecs is None else sspecs
    ar, offs, frames = place(rng, nv12, list(specs) + list(sspecs))
    if images is not None:
        for s, o, img in zip(specs, offs[:n], images):
            if s is not None and img is not None:
                write_image(ar.start, nv12, s, o, img)
        ar.dev.copy_(torch.from_numpy(ar.start))
    d_recs = to_dev(records_of(F, lists))
    stride = max(1, max(len(b) for b in lists)) + 3
    order = list(rng.permutation(len(lists))) if first_given else list(range(len(lists)))     # list t lies in slot order[t]
    slots = [None] * len(lists)
    for t, s in enumerate(order):
        slots[s] = lists[t]
    d_lists = None if use_records else to_dev(flat_lists(slots, stride))
    first = [int(s) * stride for s in order] if first_given else None
    fn = F.blur_boxes_nv12_dev if nv12 else F.blur_boxes_bgr_dev
    for _ in range(calls):
        fn(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride, frames[:n], frames[n:], c_spec(F, sp), first)
    want = ar.start.copy()
    ref_lists = [b[:128] for b in lists] if use_records else lists
    for _ in range(calls):
        fuzzcases.reference(want, nv12, specs, sspecs, offs[:n], offs[n:], ref_lists, sp, stats)
    if after is not None:
        after(d_recs, d_lists, stride, frames[:n], want, offs[:n])
    got = ar.download()
    explain(got, want, regions_of(nv12, specs, sspecs, offs[:n], offs[n:]), what)
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. the seeded fuzz
@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("nv12", [False, True])
def test_operator_fuzz(F, nv12, outside):
    """the seeded cases of tests/blur/fuzzcases.py: every size of SIZES as one target each per call (1 x 1 to 150 x 140, 63 to 66 wide and high, odd
    NV12 sizes), odd base addresses, row padding, a scratch pitch that differs from the target's, radii 1, 2, 7, 16, 31 with 1 to 3 passes, lists of
    0 to 7 boxes with the degenerate boxes of the draw fuzz and boxes on the block borders mixed in, half of the frames steps and ramps.
    check_stats asserts the conditions that keep the fuzz from passing vacuously (tests/test_blur_abi.py: they hold on the reference alone)."""
    rng = np.random.default_rng(5440 + 2 * nv12 + outside)
    cases = fuzz_cases(nv12, outside)
    per_target = []
    for c in cases:
        run(F, rng, nv12, c["specs"], c["lists"], c["spec"], "nv12 %s, radius %d, passes %d, outside %s" % (nv12, c["radius"], c["passes"], outside),
            images=c["images"], stats=per_target, sspecs=c["sspecs"])
    check_stats(cases, per_target, outside)


# ---------------------------------------------------------------------------------------------------------------- 2. counts, list starts, launches
@pytest.mark.parametrize("nv12", [False, True])
def test_operator_records_own_boxes(F, nv12):
    """d_lists == NULL: box[0 .. count) of each record, whatever nfull says; a list longer than the record keeps its first 128"""
    rng = np.random.default_rng(5450 + nv12)
    specs = targets_of(rng, nv12, [(64, 48), (40, 30), (70, 45), (33, 17)])
    lists = [rand_boxes(rng, n, s[0], s[1]) for n, s in zip((0, 5, 129, 300), specs)]
    for b in lists[2:]:
        b["x2"], b["y2"] = np.minimum(b["x2"], b["x1"] + 3), np.minimum(b["y2"], b["y1"] + 2)
    run(F, rng, nv12, specs, lists, Spec(2, 1, False, 0.2), "records' own boxes", use_records=True)
    run(F, rng, nv12, specs, lists, Spec(7, 2, True, 0.2), "records' own boxes, outside", use_records=True)


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_list_first_and_a_skipped_target(F, nv12):
    """the lists in scattered slots named by list_first, against the uniform stride of a NULL list_first; a NULL-address target (and scratch) in the
    middle stays untouched"""
    rng = np.random.default_rng(5452 + nv12)
    specs = targets_of(rng, nv12, [(64, 48), (7, 5), (150, 140), (13, 9), (1, 1)])
    specs[1] = specs[3] = None
    lists = [rand_boxes(rng, n, 64, 48) for n in (7, 5, 6, 3, 1)]
    for outside in (False, True):
        run(F, rng, nv12, specs, lists, Spec(16, 1, outside, 0.1), "list_first given", first_given=True)
        run(F, rng, nv12, specs, lists, Spec(3, 2, outside, 0.1), "list_first NULL")


def test_operator_counts_are_clamped(F):
    """records whose count / nfull is negative or beyond the stride blur by the clamped number of boxes and touch nothing else"""
    rng = np.random.default_rng(5454)
    w, h, pitch, stride = 40, 30, 131, 9
    sp = Spec(2, 1, False, 0.0)
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
        sspecs = scratch_of(specs, False)
        ar, offs, frames = place(rng, False, specs + sspecs)
        d_recs = to_dev(recs)
        d_lists = None if use_records else to_dev(flat_lists(lists, stride))
        F.blur_boxes_bgr_dev(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride, frames[:4], frames[4:], c_spec(F, sp))
        got = ar.download()
        want = ar.start.copy()
        fuzzcases.reference(want, False, specs, sspecs, offs[:4], offs[4:], [b[:0] if c < 0 else b for b, c in zip(lists, claimed)], sp)
        explain(got, want, regions_of(False, specs, sspecs, offs[:4], offs[4:]), "clamped counts, records %s" % use_records)
        assert want.tobytes() != ar.start.tobytes()
        assert d_recs.cpu().numpy().tobytes() == recs.tobytes()


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_a_list_past_the_staging_chunk(F, nv12):
    """300 boxes on a 40 x 30 target: the list is staged 256 boxes at a time; small boxes, so covered and uncovered pixels both remain"""
    rng = np.random.default_rng(5456 + nv12)
    specs = targets_of(rng, nv12, [(40, 30)])
    b = rand_boxes(rng, 300, 40, 30)
    b["x2"], b["y2"] = np.minimum(b["x2"], b["x1"] + 2), np.minimum(b["y2"], b["y1"] + 2)
    only_late = b.copy()
    only_late["score"][:256] = 0.0                                                 # only the boxes of the second trip qualify
    for boxes in (b, only_late):
        for sp in (Spec(2, 1, False, 0.3), Spec(31, 1, True, 0.3)):
            stats = []
            run(F, rng, nv12, specs, [boxes], sp, "300 boxes", stats=stats)
            assert 0 < stats[0]["covered"] < stats[0]["pixels"] and stats[0]["qualifying"] > 0, stats


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_more_targets_than_one_launch(F, nv12):
    """65 tiny targets of different sizes in one call (a launch's arguments hold 64 BGR or 48 NV12 targets), the grid sized by the largest of each
    group: the one target of several blocks is the last of a group, the last group holds small ones only"""
    rng = np.random.default_rng(5458 + nv12)
    sizes = [(1 + (t * 7) % 23, 1 + (t * 5) % 17) for t in range(65)]
    sizes[47 if nv12 else 63] = (130, 70)
    specs = targets_of(rng, nv12, sizes)
    lists = [rand_boxes(rng, int(rng.integers(0, 6)), s[0], s[1]) for s in specs]
    for sp in (Spec(1, 3, False, 0.1), Spec(31, 1, True, 0.1)):
        run(F, rng, nv12, specs, lists, sp, "65 targets", first_given=True)


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_nan_scores(F, nv12):
    """a NaN score never qualifies and a NaN min_score lets nothing qualify: without OUTSIDE nothing is written, with it the whole target"""
    rng = np.random.default_rng(5460 + nv12)
    specs = targets_of(rng, nv12, [(70, 45), (13, 9)])
    lists = [rand_boxes(rng, 6, s[0], s[1]) for s in specs]
    for b in lists:
        b["score"][::2] = float("nan")
    for min_score in (0.0, float("nan")):
        for outside in (False, True):
            stats = []
            run(F, rng, nv12, specs, lists, Spec(7, 1, outside, min_score), "NaN scores, min_score %s" % min_score, stats=stats)
            assert sum(st["rejected_score"] for st in stats) == (12 if min_score != min_score else 6), stats
            if min_score != min_score:
                assert all(st["covered"] == (st["pixels"] if outside else 0) for st in stats), stats


def test_same_call_twice(F):
    """the same call twice on the same surfaces is the reference applied twice (the second call reads what the first left, scratch included), and
    the same two calls on fresh copies of the same start bytes give identical bytes"""
    for nv12 in (False, True):
        outs = []
        for _ in range(2):
            rng = np.random.default_rng(5462)
            specs = targets_of(rng, nv12, [(150, 140), (64, 48)])
            lists = [np.concatenate([border_boxes(150, 140)[:3], rand_boxes(rng, 4, 150, 140)]), rand_boxes(rng, 7, 30, 30)]
            images = [image_of(rng, s[0], s[1], nv12, True) for s in specs]
            outs.append(run(F, rng, nv12, specs, lists, Spec(16, 2, False, 0.1, None, (1, 2)), "run twice", images=images, calls=2).tobytes())
        assert outs[0] == outs[1]


def test_blur_then_mosaic_then_draw(F):
    """a 1-pass blur followed by a redact MOSAIC and a draw on the same frames: blurref, redactref, drawref in that order"""
    rng = np.random.default_rng(5464)
    specs = targets_of(rng, False, [(150, 140), (70, 45)])
    lists = [rand_boxes(rng, 6, s[0], s[1]) for s in specs]
    blurred = {}

    def after(d_recs, d_lists, stride, frames, want, offs):
        blurred["bytes"] = want.tobytes()
        rsp = redactref.Spec(redactref.MOSAIC, 8, False, 0.5)
        F.redact_boxes_bgr_dev(d_recs.data_ptr(), d_lists.data_ptr(), stride, frames, F.redact_spec(F.REDACT_MOSAIC, 8, False, 0.5))
        F.draw_boxes_bgr_dev(d_recs.data_ptr(), d_lists.data_ptr(), stride, frames, F.draw_style(color=(0, 255, 0), thickness=1))
        for s, o, b in zip(specs, offs, lists):
            redactref.redact_bgr(want, o, s[0], s[1], s[2], b, rsp)
        blurred["mosaic"] = want.tobytes()
        for s, o, b in zip(specs, offs, lists):
            drawref.draw_bgr(want, o, s[0], s[1], s[2], b, drawref.colours_of(b, (0, 255, 0)), 1)
        assert blurred["bytes"] != blurred["mosaic"] != want.tobytes()
    run(F, rng, False, specs, lists, Spec(7, 1, False, 0.1, None, (1, 4)), "blur, mosaic, draw", after=after)


# ---------------------------------------------------------------------------------------------------------------- the real net
def with_scratch(ar, where):
    """scratch surfaces for the BGR pictures of an arena that is not uploaded yet: [(offset, w, h, pitch)], another pitch than the picture's"""
    return [(ar.alloc(bgr_bytes(w, h, p + 8), parity=0), w, h, p + 8) for _, w, h, p in where]


def bgr_regions(where, swhere):
    return [("%s %d" % (k, t), o, o + bgr_bytes(w, h, p)) for k, ww in (("frame", where), ("scratch", swhere)) for t, (o, w, h, p) in enumerate(ww)]


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_blur_entries_bgr(F, net, picture, flags):
    """batch 4 (flags 32: FFGPU_SPLIT2): the very array handed to the forward is blurred frame by frame, radius 8, 3 passes; the records, the full
    lists and the one captured graph are what they were"""
    rng = np.random.default_rng(5470)
    imgs = four_frames(picture)
    ar, where = bgr_arena(rng, imgs)
    swhere = with_scratch(ar, where)
    base = ar.upload()
    fill_bgr(ar, where, imgs)
    frames, scratch = [(base + o, w, h, p) for o, w, h, p in where], [(base + o, w, h, p) for o, w, h, p in swhere]
    sp = Spec(8, 3, False, 0.0, None, (1, 8))
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)], ex.graph_captures
        assert caps == 1 and all(len(b) > 0 for b in boxes)
        ex.blur_bgr(frames, scratch, c_spec(F, sp), F.BLUR_ENTRIES)
        got = ar.download()
        want = ar.start.copy()
        stats = {}
        for (o, w, h, p), (so, _, _, spitch), b in zip(where, swhere, boxes):
            blurref.blur_bgr(want, o, so, w, h, p, spitch, b, sp, stats)
        explain(got, want, bgr_regions(where, swhere), "exec entries, flags %d" % flags)
        assert got.tobytes() != ar.start.tobytes() and stats["changed"] > 0 and stats["win_neighbour"] > 0
        assert ex.read_dets().tobytes() == dets and ex.graph_captures == 1
        assert all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(4))


def test_exec_blur_entries_nv12(F, net, picture):
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    rng = np.random.default_rng(5471)
    imgs = four_frames(picture)
    ar = Arena(rng)
    where, swhere = [], []
    for im in imgs:
        h, w = im.shape[:2]
        for dst, py, puv in ((where, w + 3, 2 * ((w + 1) // 2) + 4), (swhere, w + 1, 2 * ((w + 1) // 2))):
            dst.append((ar.alloc(py * (h - 1) + w, parity=1), ar.alloc(puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2), parity=0), w, h, py, puv))
    base = ar.upload()
    for (oy, ouv, w, h, py, puv), im in zip(where, imgs):
        Y, UV = bgr_to_nv12(im)
        np.lib.stride_tricks.as_strided(ar.start[oy:], shape=(h, w), strides=(py, 1), writeable=True)[...] = Y
        np.lib.stride_tricks.as_strided(ar.start[ouv:], shape=UV.shape, strides=(puv, 1), writeable=True)[...] = UV
    ar.dev.copy_(torch.from_numpy(ar.start))
    frames, scratch = [[(base + oy, base + ouv, w, h, py, puv) for oy, ouv, w, h, py, puv in ww] for ww in (where, swhere)]
    sp = Spec(31, 1, False, 0.0)
    with net.executor(4) as ex:
        ex.forward_nv12_frames_dev(frames)
        dets, boxes = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)]
        assert sum(len(b) for b in boxes) > 0
        ex.blur_nv12(frames, scratch, c_spec(F, sp), F.BLUR_ENTRIES)
        got = ar.download()
        want = ar.start.copy()
        for (oy, ouv, w, h, py, puv), (soy, souv, _, _, spy, spuv), b in zip(where, swhere, boxes):
            blurref.blur_nv12(want, oy, ouv, soy, souv, w, h, py, puv, spy, spuv, b, sp)
        regions = [("%s %d %s" % (k, t, pl), x[i], x[i] + n) for k, ww in (("frame", where), ("scratch", swhere)) for t, x in enumerate(ww)
                   for i, pl, n in ((0, "Y", x[4] * (x[3] - 1) + x[2]), (1, "UV", x[5] * ((x[3] + 1) // 2 - 1) + 2 * ((x[2] + 1) // 2)))]
        explain(got, want, regions, "exec entries, nv12")
        assert got.tobytes() != ar.start.tobytes()
        assert ex.read_dets().tobytes() == dets and ex.graph_captures == 1


def test_exec_blur_merged_then_draw(F, net, picture):
    """2 pictures x 2 tiles: plan, forward, merge, blur the merged lists in the two pictures (everything BUT the boxes), then draw them: blurref
    followed by drawref -- the outlines lie on top; the merged records and lists stay what they were"""
    rng = np.random.default_rng(5472)
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    pics = [wide, np.ascontiguousarray(wide[::-1])]
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    assert len(plan) == 2
    ar, where = bgr_arena(rng, pics, pad=7)
    swhere = with_scratch(ar, where)
    base = ar.upload()
    fill_bgr(ar, where, pics)
    frames, tiles = [], []
    for g, (o, w, h, p) in enumerate(where):
        for x0, y0, tw, th in plan:
            frames.append((base + o + y0 * p + 3 * x0, tw, th, p))
            tiles.append((g, x0, y0))
    whole, scratch = [(base + o, w, h, p) for o, w, h, p in where], [(base + o, w, h, p) for o, w, h, p in swhere]
    sp = Spec(5, 1, True, 0.0, None, (1, 4))
    with net.executor(4) as ex:
        with pytest.raises(RuntimeError, match="no ffgpu_exec_merge_tiles has run"):
            ex.blur_bgr(whole, scratch, c_spec(F, sp), F.BLUR_MERGED)
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 2)
        merged, lists = ex.read_merged(2).tobytes(), [ex.read_merged_boxes(g) for g in range(2)]
        assert all(len(b) > 0 for b in lists)
        ex.blur_bgr(whole, scratch, c_spec(F, sp), F.BLUR_MERGED)
        ex.draw_bgr(whole, F.DRAW_MERGED, color=(255, 0, 255), thickness=2)
        got = ar.download()
        want = ar.start.copy()
        for (o, w, h, p), (so, _, _, spitch), b in zip(where, swhere, lists):
            blurref.blur_bgr(want, o, so, w, h, p, spitch, b, sp)
        only_blurred = want.copy()
        for (o, w, h, p), b in zip(where, lists):
            drawref.draw_bgr(want, o, w, h, p, b, drawref.colours_of(b, (255, 0, 255)), 2)
        explain(got, want, bgr_regions(where, swhere), "exec merged, then draw")
        assert want.tobytes() != only_blurred.tobytes() != ar.start.tobytes()
        assert ex.read_merged(2).tobytes() == merged and ex.graph_captures == 1
        assert all(ex.read_merged_boxes(g).tobytes() == lists[g].tobytes() for g in range(2))


def test_rejections(F, net, picture):
    """every rejected argument with its message, the target's index where there is one; nothing is written by a rejected call, and the next valid
    call on the same executor equals blurref"""
    import ctypes as C
    import torch
    rng = np.random.default_rng(5480)
    imgs = four_frames(picture)
    ar, where = bgr_arena(rng, imgs)
    swhere = with_scratch(ar, where)
    base = ar.upload()
    fill_bgr(ar, where, imgs)
    frames, scratch = [(base + o, w, h, p) for o, w, h, p in where], [(base + o, w, h, p) for o, w, h, p in swhere]
    L = F.lib()
    good = F.blur_spec(8)
    cls = (C.c_ubyte * 8)()

    def spec(radius=8, passes=1, flags=0, nclasses=0, classes=False, margin=(0, 1), reserved=0):
        s = F.BlurSpec()
        s.radius, s.passes, s.flags, s.nclasses, s.classes, s.reserved = radius, passes, flags, nclasses, (C.addressof(cls) if classes else None), reserved
        s.margin_num, s.margin_den = margin
        return s

    def nv_table(ww):
        return F.nv12_frame_table([(base + ww[t][0] + (ww[t][0] & 1), 0, 64, 48) for t in range(4)])     # (an even address: a valid 64 x 48 surface inside surface t)
    with net.executor(4) as ex:
        ex.forward_bgr_frames_dev(frames)
        boxes = [ex.read_boxes(t) for t in range(4)]
        tab, stab, nv, snv = F.bgr_frame_table(frames), F.bgr_frame_table(scratch), nv_table(where), nv_table(swhere)
        d_recs, _ = ex.dets_dev()

        def both(args, msg, nv12_too=True, bgr_too=True):
            """the executor form and the operator, BGR (and NV12 with the same spec / counts; bgr_too False: the tables are NV12 ones)"""
            which, t, c, n, s = args
            calls = []
            if bgr_too:
                calls.append(lambda: L.ffgpu_exec_blur_bgr(ex.h, which, t, c, n, s, None))
                if which == 0:
                    calls.append(lambda: L.ffgpu_blur_boxes_bgr_dev(d_recs, None, 0, None, t, c, n, s, None))
            if nv12_too:
                tn, cn = (t, c) if not bgr_too else ((None if t is None else nv), (None if c is None else snv))
                calls.append(lambda: L.ffgpu_exec_blur_nv12(ex.h, which, tn, cn, n, s, None))
                if which == 0:
                    calls.append(lambda: L.ffgpu_blur_boxes_nv12_dev(d_recs, None, 0, None, tn, cn, n, s, None))
            for c_ in calls:
                assert c_() < 0
                assert re.search(msg, F.last_error()), (msg, F.last_error())
        both((0, None, stab, 4, good), "NULL targets")
        both((0, tab, None, 4, good), "NULL scratch")
        both((0, tab, stab, 4, None), "NULL spec")
        for r in (0, -1, 32, 64):
            both((0, tab, stab, 4, spec(radius=r)), "radius %d " % r)
        for p in (0, -1, 4):
            both((0, tab, stab, 4, spec(passes=p)), "passes %d " % p)
        both((0, tab, stab, 4, spec(flags=2)), "unknown flags 0x2")
        both((0, tab, stab, 4, spec(flags=-1)), "unknown flags")
        both((0, tab, stab, 4, spec(reserved=1)), "reserved must be 0")
        both((0, tab, stab, 4, spec(classes=True, nclasses=0)), "nclasses 0")
        both((0, tab, stab, 4, spec(classes=True, nclasses=257)), "nclasses 257")
        both((0, tab, stab, 4, spec(classes=False, nclasses=2)), "nclasses 2")
        both((0, tab, stab, 4, spec(margin=(1, 0))), "margin 1 / 0")
        both((0, tab, stab, 4, spec(margin=(-1, 4))), "margin -1 / 4")
        both((0, tab, stab, 4, spec(margin=(17, 4))), "margin 17 / 4")
        both((0, tab, stab, 4, spec(margin=(1, 1025))), "margin 1 / 1025")
        both((2, tab, stab, 4, good), "which = 2")
        both((-1, tab, stab, 4, good), "which = -1")
        both((1, tab, stab, 4, good), "no ffgpu_exec_merge_tiles has run")
        assert L.ffgpu_exec_blur_bgr(ex.h, 0, tab, stab, 3, good, None) < 0 and "3 targets for an executor of batch 4" in F.last_error()
        assert L.ffgpu_exec_blur_nv12(ex.h, 0, nv, snv, 5, good, None) < 0 and "5 targets for an executor of batch 4" in F.last_error()
        assert L.ffgpu_blur_boxes_bgr_dev(d_recs, None, 0, None, tab, stab, 0, good, None) < 0 and "ntargets" in F.last_error()
        assert L.ffgpu_blur_boxes_bgr_dev(None, None, 0, None, tab, stab, 4, good, None) < 0 and "NULL records" in F.last_error()
        assert L.ffgpu_blur_boxes_bgr_dev(d_recs, d_recs, 0, None, tab, stab, 4, good, None) < 0 and "list_stride" in F.last_error()
        first = (C.c_int * 4)(0, 0, -5, 0)
        assert L.ffgpu_blur_boxes_bgr_dev(d_recs, d_recs, 8, first, tab, stab, 4, good, None) < 0 and "target 2: negative list start" in F.last_error()
        st = torch.cuda.Stream()
        assert L.ffgpu_exec_blur_bgr(ex.h, 0, tab, stab, 4, good, st.cuda_stream) < 0 and "stream of the forward" in F.last_error()
        # a bad descriptor, target or scratch, with its index and its noun
        for noun in ("target", "scratch"):
            for k, field, val, msg in ((1, "w", 0, "bad size"), (2, "h", -3, "bad size"), (3, "reserved", 1, "reserved"), (0, "pitch", 5, "pitch")):
                bad = F.bgr_frame_table(frames if noun == "target" else scratch)
                setattr(bad[k], field, val)
                both((0, bad, stab, 4, good) if noun == "target" else (0, tab, bad, 4, good), "%s %d: .*%s" % (noun, k, msg), nv12_too=False)
            for k, field, val, msg in ((1, "w", 0, "bad size"), (2, "matrix", 4, "matrix"), (3, "reserved", 1, "reserved"), (0, "pitch_y", 5, "pitch_y"),
                                       (2, "pitch_uv", 63, "pitch_uv"), (1, "uv", base + 1, "odd")):
                bad = nv_table(where if noun == "target" else swhere)
                setattr(bad[k], field, val)
                a, b = (bad, snv) if noun == "target" else (nv, bad)
                assert L.ffgpu_exec_blur_nv12(ex.h, 0, a, b, 4, good, None) < 0
                assert re.search("%s %d: .*%s" % (noun, k, msg), F.last_error()), F.last_error()
                assert L.ffgpu_blur_boxes_nv12_dev(d_recs, None, 0, None, a, b, 4, good, None) < 0
                assert re.search("%s %d: .*%s" % (noun, k, msg), F.last_error()), F.last_error()
        # the scratch table against the targets: sizes, NULLs, overlaps
        bad = F.bgr_frame_table(scratch)
        bad[2].w -= 1
        both((0, tab, bad, 4, good), "scratch 2: %d x %d is not its target's %d x %d" % (where[2][1] - 1, where[2][2], where[2][1], where[2][2]), nv12_too=False)
        bad = nv_table(swhere)
        bad[1].h = 46
        both((0, nv, bad, 4, good), "scratch 1: 64 x 46 is not its target's 64 x 48", bgr_too=False)
        both((0, tab, F.bgr_frame_table(scratch[:3] + [None]), 4, good), "scratch 3 is NULL where its target is not", nv12_too=False)
        both((0, F.bgr_frame_table([None] + frames[1:]), stab, 4, good), "scratch 0 is not NULL where its target is", nv12_too=False)
        o1, w1, h1, p1 = swhere[1]
        both((0, tab, F.bgr_frame_table([scratch[0], scratch[1], scratch[2], (base + o1 + 3 * 7, where[3][1], where[3][2], where[3][3])]), 4, good),
             "scratch 1 overlaps scratch 3", nv12_too=False)
        both((0, tab, F.bgr_frame_table([scratch[0], frames[1], scratch[2], scratch[3]]), 4, good), "scratch 1 overlaps target 1", nv12_too=False)
        both((0, tab, F.bgr_frame_table([scratch[0], scratch[1], (base + where[3][0] + 2, where[2][1], where[2][2], where[2][3]), scratch[3]]), 4, good),
             "scratch 2 overlaps target 3", nv12_too=False)
        bad = nv_table(swhere)
        bad[3].y, bad[3].uv = bad[0].y + 64 * 48 - 2, 0                          # its luma starts inside the chroma plane of scratch 0
        both((0, nv, bad, 4, good), "scratch 0 overlaps scratch 3", bgr_too=False)
        huge, shuge = nv_table(where), nv_table(swhere)                          # 2^24 x 2^24 blocks of 64 x 64: never launched
        for tb in (huge, shuge):
            tb[3].w = tb[3].h = (1 << 30) - 1
            tb[3].pitch_y = tb[3].pitch_uv = 1 << 30
        assert L.ffgpu_exec_blur_nv12(ex.h, 0, huge, shuge, 4, good, None) < 0 and re.search("target 3: .*more than 2\\^23 blocks", F.last_error()), F.last_error()
        assert ar.download().tobytes() == ar.start.tobytes()                    # nothing was launched
        sp = Spec(8)
        ex.blur_bgr(frames[:2] + [None] + frames[3:], scratch[:2] + [None] + scratch[3:], c_spec(F, sp))   # still usable; a NULL address is a skipped target
        got = ar.download()
        want = ar.start.copy()
        for t, ((o, w, h, p), (so, _, _, spitch), b) in enumerate(zip(where, swhere, boxes)):
            if t != 2:
                blurref.blur_bgr(want, o, so, w, h, p, spitch, b, sp)
        explain(got, want, bgr_regions(where, swhere), "after the rejections")
        assert got.tobytes() != ar.start.tobytes()
