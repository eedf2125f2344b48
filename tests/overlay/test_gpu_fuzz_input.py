"""The detections drawn into the frames on the device: ffgpu_draw_boxes_bgr_dev / _nv12_dev (the operators, on synthetic records and lists) and
ffgpu_exec_draw_bgr / _nv12 (behind a forward or a merge of the real net) against tests/overlay/drawref.py, the numpy restatement of the
contract in include/ffcnn_hip.h.  Every comparison is byte for byte over the WHOLE allocation: the targets lie in one arena of seeded random
bytes with 64 guard bytes in front of and behind each, so a byte that should have stayed and did not is a failure like a wrong pixel.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLD
from overlay import drawref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BOX = drawref.BOX_DTYPE
COUNTS = (0, 1, 2, 127, 128, 129, 300)
SIZES = ((1, 1), (7, 5), (64, 48), (333, 257))
GUARD = 64



class Arena:
    """one host buffer of seeded random bytes, the targets carved out of it with GUARD bytes around each; the same bytes on the device"""

    def __init__(self, rng):
        self.rng, self.size, self.start, self.dev = rng, 0, None, None

    def alloc(self, nbytes, parity=None):
        """offset of a region of nbytes behind a guard; parity 0 / 1: an even / odd offset (the device base is 256-byte aligned)"""
        off = self.size + GUARD
        if parity is not None and (off & 1) != parity:
            off += 1
        self.size = off + nbytes
        return off

    def upload(self):
        import torch
        self.size += GUARD
        self.start = self.rng.integers(0, 256, self.size, dtype=np.uint8)
        self.dev = torch.from_numpy(self.start.copy()).cuda()
        assert self.dev.data_ptr() % 2 == 0
        return self.dev.data_ptr()

    def download(self):
        import torch
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()


def rand_boxes(rng, n, w, h, ntypes=300):
    """n boxes around a w x h target: about 40 % wholly inside, 35 % across an edge, 25 % wholly outside; classes -ntypes .. ntypes"""
    b = np.zeros(n, BOX)
    b["type"] = rng.integers(-ntypes, ntypes + 1, n)
    b["score"] = rng.uniform(0, 1, n)
    for k in range(n):
        a, c = sorted(int(v) for v in rng.integers(0, w, 2))
        t, d = sorted(int(v) for v in rng.integers(0, h, 2))
        x1, y1, x2, y2 = a + rng.uniform(0, 0.99), t + rng.uniform(0, 0.99), c + rng.uniform(0, 0.99), d + rng.uniform(0, 0.99)
        kind = rng.random()
        if kind < 0.35:                                                          # one or two corners pushed out: part of the outline stays
            side = int(rng.integers(0, 6))
            if side in (0, 4):
                x1 = -rng.uniform(1, w + 2)
            if side in (1, 5):
                y1 = -rng.uniform(1, h + 2)
            if side in (2, 5):
                x2 = w + rng.uniform(0, w + 2)
            if side in (3, 4):
                y2 = h + rng.uniform(0, h + 2)
        elif kind < 0.60:                                                        # moved out as a whole
            dx, dy = ((w + rng.uniform(0, 40), 0), (-(w + rng.uniform(1, 40)), 0), (0, h + rng.uniform(0, 40)), (0, -(h + rng.uniform(1, 40))))[int(rng.integers(0, 4))]
            x1, x2, y1, y2 = x1 + dx, x2 + dx, y1 + dy, y2 + dy
        b[k]["x1"], b[k]["y1"], b[k]["x2"], b[k]["y2"] = x1, y1, x2, y2
    return b


def fixed_boxes(w, h):
    """+-1e30, NaN, inverted and zero-size boxes, a box equal to the frame, boxes on the last row and column"""
    nan, big = float("nan"), 1e30
    rows = [(-big, h // 3, big, big), (-big, -big, big, big), (big, big, big, big), (nan, nan, w // 2, h // 2), (w // 2, nan, nan, h - 1),
            (w - 2, 1, 2, h - 2), (2, h - 2, w - 2, 1), (w - 2, h - 2, 1, 1), (w // 2, h // 2, w // 2, h // 2), (0, 0, w - 1, h - 1),
            (w - 1, h - 1, w - 1, h - 1), (0, h - 1, w - 1, h - 1), (w - 1, 0, w - 1, h - 1), (0, 0, w, h), (-1, -1, w - 1, h - 1),
            (-0.99, -0.99, w - 0.01, h - 0.01), (3e9, 1, -3e9, h - 2), (w // 4, h // 4, w // 4 + 1, h // 4 + 1)]
    b = np.zeros(len(rows), BOX)
    for k, r in enumerate(rows):
        b[k] = (k - 5, 0.5, r[0], r[1], r[2], r[3])
    return b


def records_of(F, lists):
    """the records k_nms would leave beside these full lists"""
    r = np.zeros(len(lists), F.DETS_DTYPE)
    for t, b in enumerate(lists):
        n = len(b)
        r[t]["count"], r[t]["nfull"], r[t]["ncand"] = min(n, 128), n, n
        r[t]["box"][:min(n, 128)] = b[:128]
    return r


def flat_lists(lists, stride):
    flat = np.zeros((len(lists), stride), BOX)
    flat.view(np.uint8)[:] = 0x3C                                               # (slots behind a list hold junk: never read)
    for t, b in enumerate(lists):
        flat[t, :len(b)] = b
    return flat.reshape(-1)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def bgr_bytes(w, h, pitch):
    return pitch * (h - 1) + 3 * w


def explain(got, want, regions, what):
    """which target's region (guards included) differs first"""
    if got.tobytes() == want.tobytes():
        return
    bad = np.nonzero(got != want)[0]
    for name, lo, hi in regions:
        hit = bad[(bad >= lo - GUARD) & (bad < hi + GUARD)]
        if len(hit):
            pytest.fail("%s: %s: %d bytes differ, first at region offset %d (region of %d bytes): got %d, want %d"
                        % (what, name, len(hit), int(hit[0]) - lo, hi - lo, got[hit[0]], want[hit[0]]), pytrace=False)
    pytest.fail("%s: %d bytes differ outside every region, first at %d" % (what, len(bad), int(bad[0])), pytrace=False)


def style_of(F, rng, npal, thickness):
    """(DrawStyle, color, palette): npal 0 = no palette"""
    color = tuple(int(v) for v in rng.integers(0, 256, 3))
    pal = rng.integers(0, 256, (npal, 3)).astype(np.uint8) if npal else None
    return F.draw_style(color, pal, thickness), color, pal


def run_bgr(F, rng, specs, lists, npal, thickness, what, stats=None, use_records=False, first_given=False, twice=False):
    """specs: (w, h, pitch) per target (None: a skipped target), lists: its boxes.  Draws on the device and with drawref; compares the arena."""
    ar = Arena(rng)
    offs = [None if s is None else ar.alloc(bgr_bytes(*s), parity=1) for s in specs]      # odd base addresses
    base = ar.upload()
    st, color, pal = style_of(F, rng, npal, thickness)
    frames = [None if s is None else (base + o, s[0], s[1], s[2]) for s, o in zip(specs, offs)]
    recs = records_of(F, lists)
    d_recs = to_dev(recs)
    stride = max(1, max(len(b) for b in lists)) + 3
    order = list(rng.permutation(len(lists))) if first_given else list(range(len(lists)))     # list t lies in slot order[t]
    slots = [None] * len(lists)
    for t, s in enumerate(order):
        slots[s] = lists[t]
    d_lists = None if use_records else to_dev(flat_lists(slots, stride))
    first = [int(s) * stride for s in order] if first_given else None
    for _ in range(2 if twice else 1):
        F.draw_boxes_bgr_dev(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride, frames, st, first)
    got = ar.download()
    want = ar.start.copy()
    regions = []
    for t, (s, o) in enumerate(zip(specs, offs)):
        if s is None:
            continue
        b = lists[t][:128] if use_records else lists[t]
        local = {}
        drawref.draw_bgr(want, o, s[0], s[1], s[2], b, drawref.colours_of(b, color, pal), thickness, local)
        regions.append(("target %d (%d x %d, pitch %d, %d boxes)" % (t, s[0], s[1], s[2], len(b)), o, o + bgr_bytes(*s)))
        if stats is not None:
            for k, v in local.items():
                stats[k] = stats.get(k, 0) + v
    explain(got, want, regions, what)
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. the operator, BGR
@pytest.mark.parametrize("thickness", [1, 2, 3, 8])
def test_operator_bgr_fuzz(F, thickness):
    """every size x pitch (3 w, ALIGN(3 w, 4), 3 w + 13) as one target each per call, odd base addresses, the list lengths of COUNTS rotated over
    the targets from call to call (each length meets each target within the four thicknesses x four palettes), palettes NULL, 1, 3 and 256"""
    rng = np.random.default_rng(5170 + thickness)
    specs = [(w, h, p) for w, h in SIZES for p in (3 * w, (3 * w + 3) & ~3, 3 * w + 13)]
    total = {}
    for call, npal in enumerate((0, 1, 3, 256)):
        rot = call + 4 * (1, 2, 3, 8).index(thickness)
        lists = [rand_boxes(rng, COUNTS[(k + rot) % 7], s[0], s[1]) for k, s in enumerate(specs)]
        stats = {}
        run_bgr(F, rng, specs, lists, npal, thickness, "thickness %d, palette %d" % (thickness, npal), stats)
        print("thickness %d palette %d: %s" % (thickness, npal, stats))
        if npal >= 2:
            assert stats["overwritten"] > 0, stats
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    assert min(total["clipped"], total["inside"], total["outside"]) * 10 >= total["boxes"], total


@pytest.mark.parametrize("thickness", [1, 8])
def test_operator_bgr_fixed_boxes(F, thickness):
    rng = np.random.default_rng(5180)
    specs = [(64, 48, 3 * 64 + 13), (7, 5, 21), (1, 1, 3), (333, 257, 1000)]
    lists = [fixed_boxes(w, h) for w, h, _ in specs]
    run_bgr(F, rng, specs, lists, 3, thickness, "fixed boxes, thickness %d" % thickness)
    run_bgr(F, rng, specs, [np.concatenate([b, rand_boxes(rng, 20, 64, 48), b[::-1]]) for b in lists], 256, thickness, "fixed boxes twice")


# ---------------------------------------------------------------------------------------------------------------- 2. counts and list starts
def test_operator_records_own_boxes(F):
    """d_lists == NULL: box[0 .. count) of each record, whatever nfull says; a list longer than the record keeps its first 128"""
    rng = np.random.default_rng(5190)
    specs = [(64, 48, 192)] * 5
    lists = [rand_boxes(rng, n, 64, 48) for n in (0, 5, 128, 129, 300)]
    run_bgr(F, rng, specs, lists, 3, 2, "records' own boxes", use_records=True)


def test_operator_list_first(F):
    """the lists in scattered slots named by list_first, against the uniform stride of a NULL list_first; a skipped target stays untouched"""
    rng = np.random.default_rng(5191)
    specs = [(64, 48, 192), None, (7, 5, 21), (333, 257, 999), None, (1, 1, 3)]
    lists = [rand_boxes(rng, n, 64, 48) for n in (40, 9, 2, 129, 300, 1)]
    run_bgr(F, rng, specs, lists, 3, 1, "list_first given", first_given=True)
    run_bgr(F, rng, specs, lists, 3, 1, "list_first NULL")


def test_operator_counts_are_clamped(F):
    """records whose count / nfull is negative or beyond the stride draw the clamped number and touch nothing else"""
    import torch
    rng = np.random.default_rng(5192)
    w, h, pitch, stride = 64, 48, 200, 40
    for use_records in (False, True):
        cap = 128 if use_records else stride
        lists = [rand_boxes(rng, cap, w, h) for _ in range(4)]
        recs = records_of(F, lists)
        claimed = (-1, -2 ** 31, cap + 1, 2 ** 31 - 1)
        for t, c in enumerate(claimed):
            recs[t]["count" if use_records else "nfull"] = c
            recs[t]["nfull" if use_records else "count"] = 7                     # (the other field is not the one that is read)
        ar = Arena(rng)
        offs = [ar.alloc(bgr_bytes(w, h, pitch), parity=1) for _ in range(4)]
        base = ar.upload()
        d_recs = to_dev(recs)
        d_lists = None if use_records else to_dev(flat_lists(lists, stride))
        F.draw_boxes_bgr_dev(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride,
                             [(base + o, w, h, pitch) for o in offs], F.draw_style((9, 8, 7), None, 2))
        got = ar.download()
        want = ar.start.copy()
        for t, o in enumerate(offs):
            b = lists[t][:0] if claimed[t] < 0 else lists[t]
            drawref.draw_bgr(want, o, w, h, pitch, b, drawref.colours_of(b, (9, 8, 7)), 2)
        explain(got, want, [("target %d" % t, o, o + bgr_bytes(w, h, pitch)) for t, o in enumerate(offs)], "clamped counts, records %s" % use_records)
        assert d_recs.cpu().numpy().tobytes() == recs.tobytes()
        torch.cuda.synchronize()


def test_operator_more_targets_than_one_launch(F):
    """300 targets of 8 x 8 (a launch's arguments hold 64) and, at the boundary, 64 and 65"""
    rng = np.random.default_rng(5193)
    for nt in (300, 64, 65):
        specs = [(8, 8, 24 + (t % 3)) for t in range(nt)]
        lists = [rand_boxes(rng, int(rng.integers(0, 6)), 8, 8) for _ in range(nt)]
        run_bgr(F, rng, specs, lists, 3, 1, "%d targets" % nt, first_given=(nt == 300))


# ---------------------------------------------------------------------------------------------------------------- 3. the operator, NV12
def run_nv12(F, rng, specs, lists, npal, thickness, what, twice=False):
    """specs: (w, h, pitch_y, pitch_uv, separate uv plane) per target; both planes, all padding and the guards are compared"""
    ar = Arena(rng)
    offs = []
    for w, h, py, puv, sep in specs:
        ch = (h + 1) // 2
        uv_bytes = puv * (ch - 1) + 2 * ((w + 1) // 2)
        if sep:
            offs.append((ar.alloc(py * (h - 1) + w, parity=1), ar.alloc(uv_bytes, parity=0)))
        else:                                                                  # one surface: uv = y + pitch_y h, which must come out even
            oy = ar.alloc(py * h + uv_bytes, parity=(py * h) & 1)
            offs.append((oy, oy + py * h))
    base = ar.upload()
    st, color, pal = style_of(F, rng, npal, thickness)
    frames = [(base + oy, base + ouv if s[4] else 0, s[0], s[1], s[2], s[3]) for s, (oy, ouv) in zip(specs, offs)]
    recs = records_of(F, lists)
    stride = max(1, max(len(b) for b in lists))
    d_recs, d_lists = to_dev(recs), to_dev(flat_lists(lists, stride))
    for _ in range(2 if twice else 1):
        F.draw_boxes_nv12_dev(d_recs.data_ptr(), d_lists.data_ptr(), stride, frames, st)
    got = ar.download()
    want = ar.start.copy()
    regions = []
    for t, (s, (oy, ouv)) in enumerate(zip(specs, offs)):
        drawref.draw_nv12(want, oy, ouv, s[0], s[1], s[2], s[3], lists[t], drawref.colours_of(lists[t], color, pal), thickness)
        regions.append(("target %d Y (%d x %d, pitches %d / %d, %d boxes)" % (t, s[0], s[1], s[2], s[3], len(lists[t])), oy, oy + s[2] * (s[1] - 1) + s[0]))
        regions.append(("target %d UV" % t, ouv, ouv + s[3] * ((s[1] + 1) // 2 - 1) + 2 * ((s[0] + 1) // 2)))
    explain(got, want, regions, what)
    return got


@pytest.mark.parametrize("thickness", [1, 2, 3, 8])
def test_operator_nv12_fuzz(F, thickness):
    rng = np.random.default_rng(5200 + thickness)
    specs = []
    for w, h in ((1, 1), (7, 5), (63, 47), (64, 48)):
        mu = 2 * ((w + 1) // 2)
        specs += [(w, h, w, mu, False), (w, h, w, mu, True), (w, h, w + 5, mu + 6, False), (w, h, w + 6, mu + 10, True)]
    for call, npal in enumerate((0, 3, 256)):
        rot = call + 3 * (1, 2, 3, 8).index(thickness)
        lists = [rand_boxes(rng, COUNTS[(k + rot) % 7], s[0], s[1]) for k, s in enumerate(specs)]
        run_nv12(F, rng, specs, lists, npal, thickness, "nv12 thickness %d, palette %d" % (thickness, npal))
    run_nv12(F, rng, specs, [fixed_boxes(s[0], s[1]) for s in specs], 3, thickness, "nv12 fixed boxes")


def test_operator_nv12_shared_chroma_sample(F):
    """two boxes of different colours share chroma sample (1, 1) through different luma pixels: each keeps its Y, the sample is the later box's;
    and the earlier box wins nothing back when it comes first in a longer list"""
    rng = np.random.default_rng(5210)
    b = np.zeros(2, BOX)
    b[0] = (0, 0.5, 2, 2, 2, 2)
    b[1] = (1, 0.5, 3, 3, 3, 3)
    for lists in ([b], [b[::-1].copy()], [np.concatenate([b, b[:1]])]):
        got = run_nv12(F, rng, [(8, 6, 8, 8, False)], lists, 3, 1, "shared chroma sample")
        assert len(got)


# ---------------------------------------------------------------------------------------------------------------- 4. run twice
def test_same_list_twice_gives_the_same_bytes(F):
    """one heavily overlapping list, drawn twice from the same start buffer in two separate runs: identical bytes (and both equal drawref)"""
    outs = []
    for _ in range(2):
        rng = np.random.default_rng(5220)
        specs = [(333, 257, 1012), (64, 48, 192)]
        lists = [rand_boxes(rng, 300, 40, 30), rand_boxes(rng, 129, 20, 20)]     # crowded into a corner: most pixels have several writers
        outs.append(run_bgr(F, rng, specs, lists, 256, 3, "run twice").tobytes())
    assert outs[0] == outs[1]
    rng = np.random.default_rng(5221)
    run_bgr(F, rng, [(64, 48, 192)], [rand_boxes(rng, 129, 20, 20)], 256, 3, "drawn twice into the same buffer", twice=True)


# ---------------------------------------------------------------------------------------------------------------- the real net
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return rows[:, :3 * w].reshape(h, w, 3)


def four_frames(picture):
    """four seeded crops / shifts of the picture, all of different sizes"""
    rng = np.random.default_rng(5230)
    out = [picture]
    for _ in range(3):
        x0, y0 = int(rng.integers(0, 60)), int(rng.integers(0, 40))
        out.append(picture[y0:424 - int(rng.integers(0, 40)), x0:640 - int(rng.integers(0, 60))])
    return [np.ascontiguousarray(f) for f in out]


def bgr_arena(rng, imgs, pad=13):
    """the pictures in one arena (pitch 3 w + pad); returns (arena, [(offset, w, h, pitch)])"""
    ar = Arena(rng)
    where = []
    for im in imgs:
        h, w = im.shape[:2]
        where.append((ar.alloc(bgr_bytes(w, h, 3 * w + pad), parity=1), w, h, 3 * w + pad))
    return ar, where


def fill_bgr(ar, where, imgs):
    import torch
    for (o, w, h, pitch), im in zip(where, imgs):
        v = np.lib.stride_tricks.as_strided(ar.start[o:], shape=(h, w, 3), strides=(pitch, 3, 1), writeable=True)
        v[...] = im
    ar.dev.copy_(torch.from_numpy(ar.start))


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_draw_entries_bgr(F, net, picture, flags):
    """batch 4 (flags 32: FFGPU_SPLIT2): the very array handed to the forward draws each frame's boxes into that frame; the records, the full
    lists and the one captured graph are what they were"""
    rng = np.random.default_rng(5231)
    imgs = four_frames(picture)
    ar, where = bgr_arena(rng, imgs)
    base = ar.upload()
    fill_bgr(ar, where, imgs)
    frames = [(base + o, w, h, p) for o, w, h, p in where]
    pal = rng.integers(0, 256, (80, 3)).astype(np.uint8)
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)], ex.graph_captures
        assert caps == 1 and all(len(b) > 0 for b in boxes)
        ex.draw_bgr(frames, F.DRAW_ENTRIES, palette=pal, thickness=2)
        got = ar.download()
        want = ar.start.copy()
        for (o, w, h, p), b in zip(where, boxes):
            drawref.draw_bgr(want, o, w, h, p, b, drawref.colours_of(b, palette=pal), 2)
        explain(got, want, [("frame %d" % t, o, o + bgr_bytes(w, h, p)) for t, (o, w, h, p) in enumerate(where)], "exec entries, flags %d" % flags)
        assert got.tobytes() != ar.start.tobytes()
        assert ex.read_dets().tobytes() == dets and ex.graph_captures == 1
        assert all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(4))


def test_exec_draw_entries_nv12(F, net, picture):
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    rng = np.random.default_rng(5232)
    imgs = four_frames(picture)
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
    frames = [(base + oy, base + ouv, w, h, py, puv) for oy, ouv, w, h, py, puv in where]
    with net.executor(4) as ex:
        ex.forward_nv12_frames_dev(frames)
        dets, boxes = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)]
        assert sum(len(b) for b in boxes) > 0
        ex.draw_nv12(frames, F.DRAW_ENTRIES, color=(81, 90, 240), thickness=3)
        got = ar.download()
        want = ar.start.copy()
        for (oy, ouv, w, h, py, puv), b in zip(where, boxes):
            drawref.draw_nv12(want, oy, ouv, w, h, py, puv, b, drawref.colours_of(b, (81, 90, 240)), 3)
        explain(got, want, [("frame %d Y" % t, x[0], x[0] + x[4] * (x[3] - 1) + x[2]) for t, x in enumerate(where)], "exec entries, nv12")
        assert got.tobytes() != ar.start.tobytes()
        assert ex.read_dets().tobytes() == dets and ex.graph_captures == 1


def test_exec_draw_merged(F, net, picture):
    """2 pictures x 2 tiles: plan, forward, merge, draw the merged lists into the two pictures; the merged records stay what they were"""
    rng = np.random.default_rng(5233)
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
    with net.executor(4) as ex:
        with pytest.raises(RuntimeError, match="no ffgpu_exec_merge_tiles has run"):
            ex.draw_bgr([(base + o, w, h, p) for o, w, h, p in where], F.DRAW_MERGED)
        ex.forward_bgr_frames_dev(frames)
        ex.merge_tiles(tiles, 2)
        merged, lists = ex.read_merged(2).tobytes(), [ex.read_merged_boxes(g) for g in range(2)]
        assert all(len(b) > 0 for b in lists)
        ex.draw_bgr([(base + o, w, h, p) for o, w, h, p in where], F.DRAW_MERGED, color=(255, 0, 255), thickness=2)
        got = ar.download()
        want = ar.start.copy()
        for (o, w, h, p), b in zip(where, lists):
            drawref.draw_bgr(want, o, w, h, p, b, drawref.colours_of(b, (255, 0, 255)), 2)
        explain(got, want, [("picture %d" % g, o, o + bgr_bytes(w, h, p)) for g, (o, w, h, p) in enumerate(where)], "exec merged")
        assert got.tobytes() != ar.start.tobytes()
        assert ex.read_merged(2).tobytes() == merged and ex.graph_captures == 1


def test_end_to_end_is_the_reference_programs_out_bmp(F):
    """a net loaded at 640 x 424 (rounded to 640 x 448), data/test.bmp on the device, forward, draw green with thickness 1, download, write
    with the demo's header: the SHA-256 of the reference program's own out.bmp (tests/golden/cli.json)"""
    import torch
    cli = json.load(open(os.path.join(GOLD, "cli.json")))
    rects = [tuple(int(v) for v in re.search(r"rect: \(\s*(-?\d+)\s+(-?\d+)\s+(-?\d+)\s+(-?\d+)\)", line).groups()) for line in cli["detections"]]
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    dev = torch.from_numpy(rows.copy()).cuda()
    with F.Net(w=w, h=h) as n:
        assert n.input_shape == (3, 448, 640)
        with n.executor(1) as ex:
            frame = [(dev.data_ptr(), w, h, rows.shape[1])]
            ex.forward_bgr_frames_dev(frame)
            got = [drawref.corners(b) for b in ex.read_boxes(0)]
            assert got == rects, "a finding about the FORWARD, not about the drawing: the executor's truncated corners %s are not the reference's %s" % (got, rects)
            ex.draw_bgr(frame, F.DRAW_ENTRIES, color=(0, 255, 0), thickness=1)
            torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert hashlib.sha256(drawref.bmp_file(out, w, h)).hexdigest() == cli["out_bmp_sha256"]


def test_rejections(F, net, picture):
    """every rejected argument with its message, the target's index where there is one; nothing is drawn by a rejected call, and the next valid
    call on the same executor equals drawref"""
    import ctypes as C
    import torch
    rng = np.random.default_rng(5240)
    imgs = four_frames(picture)
    ar, where = bgr_arena(rng, imgs)
    base = ar.upload()
    fill_bgr(ar, where, imgs)
    frames = [(base + o, w, h, p) for o, w, h, p in where]
    L = F.lib()
    good = F.draw_style()
    pal = (C.c_ubyte * 8)()

    def style(thickness=1, palette=None, npalette=0):
        s = F.DrawStyle()
        s.thickness, s.palette, s.npalette = thickness, (C.addressof(pal) if palette else None), npalette
        return s
    with net.executor(4) as ex:
        ex.forward_bgr_frames_dev(frames)
        boxes = [ex.read_boxes(t) for t in range(4)]
        tab = F.bgr_frame_table(frames)
        nv = F.nv12_frame_table([(base + where[t][0] + 1, 0, 64, 48) for t in range(4)])     # (an even address: a valid 64 x 48 surface inside frame t)
        d_recs, _ = ex.dets_dev()

        def both(args_bgr, msg, nv12_too=True):
            """the executor form and the operator, BGR (and NV12 with the same style / counts)"""
            which, t, n, s = args_bgr
            calls = [lambda: L.ffgpu_exec_draw_bgr(ex.h, which, t, n, s, None)]
            if which == 0:
                calls.append(lambda: L.ffgpu_draw_boxes_bgr_dev(d_recs, None, 0, None, t, n, s, None))
            if nv12_too:
                calls.append(lambda: L.ffgpu_exec_draw_nv12(ex.h, which, None if t is None else nv, n, s, None))
            for c in calls:
                assert c() < 0
                assert re.search(msg, F.last_error()), (msg, F.last_error())
        both((0, None, 4, good), "NULL targets")
        both((0, tab, 4, None), "NULL style")
        both((0, tab, 4, style(0)), "thickness 0")
        both((0, tab, 4, style(9)), "thickness 9")
        both((0, tab, 4, style(1, True, 0)), "npalette 0")
        both((0, tab, 4, style(1, True, 257)), "npalette 257")
        both((0, tab, 4, style(1, False, 2)), "npalette 2")
        both((2, tab, 4, good), "which = 2")
        both((-1, tab, 4, good), "which = -1")
        both((1, tab, 4, good), "no ffgpu_exec_merge_tiles has run")
        assert L.ffgpu_exec_draw_bgr(ex.h, 0, tab, 3, good, None) < 0 and "3 targets for an executor of batch 4" in F.last_error()
        assert L.ffgpu_exec_draw_nv12(ex.h, 0, nv, 5, good, None) < 0 and "5 targets for an executor of batch 4" in F.last_error()
        assert L.ffgpu_draw_boxes_bgr_dev(d_recs, None, 0, None, tab, 0, good, None) < 0 and "ntargets" in F.last_error()
        assert L.ffgpu_draw_boxes_bgr_dev(None, None, 0, None, tab, 4, good, None) < 0 and "NULL records" in F.last_error()
        assert L.ffgpu_draw_boxes_bgr_dev(d_recs, d_recs, 0, None, tab, 4, good, None) < 0 and "list_stride" in F.last_error()
        first = (C.c_int * 4)(0, 0, -5, 0)
        assert L.ffgpu_draw_boxes_bgr_dev(d_recs, d_recs, 8, first, tab, 4, good, None) < 0 and "target 2: negative list start" in F.last_error()
        st = torch.cuda.Stream()
        assert L.ffgpu_exec_draw_bgr(ex.h, 0, tab, 4, good, st.cuda_stream) < 0 and "stream of the forward" in F.last_error()
        for k, field, val, msg in ((1, "w", 0, "bad size"), (2, "h", -3, "bad size"), (3, "reserved", 1, "reserved"), (0, "pitch", 5, "pitch")):
            bad = F.bgr_frame_table(frames)
            setattr(bad[k], field, val)
            both((0, bad, 4, good), "target %d: .*%s" % (k, msg), nv12_too=False)
        for k, field, val, msg in ((1, "w", 0, "bad size"), (2, "matrix", 4, "matrix"), (3, "reserved", 1, "reserved"), (0, "pitch_y", 5, "pitch_y"),
                                   (2, "pitch_uv", 63, "pitch_uv"), (1, "uv", base + 1, "odd")):
            bad = F.nv12_frame_table([(base + where[t][0] + 1, 0, 64, 48) for t in range(4)])
            setattr(bad[k], field, val)
            assert L.ffgpu_exec_draw_nv12(ex.h, 0, bad, 4, good, None) < 0
            assert re.search("target %d: .*%s" % (k, msg), F.last_error()), F.last_error()
            assert L.ffgpu_draw_boxes_nv12_dev(d_recs, None, 0, None, bad, 4, good, None) < 0
            assert re.search("target %d: .*%s" % (k, msg), F.last_error()), F.last_error()
        assert ar.download().tobytes() == ar.start.tobytes()                    # nothing was launched
        ex.draw_bgr(frames[:2] + [None] + frames[3:])                           # the executor is still usable; a NULL address is a skipped target
        got = ar.download()
        want = ar.start.copy()
        for t, ((o, w, h, p), b) in enumerate(zip(where, boxes)):
            if t != 2:
                drawref.draw_bgr(want, o, w, h, p, b, drawref.colours_of(b, (0, 255, 0)), 1)
        explain(got, want, [("frame %d" % t, o, o + bgr_bytes(w, h, p)) for t, (o, w, h, p) in enumerate(where)], "after the rejections")
        assert got.tobytes() != ar.start.tobytes()
