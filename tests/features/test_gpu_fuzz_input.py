"""The crops classified on the device: ffgpu_features_dev / ffgpu_topk_dev / ffgpu_crops_relabel_dev (the operators, on seeded tensors, rows, tables and
lists), headless executors with ffgpu_exec_features, and one cascade end to end with ffgpu_exec_relabel -- against tests/features/featref.py, the numpy
restatement of the contract in include/ffcnn_hip.h.  FLAT, MAX, top-k and relabel are compared byte for byte; MEAN, SOFTMAX and L2 against float64 with
the bounds the contract's arithmetic gives (stated where they are used).  Outputs lie in buffers of seeded bytes with guard words before, between and
behind the rows; every byte that is no output must have stayed.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import os
import re

import numpy as np
import pytest

from crops import cropref
from crops.test_gpu_fuzz_input import Arena, four_frames, picture, picture_on_device, to_dev  # noqa: F401  (helpers / fixture)
from features import featref
from layer_ops import cfgs
from overlay import drawref
from test_features_abi import relabel_case
from test_gpu_parity import _write_random_weights
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN, INF = float("nan"), float("inf")
BOX, DETS, LABEL = featref.BOX_DTYPE, featref.DETS_DTYPE, featref.LABEL_DTYPE
PLANES = ((1, 1), (3, 1), (7, 5), (8, 8), (13, 5), (10, 10), (13, 17), (40, 40))      # (h, w): below, at and above one wave's 64 quads, % 4 zero and not
CN = ((1, 1), (3, 2), (5, 3), (65, 64), (129, 65), (1, 65), (129, 1))                # every C of {1, 3, 5, 65, 129} and every N of {1, 2, 3, 64, 65}
GUARD = 7                                                                            # floats in front of the rows (odd: rows are not 16-byte aligned)


def tensor(rng, C, N, H, W, specials=True):
    """(C, N, H, W): planes of different scales up to +-1e4, exact zeros of both signs; every third plane keeps only finite values, the others carry
    layer_ops.cfgs.SPECIALS (NaN with payloads, +-Inf, -0)"""
    x = rng.uniform(-1, 1, (C, N, H, W)).astype(F32) * (10.0 ** rng.integers(-2, 5, (C, N, 1, 1))).astype(F32)
    x[rng.random(x.shape) < 0.05] = 0.0
    x[rng.random(x.shape) < 0.05] = -0.0
    if (C * N) % 5 == 0:
        x[C // 2, N // 2] = np.where(rng.random((H, W)) < 0.5, F32(0.0), F32(-0.0))  # a plane of zeros only
    if specials:
        k = 0
        for c in range(C):
            for n in range(N):
                if (c * N + n) % 3 == 2:
                    continue
                for j in range(1 + k % 3):
                    x[c, n, (k + j) % H, (2 * k + j) % W] = cfgs.SPECIALS[(k + j) % len(cfgs.SPECIALS)]
                k += 1
    return x


class Rows:
    """an output buffer of seeded bytes on the device: GUARD floats, then n rows stride floats apart, then GUARD floats"""

    def __init__(self, rng, n, d, stride, guard=GUARD):
        import torch
        self.n, self.d, self.stride, self.guard = n, d, stride, guard
        self.start = rng.integers(0, 2 ** 32, guard + n * stride + guard, dtype=np.uint32)
        self.dev = torch.from_numpy(self.start.view(np.int32).copy()).cuda()
        self.ptr = self.dev.data_ptr() + 4 * guard

    def read(self, what=""):
        """the rows as (n, d) fp32; everything else must be as it was"""
        import torch
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy().view(np.uint32)
        body = got[self.guard:self.guard + self.n * self.stride].reshape(self.n, self.stride)
        was = self.start[self.guard:self.guard + self.n * self.stride].reshape(self.n, self.stride)
        assert (got[:self.guard] == self.start[:self.guard]).all() and (got[-self.guard:] == self.start[-self.guard:]).all(), what + ": guard words written"
        assert (body[:, self.d:] == was[:, self.d:]).all(), what + ": words between the rows written"
        return np.ascontiguousarray(body[:, :self.d]).view(F32)


def dev_tensor(x, offset):
    """the tensor on the device `offset` floats behind a 256-byte aligned address; returns (keep-alive, pointer)"""
    import torch
    buf = np.zeros(offset + x.size, F32)
    buf[offset:] = x.reshape(-1)
    t = torch.from_numpy(buf.view(np.int32)).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + 4 * offset


def same_bits(got, want, what):
    bad = featref.bits(got) != featref.bits(want)
    assert not bad.any(), "%s: %d of %d values differ in bits, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def check_mean(got, x, what):
    """against the float64 mean: |got - ref| <= gamma(HW - 1) mean|x| + 2^-24 |ref| + 2^-149 (any summation order, one division); planes with
    non-finite values: float64's NaN / +-Inf pattern"""
    ref, bound = featref.mean64(x)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)].astype(F32)), what + ": non-finite pattern"
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    worst = float((err / bound[fin]).max()) if fin.any() else 0.0
    print("%s: MEAN worst error / bound = %.3f" % (what, worst))
    assert worst <= 1.0, "%s: MEAN error is %.3f of its bound" % (what, worst)


def check_post(got, rows, post, what):
    """SOFTMAX: |got - ref| <= (D + 16 + (m - x_i)) 2^-24 ref + 2^-126; L2: <= (D / 2 + 3) 2^-24 |ref| + 2^-149; float64 references of the fp32 row"""
    worst = 0.0
    for r in range(len(rows)):
        ref, bound = (featref.softmax64 if post == featref.SOFTMAX else featref.l2_64)(rows[r])
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got[r]), nan), "%s row %d: NaN pattern" % (what, r)
        inf = np.isinf(ref)
        assert np.array_equal(got[r][inf], ref[inf].astype(F32)), "%s row %d: Inf pattern" % (what, r)
        ok = ~nan & ~inf
        if post == featref.L2 and not ref.any() and not nan.any():
            assert not featref.bits(got[r]).any(), "%s row %d: the zero row" % (what, r)
            continue
        if ok.any():
            err = np.abs(got[r][ok].astype(np.float64) - ref[ok])
            worst = max(worst, float((err / bound[ok]).max()))
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert worst <= 1.0, "%s: error is %.3f of its bound" % (what, worst)


# ---------------------------------------------------------------------------------------------------------------- 1. FLAT, MEAN, MAX
@pytest.mark.parametrize("plane", PLANES)
def test_pool_operators(F, plane):
    import torch
    H, W = plane
    rng = np.random.default_rng(5510 + 100 * H + W)
    for k, (C, N) in enumerate(CN):
        x = tensor(rng, C, N, H, W)
        keep, d_in = dev_tensor(x, (k + H) % 4)                                    # (bases that allow 16-byte loads and bases that do not)
        what = "%dx%d C %d N %d" % (H, W, C, N)
        for pool in (featref.FLAT, featref.MEAN, featref.MAX):
            D = featref.dim(C, H, W, pool)
            out = Rows(rng, N, D, D + (0 if k == 3 else 1 + k % 4), GUARD + k % 2)
            assert F.features_dev(d_in, N, C, H, W, pool, featref.NONE, out.ptr, out.stride) == D
            got = out.read(what)
            if pool == featref.FLAT:
                same_bits(got, featref.flat(x), what + " FLAT")
            elif pool == featref.MAX:
                same_bits(got, featref.maxpool(x), what + " MAX")
            else:
                check_mean(got, x, what)
        del keep
    torch.cuda.synchronize()


def rows_as_tensor(rows, c, h, w):
    """the (C, N, H, W) tensor whose FLAT rows are `rows`"""
    n, d = rows.shape
    assert d == c * h * w
    return np.ascontiguousarray(rows.reshape(n, c, h, w).transpose(1, 0, 2, 3))


def post_rows(rng, D):
    """ordinary rows (one with a +60 outlier, one of large spread), then the special ones: a NaN, a +Inf, a -Inf element, all -Inf, all zero"""
    r = (rng.standard_normal((9, D)) * 3).astype(F32)
    r[1, rng.integers(0, D)] += F32(60)
    r[2] *= F32(20)
    r[3] = F32(0.125)
    r[4, D // 2] = NAN
    r[5, D // 3] = INF
    r[6, (2 * D) // 3] = -INF                                                      # (D == 1: the all -Inf row)
    r[7] = -INF
    r[8] = np.where(rng.random(D) < 0.5, F32(0.0), F32(-0.0))
    return r


POST_D = ((1, (1, 1, 1)), (2, (2, 1, 1)), (5, (1, 5, 1)), (80, (80, 1, 1)), (255, (255, 1, 1)), (1000, (10, 10, 10)), (4097, (4097, 1, 1)),
          (8192, (2, 64, 64)), (8193, (8193, 1, 1)), (70000, (7, 100, 100)))          # 8192 / 8193: the last row staged in LDS, the first that is not


@pytest.mark.parametrize("D,shape", POST_D)
def test_softmax_and_l2(F, D, shape):
    rng = np.random.default_rng(5520 + D)
    rows = post_rows(rng, D)
    x = rows_as_tensor(rows, *shape)
    keep, d_in = dev_tensor(x, D % 2)
    for post in (featref.SOFTMAX, featref.L2):
        out = Rows(rng, len(rows), D, D + 3)
        F.features_dev(d_in, len(rows), *shape, featref.FLAT, post, out.ptr, out.stride)
        got = out.read("D %d post %d" % (D, post))
        check_post(got, rows, post, "D %d %s" % (D, "SOFTMAX" if post == featref.SOFTMAX else "L2"))
        if post == featref.SOFTMAX:
            assert np.isnan(got[[4, 5, 7]]).all() and (D == 1 or (got[6, (2 * D) // 3] == 0 and abs(float(got[6].sum()) - 1) < 1e-3))
            assert (featref.bits(got[[4, 5, 7]]) == 0x7fc00000).all()


def test_post_behind_mean_and_max(F):
    """the post of a pooled row: against featref applied to the device's own pooled row"""
    rng = np.random.default_rng(5530)
    C, N, H, W = 129, 5, 7, 5
    x = tensor(rng, C, N, H, W, specials=False) * F32(1e-3)
    x[:, 3] = 0.0                                                                  # frame 3: the zero row under L2
    x[7, 4, 2, 2] = NAN
    keep, d_in = dev_tensor(x, 0)
    for pool in (featref.MEAN, featref.MAX):
        base = Rows(rng, N, C, C + 2)
        F.features_dev(d_in, N, C, H, W, pool, featref.NONE, base.ptr, base.stride)
        pooled = base.read()
        for post in (featref.SOFTMAX, featref.L2):
            out = Rows(rng, N, C, C + 2)
            F.features_dev(d_in, N, C, H, W, pool, post, out.ptr, out.stride)
            check_post(out.read(), pooled, post, "pool %d post %d" % (pool, post))


def test_determinism_and_position_independence(F):
    """two calls give identical bytes; the row of a frame is the same bytes at N = 1 (on a base that forbids 16-byte loads) and as frame 37 of N = 65"""
    rng = np.random.default_rng(5540)
    for (H, W) in ((10, 10), (13, 17), (40, 40)):
        C = 129
        x = tensor(rng, C, 65, H, W, specials=False)
        one = np.ascontiguousarray(x[:, 37:38])
        k65, d65 = dev_tensor(x, 0)
        k1, d1 = dev_tensor(one, 1)
        for pool, post in ((featref.MEAN, featref.NONE), (featref.MEAN, featref.SOFTMAX), (featref.MEAN, featref.L2), (featref.MAX, featref.L2),
                           (featref.FLAT, featref.NONE)):
            D = featref.dim(C, H, W, pool)
            a, b, c = Rows(rng, 65, D, D + 1), Rows(rng, 65, D, D + 5), Rows(rng, 1, D, D)
            F.features_dev(d65, 65, C, H, W, pool, post, a.ptr, a.stride)
            F.features_dev(d65, 65, C, H, W, pool, post, b.ptr, b.stride)
            F.features_dev(d1, 1, C, H, W, pool, post, c.ptr, c.stride)
            ra, rb, rc = a.read(), b.read(), c.read()
            assert ra.tobytes() == rb.tobytes(), (H, W, pool, post)
            assert ra[37].tobytes() == rc[0].tobytes(), (H, W, pool, post)


# ---------------------------------------------------------------------------------------------------------------- 2. top-k
def topk_rows(rng, D):
    r = rng.integers(-4, 5, (10, D)).astype(F32)                                   # few distinct values: ties everywhere
    r[0] = rng.standard_normal(D)
    r[1] = F32(2.5)
    r[2] = NAN
    r[3] = np.where(rng.random(D) < 0.5, F32(0.0), F32(-0.0))
    r[4][rng.random(D) < 0.3] = INF
    r[4][rng.random(D) < 0.3] = -INF
    r[5][rng.random(D) < 0.5] = NAN
    r[6][rng.random(D) < 0.9] = NAN                                                # too few values that are no NaN
    r[7] = -INF
    r[8][rng.random(D) < 0.2] = -0.0
    return r


@pytest.mark.parametrize("D", (1, 2, 7, 8, 63, 64, 65, 1000, 4097))
def test_topk(F, D):
    import torch
    rng = np.random.default_rng(5550 + D)
    rows = topk_rows(rng, D)
    n, stride = len(rows), D + 1
    buf = np.full((n, stride), 9e9, F32)
    buf[:, :D] = rows
    d_in = to_dev(buf)
    for k in (1, 3, 8, 16):
        ar = Arena(rng)
        off = ar.alloc(8 * n * k, align=4)
        ar.fill()
        base = ar.upload()
        F.topk_dev(d_in.data_ptr(), n, D, k, base + off, in_stride=stride)
        got = ar.download()
        want = ar.start.copy()
        want[off:off + 8 * n * k] = featref.topk(rows, k).view(np.uint8).reshape(-1)
        if got.tobytes() != want.tobytes():
            g = got[off:off + 8 * n * k].view(LABEL).reshape(n, k)
            w = want[off:off + 8 * n * k].view(LABEL).reshape(n, k)
            bad = [r for r in range(n) if g[r].tobytes() != w[r].tobytes()]
            pytest.fail("D %d k %d: rows %s differ (or a guard byte was written); row %d: got %s, want %s" % (D, k, bad, bad[0] if bad else -1,
                                                                                                           g[bad[0]] if bad else "", w[bad[0]] if bad else ""), pytrace=False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 3. relabel
RELABEL_CASES = [(3, (5, 0, 140), 9, 4, True, False), (2, (130, 131), 300, 200, True, True), (4, (3, 9, 0, 1), 4, 2, False, False), (2, (0, 0), 3, 1, True, False),
                 (3, (7, 7, 7), 5, 7, True, True), (300, tuple(k % 7 for k in range(300)), 64, 1, True, False), (5, (129, 140, 3, 128, 0), 40, 9, False, False)]


@pytest.mark.parametrize("case", range(len(RELABEL_CASES)))
def test_relabel_operator(F, case):
    nt, counts, cap, per, with_lists, fg = RELABEL_CASES[case]
    rng = np.random.default_rng(5560 + case)
    for mode in (featref.KEEP_SCORE, featref.LABEL_SCORE):
        for lists_out in (True, False):
            hdr, ent, labels, recs, flat, stride, first = relabel_case(rng, nt, counts, cap, per, with_lists, fg)
            if case == 0:
                recs[1]["count"], recs[1]["nfull"], recs[2]["nfull"] = -3, -7, 2 ** 31 - 1           # counts outside their range are clamped
            if case == 4:                                                                              # entries whose target is outside 0 .. ntargets-1 are ignored
                assert hdr[1] >= 3
                ent[0]["target"], ent[2]["target"] = nt + 3, -5
            spec = featref.RelabelSpec(0.25, 1000, mode)
            want_r, want_l = featref.relabel(hdr, ent, labels, recs, flat, stride, first, spec, with_lists=lists_out)
            S = stride if with_lists else 128
            ar = Arena(rng)
            ro = ar.alloc(recs.nbytes, align=4)
            lo = ar.alloc(24 * nt * S, align=4) if lists_out else None
            ar.fill()
            base = ar.upload()
            d_tab, d_lab, d_recs = to_dev(cropref.table_bytes(hdr, ent)), to_dev(labels), to_dev(recs)
            d_flat = to_dev(flat) if with_lists else None
            k = labels.shape[1]
            F.crops_relabel_dev(d_tab.data_ptr(), cap, d_lab.data_ptr(), k, d_recs.data_ptr(), d_flat.data_ptr() if with_lists else None, stride, nt,
                                F.relabel_spec(0.25, 1000, mode), base + ro, base + lo if lists_out else None, list_first=first)
            got = ar.download()
            want = ar.start.copy()
            want[ro:ro + recs.nbytes] = want_r.view(np.uint8).reshape(-1)
            if lists_out:
                want[lo:lo + 24 * nt * S] = want_l.view(np.uint8).reshape(-1)
            if got.tobytes() != want.tobytes():
                bad = np.nonzero(got != want)[0]
                pytest.fail("case %d mode %d lists %s: %d bytes differ, first at %d (records at %d, lists at %s)" % (case, mode, lists_out, len(bad), bad[0], ro, lo),
                            pytrace=False)
            assert d_recs.cpu().numpy().tobytes() == recs.tobytes() and (not with_lists or d_flat.cpu().numpy().tobytes() == flat.tobytes())


def seeded_labels(rng, cap, k):
    labels = np.zeros((cap, k), LABEL)
    labels["index"] = rng.integers(-1, 6, (cap, k))
    labels["value"] = rng.integers(0, 9, (cap, k)) / 8
    labels["value"][rng.random((cap, k)) < 0.1] = NAN
    return labels


def exec_relabel_against_featref(F, ex, which, tab, cap, recs, lists, S, rng, mode, what):
    """ffgpu_exec_relabel into an arena of seeded bytes: records and lists byte for byte against featref.relabel on the pieces read back, every other
    byte as it was; returns the number of boxes that took a label"""
    nt, k = len(recs), int(rng.integers(1, 4))
    hdr, ent = F.crop_table(tab.cpu().numpy())
    labels = seeded_labels(rng, cap, k)
    ar = Arena(rng)
    ro, lo = ar.alloc(DETS.itemsize * nt, align=4), ar.alloc(24 * nt * S, align=4)
    ar.fill()
    base = ar.upload()
    d_lab = to_dev(labels)
    ex.relabel(tab.data_ptr(), cap, d_lab.data_ptr(), k, F.relabel_spec(0.25, 1000, mode), base + ro, base + lo, which=which, ntargets=nt)
    got = ar.download()
    flat = np.zeros((nt, S), BOX)
    for t, b in enumerate(lists):
        flat[t, :len(b)] = b
    want_r, want_l = featref.relabel((hdr["total"], hdr["taken"], hdr["empty"], hdr["capacity"]), ent, labels, recs, flat.reshape(-1), S, None,
                                     featref.RelabelSpec(0.25, 1000, mode))
    want = ar.start.copy()
    want[ro:ro + DETS.itemsize * nt] = want_r.view(np.uint8).reshape(-1)
    want[lo:lo + 24 * nt * S] = want_l.view(np.uint8).reshape(-1)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        pytest.fail("%s: %d bytes differ, first at %d (records at %d, lists at %d)" % (what, len(bad), bad[0], ro, lo), pytrace=False)
    return int((want_l["type"] >= 1000).sum())


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_relabel_entries(F, net, picture, flags):
    """batch 4 (flags 32: FFGPU_SPLIT2, a split executor: records and lists belong to the parent): FFGPU_RELABEL_ENTRIES behind the forward and
    the crop, both score modes; the records, the lists and the captured graph stay"""
    rng = np.random.default_rng(5630 + flags)
    imgs = four_frames(picture)
    devs = [picture_on_device(im, pad=1 + k) for k, im in enumerate(imgs)]
    frames = [(d.data_ptr(), im.shape[1], im.shape[0], p) for (d, p), im in zip(devs, imgs)]
    import torch
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets(), [ex.read_boxes(t) for t in range(4)], ex.graph_captures
        tab = torch.full((16 + 48 * 7,), 0xA5, dtype=torch.uint8, device="cuda")
        slots = torch.zeros(7 * 3 * 10 * 12, dtype=torch.float32, device="cuda")
        ex.crop_bgr(frames, F.crop_spec(12, 10, F.CROP_F32, per_target=2, min_score=0.3), slots.data_ptr(), tab.data_ptr(), 7)
        torch.cuda.synchronize()
        patched = 0
        for mode in (featref.KEEP_SCORE, featref.LABEL_SCORE, featref.LABEL_SCORE):
            patched += exec_relabel_against_featref(F, ex, F.FFGPU.RELABEL_ENTRIES, tab, 7, dets, boxes, ex.cand_capacity, rng, mode, "entries, flags %d, mode %d" % (flags, mode))
        assert patched > 0
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets.tobytes() and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(4))


def test_exec_relabel_merged_and_rejections(F, net, picture):
    """every rejection of ffgpu_exec_relabel with its message -- those it shares with the operator, a `which` that is neither, FFGPU_RELABEL_MERGED
    before any merge, a wrong ntargets, the wrong stream -- with nothing written; then FFGPU_RELABEL_MERGED behind a two-tile merge of a 1280 x 424
    picture against featref on the merged record and list, and a working ENTRIES call afterwards"""
    import torch
    rng = np.random.default_rng(5640)
    G, L = F.FFGPU, F.lib()
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    dev, pitch = picture_on_device(wide, pad=7)
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    assert len(plan) == 2
    frames = [(dev.data_ptr() + y0 * pitch + 3 * x0, tw, th, pitch) for x0, y0, tw, th in plan]
    whole = [(dev.data_ptr(), 1280, 424, pitch)]
    cs = F.crop_spec(12, 10, F.CROP_F32, per_target=8)
    with net.executor(2) as ex:
        S = ex.cand_capacity
        ex.forward_bgr_frames_dev(frames)
        tab = torch.full((16 + 48 * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        slots = torch.zeros(8 * 3 * 10 * 12, dtype=torch.float32, device="cuda")
        ex.crop_bgr(frames, cs, slots.data_ptr(), tab.data_ptr(), 8)
        lab = to_dev(seeded_labels(rng, 8, 2))
        out = torch.full((2 * DETS.itemsize + 24 * 2 * 2 * S,), 0xA5, dtype=torch.uint8, device="cuda")
        t, l, o, ol = tab.data_ptr(), lab.data_ptr(), out.data_ptr(), out.data_ptr() + 2 * DETS.itemsize
        good, bad_mode, bad_res = F.relabel_spec(0.25, 1000, 1), F.relabel_spec(score_mode=2), F.relabel_spec()
        bad_res.reserved = 1

        def rl(which=0, tab_=t, cap=8, lab_=l, k=2, nt=2, sp=good, orec=o, olist=ol, stream=None):
            return L.ffgpu_exec_relabel(ex.h, which, tab_, cap, lab_, k, nt, sp, orec, olist, stream)
        for kw, msg in ((dict(which=2), "which = 2 is neither"), (dict(which=-1), "which = -1 is neither"),
                        (dict(which=1, nt=1), "no ffgpu_exec_merge_tiles has run"), (dict(nt=1), "1 targets for an executor of batch 2"),
                        (dict(nt=3), "3 targets for an executor of batch 2"), (dict(stream=torch.cuda.Stream().cuda_stream), "stream of the forward or merge"),
                        (dict(tab_=None), "NULL table"), (dict(lab_=None), "NULL labels"), (dict(sp=None), "NULL spec"), (dict(orec=None), "NULL output records"),
                        (dict(cap=0), "capacity 0"), (dict(k=0), "k 0 is outside"), (dict(k=17), "k 17 is outside"), (dict(nt=0), "0 targets"),
                        (dict(sp=bad_mode), "score_mode 2"), (dict(sp=bad_res), "reserved must be 0"), (dict(tab_=t + 8), "16-byte aligned"),
                        (dict(lab_=l + 2), "4-byte aligned"), (dict(orec=o + 1), "4-byte aligned")):
            assert rl(**kw) < 0 and msg in F.last_error(), (msg, F.last_error())
        assert L.ffgpu_exec_relabel(None, 0, t, 8, l, 2, 2, good, o, ol, None) < 0 and "NULL executor" in F.last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xA5).all()                                   # nothing was launched
        ex.merge_tiles([(0, x0, y0) for x0, y0, _, _ in plan], 1)
        merged, lists = ex.read_merged(1), [ex.read_merged_boxes(0)]
        assert len(lists[0]) >= 4
        for kw, msg in ((dict(which=1, nt=2), "2 targets for a merge of 1 pictures"), (dict(which=1, nt=1, stream=torch.cuda.Stream().cuda_stream), "stream of the forward or merge")):
            assert rl(**kw) < 0 and msg in F.last_error(), (msg, F.last_error())
        ex.crop_bgr(whole, cs, slots.data_ptr(), tab.data_ptr(), 8, which=F.CROP_MERGED)
        torch.cuda.synchronize()
        patched = 0
        for mode in (featref.KEEP_SCORE, featref.LABEL_SCORE):
            patched += exec_relabel_against_featref(F, ex, G.RELABEL_MERGED, tab, 8, merged, lists, 2 * S, rng, mode, "merged, mode %d" % mode)
        assert patched > 0 and ex.read_merged(1).tobytes() == merged.tobytes() and ex.read_merged_boxes(0).tobytes() == lists[0].tobytes() and ex.graph_captures == 1
        # ... and the per-entry form works on the same executor afterwards
        dets, boxes = ex.read_dets(), [ex.read_boxes(n) for n in range(2)]
        ex.crop_bgr(frames, cs, slots.data_ptr(), tab.data_ptr(), 8)
        torch.cuda.synchronize()
        assert exec_relabel_against_featref(F, ex, G.RELABEL_ENTRIES, tab, 8, dets, boxes, S, rng, featref.LABEL_SCORE, "entries after the merge") >= 0


# ---------------------------------------------------------------------------------------------------------------- 4. rejections
def test_operator_rejections(F):
    import torch
    L = F.lib()
    x = torch.zeros(4096, dtype=torch.float32, device="cuda")
    o = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, q = x.data_ptr(), o.data_ptr()

    def no(rc, msg):
        assert rc < 0 and re.search(msg, F.last_error()), (msg, F.last_error())
    no(L.ffgpu_features_dev(None, 1, 1, 1, 1, 0, 0, q, 1, None), "NULL input")
    no(L.ffgpu_features_dev(p, 1, 1, 1, 1, 0, 0, None, 1, None), "NULL output")
    for a in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -2)):
        no(L.ffgpu_features_dev(p, *a, 0, 0, q, 4096, None), "every size >= 1")
    no(L.ffgpu_features_dev(p, 1, 2 ** 24 + 1, 1, 1, 1, 0, q, 2 ** 25, None), "more than 2\\^24")
    no(L.ffgpu_features_dev(p, 1, 1025, 128, 128, 0, 0, q, 2 ** 25, None), "more than 2\\^24")
    no(L.ffgpu_features_dev(p, 2, 5, 3, 3, 0, 0, q, 44, None), "out_stride 44 is below the row's 45")
    no(L.ffgpu_features_dev(p, 2, 5, 3, 3, 1, 0, q, 4, None), "out_stride 4 is below the row's 5")
    no(L.ffgpu_features_dev(p, 2, 5, 3, 3, 3, 0, q, 45, None), "pool 3")
    no(L.ffgpu_features_dev(p, 2, 5, 3, 3, -1, 0, q, 45, None), "pool -1")
    no(L.ffgpu_features_dev(p, 2, 5, 3, 3, 0, 3, q, 45, None), "post 3")
    no(L.ffgpu_features_dev(p, 2, 5, 3, 3, 0, 0, q + 2, 45, None), "output must be 4-byte aligned")
    no(L.ffgpu_features_dev(p + 1, 2, 5, 3, 3, 0, 0, q, 45, None), "input must be 4-byte aligned")
    no(L.ffgpu_topk_dev(None, 1, 1, 1, 1, q, None), "NULL input")
    no(L.ffgpu_topk_dev(p, 1, 1, 1, 1, None, None), "NULL output")
    no(L.ffgpu_topk_dev(p, 0, 1, 1, 1, q, None), "0 rows")
    no(L.ffgpu_topk_dev(p, 1, 0, 1, 1, q, None), "rows of 0 values")
    no(L.ffgpu_topk_dev(p, 1, 2 ** 24 + 1, 2 ** 25, 1, q, None), "rows of")
    no(L.ffgpu_topk_dev(p, 2, 8, 7, 1, q, None), "in_stride 7")
    no(L.ffgpu_topk_dev(p, 2, 8, 8, 0, q, None), "k 0 is outside 1..16")
    no(L.ffgpu_topk_dev(p, 2, 8, 8, 17, q, None), "k 17 is outside 1..16")
    no(L.ffgpu_topk_dev(p, 2, 8, 8, 1, q + 1, None), "4-byte aligned")
    sp, bad_mode, bad_res = F.relabel_spec(), F.relabel_spec(score_mode=2), F.relabel_spec()
    bad_res.reserved = 1
    first = (F.C.c_int * 1)(-1)

    def rl(tab=p, cap=4, lab=p, k=1, recs=p, lists=None, stride=0, lf=None, nt=1, s=sp, orec=q, olist=None):
        return L.ffgpu_crops_relabel_dev(tab, cap, lab, k, recs, lists, stride, lf, nt, s, orec, olist, None)
    for kw, msg in ((dict(tab=None), "NULL table"), (dict(lab=None), "NULL labels"), (dict(recs=None), "NULL records"), (dict(s=None), "NULL spec"),
                    (dict(orec=None), "NULL output records"), (dict(cap=0), "capacity 0"), (dict(k=0), "k 0"), (dict(k=17), "k 17"), (dict(nt=0), "0 targets"),
                    (dict(s=bad_mode), "score_mode 2"), (dict(s=bad_res), "reserved"), (dict(tab=p + 8), "16-byte aligned"), (dict(lab=p + 2), "4-byte aligned"),
                    (dict(orec=q + 1), "4-byte aligned"), (dict(lists=p, stride=0), "bad list_stride 0"), (dict(lists=p, stride=4, lf=first), "target 0: negative list start -1"),
                    (dict(orec=p), "must not overlap")):
        no(rl(**kw), msg)
    assert not o.cpu().numpy().any()                                               # nothing was written by a rejected call
    # ... and the operators work afterwards
    x[:8] = torch.arange(8, dtype=torch.float32, device="cuda")
    F.features_dev(p, 1, 8, 1, 1, featref.FLAT, featref.NONE, q)
    F.topk_dev(q, 1, 8, 2, q + 64)
    torch.cuda.synchronize()
    assert o[:8].cpu().numpy().tolist() == list(range(8)) and o[16:20].cpu().numpy().view(LABEL).tolist() == [(7, 7.0), (6, 6.0)]


# ---------------------------------------------------------------------------------------------------------------- 5. headless executors
def headless(trailing_dropout=False, batch=3):
    """conv 1x1 3 -> 5 leaky, max pool 2 / 2, conv 1x1 5 -> 7 linear on 12 x 10: no [yolo] layer"""
    g = cfgs.Cfg("headless%s" % ("_dropout" if trailing_dropout else ""), 12, 10, 3, batch)
    g.conv(5, "leaky")
    g.pool("max", 2, 2)
    g.conv(7)
    if trailing_dropout:
        g.dropout()
    return g


def write_net(orc, tmp, g):
    cfg, wts = os.path.join(tmp, g.name + ".cfg"), os.path.join(tmp, g.name + ".weights")
    with open(cfg, "w") as fp:
        fp.write(g.cfg_text())
    o = orc.Oracle(cfg=cfg, weights=None)
    _write_random_weights(wts, o, 5 + len(g.name))
    o.close()
    return cfg, wts


@pytest.fixture(scope="module")
def tiny(F, orc, tmp_path_factory):
    """the headless net loaded once, its 64 seeded frames and the oracle's last layer of each (computed once, shared, never changed)"""
    cfg, wts = write_net(orc, str(tmp_path_factory.mktemp("features")), headless())
    rng = np.random.default_rng(5570)
    frames = rng.uniform(-1, 1, (64, 3, 10, 12)).astype(F32)
    o = orc.Oracle(cfg=cfg, weights=wts)
    want = np.zeros((64, 7 * 5 * 6), F32)
    for n in range(64):
        o.input[...] = frames[n]
        o.forward()
        want[n] = o.layer_out(2).reshape(-1)
    o.close()
    n = F.Net(cfg, wts)
    yield dict(net=n, cfg=cfg, wts=wts, frames=frames, want=want)
    n.close()


def exec_rows(F, ex, spec, rng, pad=3):
    d = ex.feature_dim(spec)
    out = Rows(rng, ex.batch, d, d + pad)
    assert ex.features(spec, out.ptr, out.stride) == d
    return out.read()


PLAN_FLAGS = (("default", 0), ("NO_FUSE", 8), ("NO_GRAPH", 4), ("KEEP_ALL", 1), ("SPLIT2", 32), ("HOST_DETS | CONCURRENT", 16 | 64), ("KEEP_ALL | NO_FUSE | NO_GRAPH", 13))


@pytest.mark.parametrize("batch", (3, 64))
@pytest.mark.parametrize("plan", PLAN_FLAGS, ids=[p[0] for p in PLAN_FLAGS])
def test_headless_executor(F, tiny, plan, batch):
    """every plan: the records come out zero; FLAT against the oracle's last layer within the project's parity bound 1e-3 + 1e-3 |ref|; on KEEP_ALL
    plans FLAT == read_layer of every frame, bit for bit; MEAN, MAX and every post against featref applied to the executor's own FLAT rows"""
    import torch
    rng = np.random.default_rng(5580 + batch)
    frames, want = tiny["frames"][:batch], tiny["want"][:batch]
    G = F.FFGPU
    with tiny["net"].executor(batch, plan[1]) as ex:
        assert ex.cand_capacity == 1
        d_frames = to_dev(frames)
        for rounds in range(2):                                                    # (the second forward replays the graph)
            if rounds == 0:
                ex.forward_host(frames)
            else:
                ex.forward_dev(d_frames.data_ptr())
            recs = ex.read_dets()
            assert not recs.view(np.uint8).any(), "a headless executor's records are zero"
            assert len(ex.read_boxes(0)) == 0
            flat = exec_rows(F, ex, F.feature_spec(-1, G.FEAT_FLAT), rng)
            assert flat.shape == (batch, 210)
            err = np.abs(flat.astype(np.float64) - want)
            assert (err <= 1e-3 + 1e-3 * np.abs(want)).all(), "FLAT against the oracle: worst %g" % err.max()
        if plan[1] & G.KEEP_ALL:
            for n in range(batch):
                assert flat[n].tobytes() == ex.read_layer(2, n).tobytes(), n
            assert exec_rows(F, ex, F.feature_spec(2, G.FEAT_FLAT), rng).tobytes() == flat.tobytes()
            mid = exec_rows(F, ex, F.feature_spec(1, G.FEAT_FLAT), rng)
            assert mid.shape == (batch, 5 * 5 * 6) and all(mid[n].tobytes() == ex.read_layer(1, n).tobytes() for n in range(batch))
            with pytest.raises(RuntimeError, match="layer 3 is outside -1 .. 2"):
                ex.feature_dim(F.feature_spec(3))
        else:
            with pytest.raises(RuntimeError, match="needs an FFGPU_KEEP_ALL executor"):
                ex.features(F.feature_spec(2, G.FEAT_FLAT), d_frames.data_ptr(), 210)
        x = np.ascontiguousarray(flat.reshape(batch, 7, 5, 6).transpose(1, 0, 2, 3))      # the executor's own tensor, (C, N, H, W)
        mean = exec_rows(F, ex, F.feature_spec(-1, G.FEAT_MEAN), rng, pad=0)
        check_mean(mean, x, plan[0] + " MEAN")
        mx = exec_rows(F, ex, F.feature_spec(-1, G.FEAT_MAX), rng)
        same_bits(mx, featref.maxpool(x), plan[0] + " MAX")
        for pool, pooled in ((G.FEAT_FLAT, flat), (G.FEAT_MEAN, mean), (G.FEAT_MAX, mx)):
            for post in (G.POST_SOFTMAX, G.POST_L2):
                check_post(exec_rows(F, ex, F.feature_spec(-1, pool, post), rng), pooled, post, "%s pool %d post %d" % (plan[0], pool, post))
        assert not ex.read_dets().view(np.uint8).any() and (plan[1] & G.NO_GRAPH or ex.graph_captures >= 1)
    torch.cuda.synchronize()


def test_headless_u8_forms(F, tiny, orc):
    """forward_bgr_dev, forward_bgr_frames_dev and forward_nv12_frames_dev run the headless net: records zero, FLAT against the oracle's run of
    net_input of the same picture (bgr), finite rows (nv12)"""
    import torch
    rng = np.random.default_rng(5590)
    G = F.FFGPU
    w, h, pitch = 30, 22, 92
    img = rng.integers(0, 256, (2, h, pitch), dtype=np.uint8)
    dev = torch.from_numpy(img).cuda()
    o = orc.Oracle(cfg=tiny["cfg"], weights=tiny["wts"])
    want = []
    for n in range(2):
        o.input[...] = 0
        o.set_input_image(img[n], w, h)
        o.forward()
        want.append(o.layer_out(2).reshape(-1).copy())
    o.close()
    want = np.stack(want)
    with tiny["net"].executor(2) as ex:
        for form in ("bgr", "frames", "nv12"):
            if form == "bgr":
                ex.forward_bgr_dev(dev.data_ptr(), w, h)
            elif form == "frames":
                ex.forward_bgr_frames_dev([(dev.data_ptr() + n * h * pitch, w, h, pitch) for n in range(2)])
            else:
                ex.forward_nv12_frames_dev([(dev.data_ptr() + n * h * pitch, 0, 30, 14, 32, 32) for n in range(2)])
            assert not ex.read_dets().view(np.uint8).any()
            flat = exec_rows(F, ex, F.feature_spec(-1, G.FEAT_FLAT), rng)
            if form == "nv12":
                assert np.isfinite(flat).all() and flat.any()
            else:
                assert (np.abs(flat.astype(np.float64) - want) <= 1e-3 + 1e-3 * np.abs(want)).all(), form


def test_layer_resolution_and_exec_rejections(F, net, tiny, orc, tmp_path):
    """a trailing dropout resolves to its source; a net ending in [yolo] is rejected for layer -1; every rejection of ffgpu_exec_features with its
    message, and a working call afterwards"""
    import torch
    rng = np.random.default_rng(5600)
    G, L = F.FFGPU, F.lib()
    cfg, wts = write_net(orc, str(tmp_path), headless(trailing_dropout=True))
    frames = tiny["frames"][:3]
    o = orc.Oracle(cfg=cfg, weights=wts)
    want = []
    for n in range(3):
        o.input[...] = frames[n]
        o.forward()
        assert o.layer_out(3).tobytes() == o.layer_out(2).tobytes()
        want.append(o.layer_out(3).reshape(-1).copy())
    o.close()
    want = np.stack(want)
    with F.Net(cfg, wts) as nd:
        assert nd.layer_num == 4
        with nd.executor(3) as ex:
            ex.forward_host(frames)
            assert ex.feature_dim(F.feature_spec(-1, G.FEAT_FLAT)) == 210 and ex.feature_dim(F.feature_spec(-1, G.FEAT_MAX)) == 7
            a = exec_rows(F, ex, F.feature_spec(-1, G.FEAT_FLAT), rng)
            assert (np.abs(a.astype(np.float64) - want) <= 1e-3 + 1e-3 * np.abs(want)).all()
        with nd.executor(3, G.KEEP_ALL) as ex:
            ex.forward_host(frames)
            for layer in (-1, 3, 2):
                b = exec_rows(F, ex, F.feature_spec(layer, G.FEAT_FLAT), rng)
                assert all(b[n].tobytes() == ex.read_layer(2, n).tobytes() == ex.read_layer(3, n).tobytes() for n in range(3)), layer
    with net.executor(1) as ex:
        with pytest.raises(RuntimeError, match=r"\[yolo\] layer"):
            ex.feature_dim(F.feature_spec(-1))
        out = torch.zeros(64, dtype=torch.float32, device="cuda")
        assert L.ffgpu_exec_features(ex.h, F.feature_spec(-1), out.data_ptr(), 64, None) < 0 and "[yolo] layer" in F.last_error()
        assert L.ffgpu_exec_features(ex.h, F.feature_spec(0), out.data_ptr(), 64, None) < 0 and "FFGPU_KEEP_ALL" in F.last_error()
    with net.executor(1, G.KEEP_ALL) as ex:
        with pytest.raises(RuntimeError, match="not materialised"):
            ex.feature_dim(F.feature_spec(1))                                      # the inside of the fused first kernels
        with pytest.raises(RuntimeError, match=r"\[yolo\] layer"):
            ex.feature_dim(F.feature_spec(net.layer_num - 1))
    with tiny["net"].executor(3) as ex:
        ex.forward_host(frames)
        out = Rows(rng, 3, 210, 210)
        good = F.feature_spec(-1, G.FEAT_FLAT)
        other = torch.cuda.Stream()

        def no(rc, msg):
            assert rc < 0 and re.search(msg, F.last_error()), (msg, F.last_error())
        no(L.ffgpu_exec_features(ex.h, None, out.ptr, 210, None), "NULL spec")
        no(L.ffgpu_exec_features(ex.h, good, None, 210, None), "NULL output")
        no(L.ffgpu_exec_features(ex.h, good, out.ptr, 209, None), "out_stride 209")
        no(L.ffgpu_exec_features(ex.h, good, out.ptr + 2, 210, None), "4-byte aligned")
        no(L.ffgpu_exec_features(ex.h, good, out.ptr, 210, other.cuda_stream), "stream of the forward")
        for kw, msg in ((dict(pool=3), "pool 3"), (dict(post=-1), "post -1"), (dict(reserved=1), "reserved"), (dict(layer=-2), "layer -2"), (dict(layer=3), "layer 3")):
            s = F.feature_spec(-1, G.FEAT_FLAT)
            for k, v in kw.items():
                setattr(s, k, v)
            no(L.ffgpu_exec_features(ex.h, s, out.ptr, 210, None), msg)
            if "post" not in kw:
                no(L.ffgpu_exec_feature_dim(ex.h, s), msg)
        assert exec_rows(F, ex, good, rng).tobytes() == out_of(F, ex, good, out)      # a rejected call wrote nothing and the executor is usable


def out_of(F, ex, spec, out):
    ex.features(spec, out.ptr, out.stride)
    return out.read().tobytes()


# ---------------------------------------------------------------------------------------------------------------- 6. the cascade
def test_cascade_end_to_end(F, net, tiny, picture):
    """detector on data/test.bmp -> ffgpu_exec_crop_bgr (F32 slots of the tiny net's 12 x 10) -> the headless net at batch = capacity -> features
    (MEAN + SOFTMAX) -> top-k -> ffgpu_exec_relabel, all on ONE stream with no synchronisation in between; the relabelled records equal featref
    applied to the pieces read back, the first stage's records and lists are untouched, and ffgpu_draw_boxes_bgr_dev colours by the new type"""
    import torch
    rng = np.random.default_rng(5610)
    G = F.FFGPU
    cap, k = 4, 3
    dev, pitch = picture_on_device(picture)
    frame = (dev.data_ptr(), 640, 424, pitch)
    with net.executor(1) as ex1, tiny["net"].executor(cap) as ex2:
        S = ex1.cand_capacity
        slots = torch.full((cap * 3 * 10 * 12,), float("nan"), dtype=torch.float32, device="cuda")
        tab = torch.full((16 + 48 * cap,), 0xA5, dtype=torch.uint8, device="cuda")
        rows, flat, pool = Rows(rng, cap, 7, 9), Rows(rng, cap, 210, 210), Rows(rng, cap, 7, 7)
        labels = torch.full((cap * k * 2,), -7, dtype=torch.int32, device="cuda")
        ar = Arena(rng)
        ro, lo = ar.alloc(DETS.itemsize, align=4), ar.alloc(24 * S, align=4)
        ar.fill()
        base = ar.upload()
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        ex1.forward_bgr_frames_dev([frame], stream=s)
        ex1.crop_bgr([frame], F.crop_spec(12, 10, F.CROP_F32, per_target=cap, margin=(1, 8)), slots.data_ptr(), tab.data_ptr(), cap, stream=s)
        ex2.forward_dev(slots.data_ptr(), stream=s)
        ex2.features(F.feature_spec(-1, G.FEAT_MEAN, G.POST_SOFTMAX), rows.ptr, rows.stride, stream=s)
        ex2.features(F.feature_spec(-1, G.FEAT_FLAT), flat.ptr, flat.stride, stream=s)
        ex2.features(F.feature_spec(-1, G.FEAT_MEAN), pool.ptr, pool.stride, stream=s)
        F.topk_dev(rows.ptr, cap, 7, k, labels.data_ptr(), in_stride=rows.stride, stream=s)
        ex1.relabel(tab.data_ptr(), cap, labels.data_ptr(), k, F.relabel_spec(0.0, 100, G.RELABEL_LABEL_SCORE), base + ro, base + lo, stream=s)
        st.synchronize()
        dets1, boxes1 = ex1.read_dets(), ex1.read_boxes(0)
        assert len(boxes1) == 3 and not ex2.read_dets().view(np.uint8).any()
        hdr, ent = F.crop_table(tab.cpu().numpy())
        assert (hdr["total"], hdr["taken"], hdr["capacity"]) == (3, 3, cap)
        r, f = rows.read("cascade rows"), flat.read("cascade flat")
        x = np.ascontiguousarray(f.reshape(cap, 7, 5, 6).transpose(1, 0, 2, 3))
        pooled = pool.read("cascade pooled")
        check_mean(pooled, x, "cascade MEAN")
        check_post(r, pooled, featref.SOFTMAX, "cascade MEAN + SOFTMAX")
        lab = labels.cpu().numpy().view(LABEL).reshape(cap, k)
        assert lab.tobytes() == featref.topk(r, k).tobytes()
        flat_list = np.zeros(S, BOX)
        flat_list[:len(boxes1)] = boxes1
        want_r, want_l = featref.relabel((hdr["total"], hdr["taken"], hdr["empty"], hdr["capacity"]), ent, lab, dets1, flat_list, S, None,
                                         featref.RelabelSpec(0.0, 100, featref.LABEL_SCORE))
        got = ar.download()
        want = ar.start.copy()
        want[ro:ro + DETS.itemsize] = want_r.view(np.uint8).reshape(-1)
        want[lo:lo + 24 * S] = want_l.view(np.uint8).reshape(-1)
        assert got.tobytes() == want.tobytes()
        new = got[ro:ro + DETS.itemsize].view(DETS)[0]
        assert [int(t) for t in new["box"]["type"][:3]] == [100 + int(lab[n, 0]["index"]) for n in np.argsort(ent["box"][:3])]
        assert (new["box"]["score"][:3] != dets1[0]["box"]["score"][:3]).all() and new["box"]["x1"][:3].tobytes() == dets1[0]["box"]["x1"][:3].tobytes()
        # the first stage is untouched: records, lists, graph
        assert ex1.read_dets().tobytes() == dets1.tobytes() and ex1.read_boxes(0).tobytes() == boxes1.tobytes() and ex1.graph_captures == 1
        # the relabelled record is a composition point: the draw operator colours by the new type
        pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
        pal[100:107] = [(10 * j, 255 - j, 7 + j) for j in range(7)]
        F.draw_boxes_bgr_dev(base + ro, None, 0, [frame], F.draw_style(palette=pal))
        torch.cuda.synchronize()
        host = np.zeros((424, pitch), np.uint8)
        host[:, :1920] = picture.reshape(424, 1920)
        buf = host.reshape(-1).copy()
        drawref.draw_bgr(buf, 0, 640, 424, pitch, new["box"][:3], drawref.colours_of(new["box"][:3], palette=pal))
        assert dev.cpu().numpy().reshape(-1).tobytes() == buf.tobytes()
        assert buf.tobytes() != host.tobytes()
