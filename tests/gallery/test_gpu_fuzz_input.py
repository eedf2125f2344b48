"""Re-identification on the device: ffgpu_match_dev and ffgpu_gallery_enroll_dev on seeded rows, galleries, counts and ids, and one cascade end to
end -- against tests/gallery/matchref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  Exact data (every partial sum exact in fp32)
are compared byte for byte with matchref alone; random data element by element against float64 within the bound of an fp32 dot product in any order,
and the labels byte for byte with the selection matchref makes on the matrix the device wrote.  Every output lies in an arena of seeded bytes with
guards before, between and behind; every byte that is no output must have stayed.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import re

import numpy as np
import pytest

from crops.test_gpu_fuzz_input import Arena, picture, picture_on_device, to_dev  # noqa: F401  (helpers / fixture)
from features import featref
from features.test_gpu_fuzz_input import Rows, dev_tensor, same_bits, tiny  # noqa: F401  (helpers / fixture)
from gallery import matchref
from layer_ops import cfgs
from overlay import drawref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN, INF = float("nan"), float("inf")
BOX, DETS, LABEL, HEAD = featref.BOX_DTYPE, featref.DETS_DTYPE, matchref.LABEL_DTYPE, matchref.HEAD_DTYPE
JUNK = F32(9e9)
# the kernel as built: 64 queries x 64 gallery rows per workgroup, 16 queries per wave, D in chunks of 32 -- one below, at and one above each edge
NQS = (1, 15, 16, 17, 65) + (63, 64)
CAPS = (1, 15, 17, 127, 129, 300) + (63, 64, 65)
DS = (1, 3, 4, 5, 63, 64, 65, 130) + (31, 32, 33)
KS = (1, 5, 16)


def strided(x, stride):
    """the rows `stride` floats apart, junk between and behind them"""
    n, d = x.shape
    buf = np.full((n, stride), JUNK, F32)
    buf.view(np.uint32)[:, :d] = x.view(np.uint32)
    return buf


def match(F, rng, q, rows, k, ids=None, count=None, with_sim=True, q_pad=0, r_pad=0, q_off=0, r_off=0, sim_pad=0):
    """one ffgpu_match_dev into an arena of seeded bytes; returns the labels (nq, k) and the matrix (nq, capacity) fp32 or None, after checking that
    every other byte stayed.  q_off / r_off: floats behind a 256-byte aligned base (1..3 forbid 16-byte loads); *_pad: floats a stride exceeds its
    minimum by; count: a device head { count, 0, 0, 0 }, None: no head"""
    import torch
    q, rows = np.ascontiguousarray(q, F32), np.ascontiguousarray(rows, F32)
    (nq, D), cap = q.shape, len(rows)
    kq, pq = dev_tensor(strided(q, D + q_pad), q_off)
    kr, pr = dev_tensor(strided(rows, D + r_pad), r_off)
    d_ids = to_dev(np.asarray(ids, np.int32)) if ids is not None else None
    d_head = to_dev(np.array([count, 0, 0, 0], np.int32)) if count is not None else None
    g = F.gallery(pr, cap, D, d_ids.data_ptr() if ids is not None else None, d_head.data_ptr() if count is not None else None, D + r_pad)
    ss = cap + sim_pad
    ar = Arena(rng)
    lo = ar.alloc(8 * nq * k, align=4)
    so = ar.alloc(4 * ((nq - 1) * ss + cap), align=4) if with_sim else None
    ar.fill()
    base = ar.upload()
    wb = F.match_workspace_bytes(nq, cap, k)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    F.match_dev(pq, nq, g, k, base + lo, work.data_ptr(), wb, d_sim=base + so if with_sim else None, sim_stride=ss, q_stride=D + q_pad)
    got = ar.download()
    want = ar.start.copy()
    want[lo:lo + 8 * nq * k] = got[lo:lo + 8 * nq * k]
    sim = None
    if with_sim:
        full = np.zeros(nq * ss, np.uint32)
        full[:(nq - 1) * ss + cap] = got[so:so + 4 * ((nq - 1) * ss + cap)].view(np.uint32)
        sim = np.ascontiguousarray(full.reshape(nq, ss)[:, :cap]).view(F32)
        w = want[so:so + 4 * ((nq - 1) * ss + cap)].view(np.uint32)
        for r in range(nq):
            w[r * ss:r * ss + cap] = sim[r].view(np.uint32)
    assert got.tobytes() == want.tobytes(), "a byte that is no output was written (guards, or between the matrix's rows)"
    if count is not None:
        assert d_head.cpu().numpy().view(np.int32).tolist() == [count, 0, 0, 0]
    return got[lo:lo + 8 * nq * k].view(LABEL).reshape(nq, k).copy(), sim


def same_labels(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = [r for r in range(len(got)) if got[r].tobytes() != want[r].tobytes()]
        pytest.fail("%s: label rows %s differ; row %d: got %s, want %s" % (what, bad[:8], bad[0], got[bad[0]], want[bad[0]]), pytrace=False)


# ---------------------------------------------------------------------------------------------------------------- 1. exact data
def exact_gallery(cap, D):
    """asymmetric small integers, entry (g, j) = (g * D + j) % 251 - 125 scaled by a power of two per row: with one-hot queries every partial sum is
    exact in fp32 in any order"""
    g, j = np.meshgrid(np.arange(cap), np.arange(D), indexing="ij")
    return (((g * D + j) % 251 - 125) * (2.0 ** ((g % 5) - 2))).astype(F32)


@pytest.mark.parametrize("D", DS)
def test_exact_data_byte_for_byte(F, D):
    """queries: the one-hot rows of an identity (repeated past D, scaled by a dyadic per query), so sim(q, g) = scale_q gallery[g][q % D]: a swapped or
    transposed lane map, a wrong row or a wrong k shows; matrix and labels against matchref alone, bit for bit"""
    rng = np.random.default_rng(5700 + D)
    n = 0
    for nq in NQS:
        eye = np.zeros((nq, D), F32)
        eye[np.arange(nq), np.arange(nq) % D] = 2.0 ** (np.arange(nq) // D % 3)
        for cap in CAPS:
            rows = exact_gallery(cap, D)
            k = KS[n % 3]
            ref, _ = matchref.sim64(eye, rows)
            ref32 = ref.astype(F32)
            assert (ref32.astype(np.float64) == ref).all()
            what = "nq %d capacity %d D %d k %d" % (nq, cap, D, k)
            lab, sim = match(F, rng, eye, rows, k, q_pad=n % 3, r_pad=(n // 3) % 4, q_off=n % 4, r_off=(n // 2) % 4, sim_pad=n % 2)
            same_bits(sim, ref32, what)
            same_labels(lab, matchref.select(ref32, k), what)
            if n % 4 == 0:
                lab2, _ = match(F, rng, eye, rows, k, with_sim=False, q_off=1, r_off=2)
                same_labels(lab2, lab, what + " without d_sim")
            n += 1


# ---------------------------------------------------------------------------------------------------------------- 2. random data
def random_rows(rng, n, D, specials):
    """rows of different scales up to +-1e4, exact zeros of both signs; with `specials` every third row carries layer_ops.cfgs.SPECIALS"""
    x = rng.uniform(-1, 1, (n, D)).astype(F32) * (10.0 ** rng.integers(-2, 5, (n, 1))).astype(F32)
    x[rng.random(x.shape) < 0.05] = 0.0
    x[rng.random(x.shape) < 0.05] = -0.0
    if specials:
        for r in range(0, n, 3):
            for j in range(1 + r % 2):
                x[r, (r + 5 * j) % D] = cfgs.SPECIALS[(r // 3 + j) % len(cfgs.SPECIALS)]
    return x


def check_matrix(sim, q, rows, count, ids, what):
    """every finite element within gamma_D sum|a_k b_k| + D 2^-149 of the float64 value; the others by class; rows that are not there 0x7fc00000"""
    ref, mag = matchref.sim64(q, rows, count, ids)
    off = ~matchref.live(len(rows), count, ids)
    assert (featref.bits(sim)[:, off] == 0x7fc00000).all(), what + ": a row that is not there must be the quiet NaN"
    assert np.array_equal(np.isnan(sim), np.isnan(ref)), what + ": NaN pattern"
    inf = np.isinf(ref)
    assert np.array_equal(sim[inf], ref[inf].astype(F32)) and np.array_equal(np.isinf(sim), inf), what + ": Inf pattern"
    fin = np.isfinite(ref)
    if fin.any():
        worst = float((np.abs(sim[fin].astype(np.float64) - ref[fin]) / matchref.bound(mag[fin], q.shape[1])).max())
        print("%s: worst error / bound = %.3f" % (what, worst))
        assert worst <= 1.0, "%s: the error is %.3f of its bound" % (what, worst)


@pytest.mark.parametrize("D", DS)
def test_random_data(F, D):
    rng = np.random.default_rng(5720 + D)
    n = 0
    for nq in NQS:
        for cap in CAPS:
            if (nq, cap) not in ((65, 300), (1, 1)) and (n + D) % 3:                # (a third of the pairs per D, the corners always)
                n += 1
                continue
            k = KS[(n // 3) % 3]
            q, rows = random_rows(rng, nq, D, n % 2 == 0), random_rows(rng, cap, D, True)
            what = "nq %d capacity %d D %d k %d" % (nq, cap, D, k)
            lab, sim = match(F, rng, q, rows, k, q_pad=n % 3, r_pad=(n // 3) % 4, q_off=n % 4, r_off=(n // 2) % 4, sim_pad=1 + n % 2)
            check_matrix(sim, q, rows, None, None, what)
            same_labels(lab, matchref.select(sim, k), what)
            lab2, _ = match(F, rng, q, rows, k, with_sim=False, q_pad=1, r_pad=n % 2, q_off=(n + 1) % 4, r_off=n % 4)
            same_labels(lab2, lab, what + " without d_sim")
            n += 1


def test_position_independence_in_bits(F):
    """a query alone on a base that forbids 16-byte loads against the same query as number 37 of 65; a gallery row as row 0 of capacity 1 against
    the same row as row 200 of 300; two calls give identical bytes"""
    rng = np.random.default_rng(5740)
    for D in (5, 64, 130):
        q, rows = random_rows(rng, 65, D, False), random_rows(rng, 300, D, False)
        lab, sim = match(F, rng, q, rows, 5)
        lab_b, sim_b = match(F, rng, q, rows, 5, q_pad=3, r_pad=1, q_off=2, r_off=3, sim_pad=7)
        assert sim.tobytes() == sim_b.tobytes() and lab.tobytes() == lab_b.tobytes(), D
        lab1, sim1 = match(F, rng, q[37:38], rows, 5, q_off=1)
        assert sim1[0].tobytes() == sim[37].tobytes() and lab1[0].tobytes() == lab[37].tobytes(), D
        _, simg = match(F, rng, q, rows[200:201], 1, r_off=1)
        assert simg[:, 0].tobytes() == sim[:, 200].tobytes(), D
        _, simc = match(F, rng, q, rows, 1, count=201)                             # ... and with the rows behind it not there
        assert simc[:, 200].tobytes() == sim[:, 200].tobytes() and (featref.bits(simc)[:, 201:] == 0x7fc00000).all(), D


# ---------------------------------------------------------------------------------------------------------------- 3. count and ids on the device
def test_count_and_ids(F):
    """count 0, 1, a tile edge, capacity (and beyond its range: clamped) from a device head, and no head; disabled rows; repeated identities; equal
    rows tie and the lower g wins"""
    rng = np.random.default_rng(5750)
    cap, D, nq = 129, 5, 17
    q, rows = random_rows(rng, nq, D, False), random_rows(rng, cap, D, False)
    rows[7] = rng.uniform(0.5, 1, D).astype(F32) * F32(3e4)                        # the longest row by far: the best match of its own direction
    rows[40], rows[90], rows[128], rows[3] = rows[7], rows[7], rows[7], rows[7]      # equal rows, in three tiles
    q[0] = rows[7]
    ids = rng.integers(0, 6, cap).astype(np.int32)                                 # few identities: each appears many times
    ids[rng.random(cap) < 0.2] = -1 - rng.integers(0, 5)
    ids[[3, 7]] = -1, 4                                                            # the first of the equal rows is disabled: row 7 wins
    seen_tie = 0
    for count in (None, 0, 1, 63, 64, 65, 128, 129, 1000, -3):
        for use_ids in (None, ids):
            for k in (1, 16):
                what = "count %s ids %s k %d" % (count, use_ids is not None, k)
                lab, sim = match(F, rng, q, rows, k, ids=use_ids, count=count, r_off=1, sim_pad=3)
                check_matrix(sim, q, rows, count, use_ids, what)
                same_labels(lab, matchref.select(sim, k, use_ids), what)
                lab2, _ = match(F, rng, q, rows, k, ids=use_ids, count=count, with_sim=False)
                same_labels(lab2, lab, what + " without d_sim")
                c = cap if count is None else max(0, min(count, cap))
                if c == 0:
                    assert (lab["index"] == -1).all() and not lab["value"].view(np.uint32).any()
                if use_ids is None and k == 16 and c == cap:
                    for r in range(nq):                                            # rows 3, 7, 40, 90, 128 tie in bits: they stand together, in this order
                        idx = lab[r]["index"].tolist()
                        if 3 in idx and 128 in idx:
                            p = idx.index(3)
                            assert idx[p:p + 5] == [3, 7, 40, 90, 128], idx
                            seen_tie += 1
    assert seen_tie > 0
    # equal rows against a query that favours them: the lowest live g is the best match, with and without ids
    fav = rows[7:8].copy()
    lab, _ = match(F, rng, fav, rows, 4)
    assert lab[0]["index"].tolist() == [3, 7, 40, 90]
    lab, _ = match(F, rng, fav, rows, 3, ids=np.where(np.arange(cap) == 3, -1, np.arange(cap) + 500).astype(np.int32))
    assert lab[0]["index"].tolist() == [507, 540, 590]


# ---------------------------------------------------------------------------------------------------------------- 4. enrol
def unit_rows(rng, n, D):
    x = rng.standard_normal((n, D))
    return (x / np.sqrt((x * x).sum(axis=1, keepdims=True))).astype(F32)


ENROL_CASES = [dict(nq=1, cap=3, D=5, have=0), dict(nq=40, cap=64, D=33, have=0), dict(nq=255, cap=300, D=7, have=20), dict(nq=257, cap=130, D=33, have=5),
               dict(nq=1025, cap=1040, D=16, have=40), dict(nq=70, cap=66, D=4, have=66)]


@pytest.mark.parametrize("case", range(len(ENROL_CASES)), ids=["nq%(nq)d-cap%(cap)d" % c for c in ENROL_CASES])
def test_enrol_then_match(F, case):
    """on ONE stream with no synchronisation in between: match -> enrol -> match.  The gallery starts with `have` rows (0: the all-zero head); some
    queries are gallery rows again (matched), some rows are not finite, two are equal (two identities), and where the gallery is smaller
    than the demand it fills mid-way.  Rows, ids, head and labels byte for byte against matchref.enroll on the labels the device wrote; the second
    match finds every enrolled row as its own best match"""
    import torch
    c = ENROL_CASES[case]
    nq, cap, D, have = c["nq"], c["cap"], c["D"], c["have"]
    rng = np.random.default_rng(5760 + case)
    T = F32(0.9375)
    stride, k = D + 1 + case % 3, 1 + case % 2
    q = unit_rows(rng, nq, D)
    known = unit_rows(rng, max(have, 1), D)
    for r in range(nq):                                                            # a third of the queries are known already
        if have and r % 3 == 1:
            q[r] = known[(r // 3) % have]
    if nq > 20:
        q[5, D // 2], q[11, 0], q[12, D - 1] = NAN, INF, -INF
        q[18] = q[17]
    ar = Arena(rng)
    ro = ar.alloc(4 * cap * stride + 4, align=16) + 4                              # the gallery on a base that forbids 16-byte loads
    io, ho, oo = ar.alloc(4 * cap, align=4), ar.alloc(16, align=16), ar.alloc(8 * nq, align=4)
    l1, l2 = ar.alloc(8 * nq * k, align=4), ar.alloc(8 * nq * k, align=4)
    ar.fill()
    h_rows = ar.start[ro:ro + 4 * cap * stride].view(F32).reshape(cap, stride)
    h_ids, h_head = ar.start[io:io + 4 * cap].view(np.int32), ar.start[ho:ho + 16].view(HEAD)
    h_rows[:have, :D] = known[:have]
    h_ids[:have] = 100 + np.arange(have)
    h_head[0] = (have, 7 if have else 0, 2 if have else 0, 0)
    base = ar.upload()
    kq, pq = dev_tensor(strided(q, D + 2), 1)
    g = F.gallery(base + ro, cap, D, base + io, base + ho, stride)
    wb = F.match_workspace_bytes(nq, cap, k)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    sim1 = torch.empty(nq * cap, dtype=torch.float32, device="cuda")
    sim2 = torch.empty(nq * cap, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    F.match_dev(pq, nq, g, k, base + l1, work.data_ptr(), wb, d_sim=sim1.data_ptr(), q_stride=D + 2, stream=s)
    F.gallery_enroll_dev(g, pq, nq, base + l1, k, float(T), base + oo, q_stride=D + 2, stream=s)
    F.match_dev(pq, nq, g, k, base + l2, work.data_ptr(), wb, d_sim=sim2.data_ptr(), q_stride=D + 2, stream=s)
    st.synchronize()
    got = ar.download()
    m1, m2 = sim1.cpu().numpy().reshape(nq, cap), sim2.cpu().numpy().reshape(nq, cap)
    lab1 = got[l1:l1 + 8 * nq * k].view(LABEL).reshape(nq, k)
    same_labels(lab1, matchref.select(m1, k, h_ids), "the first match")
    assert (featref.bits(m1)[:, have:] == 0x7fc00000).all()
    # the enrolment, on the host copy of the arena
    want = ar.start.copy()
    w_rows = want[ro:ro + 4 * cap * stride].view(F32).reshape(cap, stride)[:, :D]
    w_ids, w_head = want[io:io + 4 * cap].view(np.int32), want[ho:ho + 16].view(HEAD)
    out = matchref.enroll(w_rows, w_ids, w_head[0:1].reshape(()), q, lab1, T)
    want[oo:oo + 8 * nq] = out.view(np.uint8)
    want[l1:l1 + 8 * nq * k] = got[l1:l1 + 8 * nq * k]
    want[l2:l2 + 8 * nq * k] = got[l2:l2 + 8 * nq * k]
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        pytest.fail("%d bytes differ, first at %d (rows at %d, ids at %d, head at %d, labels at %d); head %s, want %s" % (
            len(bad), bad[0], ro, io, ho, oo, got[ho:ho + 16].view(np.int32), w_head), pytrace=False)
    count = int(w_head[0]["count"])
    enrolled = count - have
    assert enrolled == int(w_head[0]["issued"]) - (7 if have else 0) and (enrolled > 0 or have == cap)
    if case == 3:
        assert count == cap and int(w_head[0]["dropped"]) > 2 + 3                  # the gallery filled mid-way: finite rows were dropped as well
    if nq > 20 and enrolled > 20:
        # the NaN row matches nobody and is dropped; the rows with an Inf are dropped where nobody is known (with a gallery their best sim is +Inf:
        # matched, by the contract); the two equal rows are two identities
        assert out["index"][5] == -1 and (have > 0 or out["index"][[11, 12]].tolist() == [-1, -1]) and out["index"][18] == out["index"][17] + 1
    # the second match sees the grown gallery: every enrolled query's best match is itself (of equal rows the first)
    lab2 = got[l2:l2 + 8 * nq * k].view(LABEL).reshape(nq, k)
    same_labels(lab2, matchref.select(m2, k, w_ids), "the second match")
    assert (featref.bits(m2)[:, count:] == 0x7fc00000).all() and not np.isnan(m2[0, :count]).any()
    first = {}
    fresh = [r for r in range(nq) if out[r]["index"] > 0 and not (lab1[r, 0]["index"] >= 0 and lab1[r, 0]["value"] >= T)]
    assert len(fresh) == enrolled
    for r in fresh:
        first.setdefault(q[r].tobytes(), int(out[r]["index"]))
        assert int(lab2[r, 0]["index"]) == first[q[r].tobytes()] and lab2[r, 0]["value"] >= T, (r, lab2[r], out[r])


# ---------------------------------------------------------------------------------------------------------------- 5. rejections
def test_rejections(F):
    """every rejection of the three entry points with its message, nothing written; then working calls"""
    import torch
    L = F.lib()
    x = torch.zeros(8192, dtype=torch.float32, device="cuda")
    o = torch.zeros(8192, dtype=torch.float32, device="cuda")
    p, q = x.data_ptr(), o.data_ptr()
    ids, head, lab, sim, work = q, q + 1024, q + 2048, q + 4096, q + 8192
    wb = F.match_workspace_bytes(4, 8, 2)
    assert wb > 0 and [F.match_workspace_bytes(*a) for a in ((0, 8, 2), (4, 0, 2), (4, 8, 0), (4097, 8, 2), (4, 2 ** 20 + 1, 2), (4, 8, 17))] == [0] * 6

    def no(rc, msg):
        assert rc < 0 and re.search(msg, F.last_error()), (msg, F.last_error())

    def gal(**kw):
        a = dict(d_rows=p + 4096, capacity=8, d=6, d_ids=ids, d_head=head, row_stride=6)
        a.update(kw)
        return F.gallery(a["d_rows"], a["capacity"], a["d"], a["d_ids"], a["d_head"], a["row_stride"])

    def mt(dq=p, nq=4, qs=6, g=gal(), k=2, out=lab, ds=None, ss=8, wk=work, nbytes=wb):
        return L.ffgpu_match_dev(dq, nq, qs, g, k, out, ds, ss, wk, nbytes, None)

    def en(g=gal(), dq=p, nq=4, qs=6, labels=lab, k=2, out=sim):
        return L.ffgpu_gallery_enroll_dev(g, dq, nq, qs, labels, k, 0.5, out, None)
    shared = ((dict(g=None), "NULL gallery"), (dict(g=gal(d_rows=None)), "NULL gallery rows"), (dict(dq=None), "NULL queries"),
              (dict(nq=0), "0 queries"), (dict(nq=4097), "4097 queries"), (dict(k=0), "k 0 is outside 1..16"), (dict(k=17), "k 17 is outside 1..16"),
              (dict(g=gal(capacity=0)), "capacity 0 is outside"), (dict(g=gal(capacity=2 ** 20 + 1)), "capacity 1048577 is outside"),
              (dict(g=gal(d=0)), "rows of 0 values"), (dict(g=gal(d=4097, row_stride=5000)), "rows of 4097 values"),
              (dict(g=gal(row_stride=5)), "row_stride 5 is below the row's 6"), (dict(qs=5), "q_stride 5 is below the row's 6"),
              (dict(g=gal(d_rows=p + 4098)), "d_rows and d_ids must be 4-byte aligned"), (dict(g=gal(d_ids=ids + 1)), "d_rows and d_ids must be 4-byte aligned"),
              (dict(g=gal(d_head=head + 8)), "d_head must be 16-byte aligned"), (dict(dq=p + 2), "4-byte aligned"))
    for kw, msg in shared + ((dict(out=None), "NULL labels"), (dict(wk=None), "NULL workspace"), (dict(ds=sim, ss=7), "sim_stride 7 is below the capacity 8"),
                             (dict(nbytes=wb - 1), "a workspace of %d bytes is below the %d" % (wb - 1, wb)), (dict(nbytes=0), "a workspace of 0 bytes"),
                             (dict(out=lab + 2), "4-byte aligned"), (dict(ds=sim + 1), "4-byte aligned"), (dict(wk=work + 3), "4-byte aligned")):
        no(mt(**kw), "match_dev: .*" + msg)
    for kw, msg in shared + ((dict(g=gal(d_ids=None)), "NULL d_ids"), (dict(g=gal(d_head=None)), "NULL d_head"), (dict(labels=None), "NULL labels"),
                             (dict(out=None), "NULL output labels"), (dict(labels=lab + 1), "4-byte aligned"), (dict(out=sim + 2), "4-byte aligned"),
                             (dict(out=lab), "must not overlap"), (dict(out=lab + 8 * 4 * 2 - 8), "must not overlap"), (dict(labels=sim + 8), "must not overlap")):
        no(en(**kw), "gallery_enroll_dev: .*" + msg)
    torch.cuda.synchronize()
    assert not o.cpu().numpy().any() and not x.cpu().numpy().any()                 # nothing was launched
    # ... and the operators work afterwards: an empty gallery, four queries, all enrolled, all found again
    rows = np.eye(4, 6, dtype=F32) * F32(2)
    x[:24] = torch.from_numpy(rows.reshape(-1)).cuda()
    assert mt() == 0 and en() == 0 and mt(ds=sim) == 0
    torch.cuda.synchronize()
    h = o.cpu().numpy()
    assert h[1024 // 4:1024 // 4 + 4].view(np.int32).tolist() == [4, 4, 0, 0] and h[:8].view(np.int32).tolist() == [1, 2, 3, 4, 0, 0, 0, 0]
    m = h[1024:1024 + 32].reshape(4, 8)
    assert m[:, :4].tolist() == (4 * np.eye(4)).tolist() and (m[:, 4:].view(np.uint32) == 0x7fc00000).all()
    assert h[2048 // 4:2048 // 4 + 16].view(LABEL).reshape(4, 2)[:, 0].tolist() == [(1, 4.0), (2, 4.0), (3, 4.0), (4, 4.0)]
    assert x.cpu().numpy()[1024:1024 + 24].tobytes() == rows.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 6. the cascade
def test_cascade_reidentifies_every_crop(F, net, tiny, picture):
    """data/test.bmp twice in a batch of 2, ONE stream, no synchronisation.  Pass 1: forward -> ffgpu_exec_crop_bgr -> the headless net -> features
    (MEAN + L2) -> match against the empty gallery -> enrol.  Pass 2: the same frames -> match -> ffgpu_exec_relabel -> draw.  Frame 1's crops have
    frame 0's embeddings bit for bit, so pass 1 makes two identities of each (a call does not match its own queries) and pass 2 brings EVERY crop
    back as the identity of the first crop with that embedding: equal rows tie in bits (contract item 1) and the lowest row wins (item 3)"""
    import torch
    rng = np.random.default_rng(5790)
    G = F.FFGPU
    cap, k, D, gcap = 8, 2, 7, 12
    T = 0.96875
    devs = [picture_on_device(picture, pad=4 + 4 * n) for n in range(2)]
    frames = [(d.data_ptr(), 640, 424, p) for d, p in devs]
    with net.executor(2) as ex1, tiny["net"].executor(cap) as ex2:
        S = ex1.cand_capacity
        slots = torch.full((cap * 3 * 10 * 12,), float("nan"), dtype=torch.float32, device="cuda")
        tab = torch.full((16 + 48 * cap,), 0xA5, dtype=torch.uint8, device="cuda")
        rows1, rows2 = Rows(rng, cap, D, D + 2), Rows(rng, cap, D, D + 2)
        ar = Arena(rng)
        go, io, ho = ar.alloc(4 * gcap * D, align=4), ar.alloc(4 * gcap, align=4), ar.alloc(16, align=16)
        l1, e1, l2 = ar.alloc(8 * cap * k, align=4), ar.alloc(8 * cap, align=4), ar.alloc(8 * cap * k, align=4)
        ro, lo = ar.alloc(2 * DETS.itemsize, align=4), ar.alloc(24 * 2 * S, align=4)
        ar.fill()
        ar.start[ho:ho + 16] = 0                                                   # the all-zero head: the valid empty gallery
        base = ar.upload()
        g = F.gallery(base + go, gcap, D, base + io, base + ho)
        wb = F.match_workspace_bytes(cap, gcap, k)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        sim2 = torch.empty(cap * gcap, dtype=torch.float32, device="cuda")
        cs = F.crop_spec(12, 10, F.CROP_F32, per_target=4, margin=(1, 8))
        fs = F.feature_spec(-1, G.FEAT_MEAN, G.POST_L2)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        for rows, lab in ((rows1, l1), (rows2, l2)):
            ex1.forward_bgr_frames_dev(frames, stream=s)
            ex1.crop_bgr(frames, cs, slots.data_ptr(), tab.data_ptr(), cap, stream=s)
            ex2.forward_dev(slots.data_ptr(), stream=s)
            ex2.features(fs, rows.ptr, rows.stride, stream=s)
            F.match_dev(rows.ptr, cap, g, k, base + lab, work.data_ptr(), wb, d_sim=sim2.data_ptr(), q_stride=rows.stride, stream=s)
            if rows is rows1:
                F.gallery_enroll_dev(g, rows.ptr, cap, base + lab, k, T, base + e1, q_stride=rows.stride, stream=s)
        ex1.relabel(tab.data_ptr(), cap, base + l2, k, F.relabel_spec(T, 100, G.RELABEL_LABEL_SCORE), base + ro, base + lo, stream=s)
        st.synchronize()
        dets1, boxes1 = ex1.read_dets(), [ex1.read_boxes(n) for n in range(2)]
        hdr, ent = F.crop_table(tab.cpu().numpy())
        taken = hdr["taken"]
        assert len(boxes1[0]) == 3 and boxes1[0].tobytes() == boxes1[1].tobytes() and (hdr["total"], taken, hdr["capacity"]) == (6, 6, cap)
        r1, r2 = rows1.read("pass 1 rows"), rows2.read("pass 2 rows")
        assert r1.tobytes() == r2.tobytes() and np.isfinite(r1[:taken]).all()
        assert r1[:3].tobytes() == r1[3:6].tobytes() and len({r1[n].tobytes() for n in range(3)}) == 3
        got = ar.download()
        want = ar.start.copy()
        # pass 1: nothing is known; whoever has a finite row is enrolled, in ascending crop slot
        want[l1:l1 + 8 * cap * k] = matchref.select(np.full((cap, gcap), NAN, F32), k).view(np.uint8).reshape(-1)
        w_rows, w_ids, w_head = want[go:go + 4 * gcap * D].view(F32).reshape(gcap, D), want[io:io + 4 * gcap].view(np.int32), want[ho:ho + 16].view(HEAD)
        lab1 = want[l1:l1 + 8 * cap * k].view(LABEL).reshape(cap, k)
        out1 = matchref.enroll(w_rows, w_ids, w_head[0:1].reshape(()), r1, lab1, T)
        want[e1:e1 + 8 * cap] = out1.view(np.uint8)
        assert out1["index"][:taken].tolist() == [1, 2, 3, 4, 5, 6] and int(w_head[0]["count"]) >= 6
        # pass 2: the selection matchref makes on the matrix the device wrote; every crop is the first crop with its embedding
        m2 = sim2.cpu().numpy().reshape(cap, gcap)
        lab2 = matchref.select(m2, k, w_ids)
        want[l2:l2 + 8 * cap * k] = lab2.view(np.uint8).reshape(-1)
        assert lab2[:taken, 0]["index"].tolist() == [1, 2, 3, 1, 2, 3] and (lab2[:taken, 0]["value"] >= F32(T)).all()
        assert lab2[:3, 1]["index"].tolist() == [4, 5, 6] and lab2[:3, 1]["value"].tobytes() == lab2[:3, 0]["value"].tobytes()
        flat_list = np.zeros((2, S), BOX)
        for n in range(2):
            flat_list[n, :len(boxes1[n])] = boxes1[n]
        want_r, want_l = featref.relabel((hdr["total"], taken, hdr["empty"], hdr["capacity"]), ent, lab2, dets1, flat_list.reshape(-1), S, None,
                                         featref.RelabelSpec(T, 100, featref.LABEL_SCORE))
        want[ro:ro + 2 * DETS.itemsize] = want_r.view(np.uint8).reshape(-1)
        want[lo:lo + 24 * 2 * S] = want_l.view(np.uint8).reshape(-1)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got != want)[0]
            pytest.fail("%d bytes differ, first at %d (gallery %d, ids %d, head %d, labels %d / %d / %d, records %d, lists %d)" % (
                len(bad), bad[0], go, io, ho, l1, e1, l2, ro, lo), pytrace=False)
        new = got[ro:ro + 2 * DETS.itemsize].view(DETS)
        assert sorted(int(t) for t in new[0]["box"]["type"][:3]) == [101, 102, 103] and new[1]["box"]["type"][:3].tobytes() == new[0]["box"]["type"][:3].tobytes()
        # the first stage is untouched: records, lists, graph
        assert ex1.read_dets().tobytes() == dets1.tobytes() and all(ex1.read_boxes(n).tobytes() == boxes1[n].tobytes() for n in range(2)) and ex1.graph_captures == 1
        # the relabelled records are a composition point: the draw operator colours by identity
        pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
        pal[100:107] = [(10 * j, 255 - j, 7 + j) for j in range(7)]
        F.draw_boxes_bgr_dev(base + ro, None, 0, frames, F.draw_style(palette=pal))
        torch.cuda.synchronize()
        for n, (d, pitch) in enumerate(devs):
            host = np.zeros((424, pitch), np.uint8)
            host[:, :1920] = picture.reshape(424, 1920)
            buf = host.reshape(-1).copy()
            drawref.draw_bgr(buf, 0, 640, 424, pitch, new[n]["box"][:3], drawref.colours_of(new[n]["box"][:3], palette=pal))
            assert d.cpu().numpy().reshape(-1).tobytes() == buf.tobytes() and buf.tobytes() != host.tobytes(), n
