"""The sparse form of the pointwise layer in front of a yolo head (ffgpu_conv_x3.inc "SPARSE HEAD": a box pass over all pixels that lists the quads whose
objectness can pass, a class pass over the listed quads) through ffgpu_sparse_head_dev, against the dense K_CONV_X3 launch on the same tensors.

Every value the pair writes must have the dense launch's BITS: the output starts as a sentinel (a NaN with a payload no arithmetic produces) between guard
words, and after the pair
  * the 15 box rows equal the dense ones everywhere,
  * the list, as a set and without duplicates, is the set of quads with a passing (pixel, anchor) under k_yolo's predicate evaluated here from the dense
    launch's objectness bits,
  * the class rows equal the dense ones at listed quads and are still the sentinel everywhere else.

The predicate on the host.  The device evaluates !(1 / (1 + __expf(-bs)) < thresh * 0.999f).  The right side is one IEEE fp32 product: exact here.  The
left side goes through the hardware's exp2 approximation (1 ulp) behind an fp32 product with log2(e), then an fp32 add and divide: a relative error of a
few 2^-23 in all, for |bs| up to the few units that matter.  The host computes the sigmoid in float64 and calls an objectness DECIDED when it differs
from the threshold by more than 1e-5 relative (about thirty times that error) and UNDECIDED inside: a quad whose outcome hangs on an undecided value
may be listed or not, and is then held to the same rule as every quad -- class rows dense where listed, sentinel where not.  The boundary case plants
values one ulp either side of the float64 boundary (undecided: either outcome, consistently) and 1e-4 either side (decided: the exact outcome).

Shapes (P pixels x ic channels x classes): P = 4 (one quad), 68 (a tile seam: 17 quads), 260 (a range seam of the four-wave workgroup's 256 pixels; five
frames of 13 x 4, quads straddle frames); ic = 8 (one k-unit), 40 (a ragged last group), 120 (the real layer); classes = 1, 20 (padded class block), 80.


(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = 0x7FC5A5A5           # the output's sentinel: a quiet NaN with a payload
GUARD = 0x5A5AA5A5
LSENT = -0x12345678         # the list's sentinel
THRESH = 0.45
PLANES = {4: (1, 2, 2), 68: (1, 17, 4), 260: (5, 13, 4)}       # P -> (N, iw, ih)
CASES = ("none", "all", "first", "last", "per_tile", "boundary", "nonfinite", "overflow")


@pytest.fixture(scope="module")
def env():
    import torch
    from ffcnn_amd import capi
    capi.lib()
    return capi, torch


@pytest.fixture()
def clean(monkeypatch):
    from test_irb_choice import knob_names
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def boundary32():
    """the float32 nearest the float64 solution of sigmoid(b) = thresh * 0.999f"""
    t = float(np.float32(THRESH) * np.float32(0.999))
    return np.float32(-np.log(1.0 / t - 1.0))


@functools.lru_cache(maxsize=None)
def tensors(P, ic, classes, case):
    """input (ic, P) and filter rows (oc, k4 + 4), read only.  Objectness of anchor a is input channel a alone (weight 1, scale 1, bias 0), so a case
    steers it through x[a]: -10 fails, +3 passes.  Every other row is a random filter with a random scale and bias."""
    rng = np.random.default_rng(1000 * P + 10 * ic + classes)
    A = 5 + classes
    oc, k4 = 3 * A, (ic + 3) & ~3
    x = rng.standard_normal((ic, P)).astype(np.float32)
    f = np.zeros((oc, k4 + 4), np.float32)
    f[:, :ic] = rng.standard_normal((oc, ic)).astype(np.float32) / np.float32(np.sqrt(ic))
    f[:, k4] = rng.uniform(0.5, 1.5, oc).astype(np.float32)
    f[:, k4 + 1] = rng.uniform(-0.5, 0.5, oc).astype(np.float32)
    for a in range(3):
        f[a * A + 4, :] = 0
        f[a * A + 4, a] = 1
        f[a * A + 4, k4] = 1
    nq = P // 4
    x[:3] = -10
    if case in ("all", "overflow"):
        x[:3] = 3
    elif case == "first":
        x[1, 2] = 3                                     # quad 0: its third pixel, the second anchor
    elif case == "last":
        x[2, P - 1] = 3
    elif case == "per_tile":
        for q in range(0, nq, 16):
            x[(q // 16) % 3, 4 * q + (q // 16) % 4] = 3
        x[0, P - 4] = 3
    elif case == "boundary":
        b = boundary32()
        vals = [np.nextafter(b, np.float32(-np.inf)), b, np.nextafter(b, np.float32(np.inf)), b - np.float32(1e-4), b + np.float32(1e-4)]
        for q in range(nq):
            x[q % 3, 4 * q + q % 4] = vals[q % 5]
    elif case == "nonfinite":
        xb = x.view(np.uint32)
        specials = [0x7FC12345, 0x7F800000, 0xFF800000]
        for q in range(nq):
            xb[q % 3, 4 * q + (q + 1) % 4] = specials[q % 3]                       # in the objectness itself
        for p in range(0, P, 3):
            xb[3 + p % (ic - 3), p] = specials[(p // 3) % 3]                         # and in the inputs of every other row
    x.setflags(write=False)
    f.setflags(write=False)
    return x, f


def expected(obj_bits, P):
    """from the dense objectness bits (3, P): per quad 1 = some (pixel, anchor) passes decidedly, 0 = none can, -1 = it hangs on an undecided value"""
    bs = obj_bits.view(np.float32).astype(np.float64)
    t = float(np.float32(THRESH) * np.float32(0.999))
    with np.errstate(over="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-bs))
    sure_pass = np.isnan(s) | (s > t * (1 + 1e-5))          # (!(NaN < t) holds)
    sure_fail = s < t * (1 - 1e-5)
    anyp = sure_pass.reshape(3, P // 4, 4).any(axis=(0, 2))
    allf = sure_fail.reshape(3, P // 4, 4).all(axis=(0, 2))
    return np.where(anyp, 1, np.where(allf, 0, -1))


def run(capi, torch, P, ic, classes, case):
    N, iw, ih = PLANES[P]
    A = 5 + classes
    oc, nq = 3 * A, P // 4
    x, f = tensors(P, ic, classes, case)
    dx, df = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(f.copy()).cuda()
    g = 256
    buf = torch.full((2, g + oc * P + g), GUARD, dtype=torch.int32, device="cuda")
    buf[:, g:g + oc * P] = SENT
    dense, sparse = buf[0, g:g + oc * P], buf[1, g:g + oc * P]
    lst = torch.full((g + nq + g,), LSENT, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    if case == "overflow":
        cnt += nq + 5
    capi.groupconv_dev(dx.data_ptr(), df.data_ptr(), dense.data_ptr(), N, iw, ih, ic, 1, 0, 1, 1, oc, act=0, variant=capi.FFGPU.K_CONV_X3)
    capi.sparse_head_dev(dx.data_ptr(), df.data_ptr(), sparse.data_ptr(), N, iw, ih, ic, classes, THRESH, lst[g:].data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    hb = buf.cpu().numpy().view(np.uint32)
    assert (hb[:, :g] == GUARD).all() and (hb[:, g + oc * P:] == GUARD).all(), "guard words of the output overwritten"
    assert dx.cpu().numpy().tobytes() == x.tobytes() and df.cpu().numpy().tobytes() == f.tobytes(), "an input changed"
    hl = lst.cpu().numpy()
    assert (hl[:g] == LSENT).all() and (hl[g + nq:] == LSENT).all(), "guard words of the list overwritten"
    d = hb[0, g:g + oc * P].reshape(3, A, nq, 4)
    s = hb[1, g:g + oc * P].reshape(3, A, nq, 4)
    assert not (d == SENT).any(), "the dense launch left a value unwritten"
    return d, s, hl[g:g + nq], int(cnt.cpu()[0])


@pytest.mark.parametrize("classes", [1, 20, 80])
@pytest.mark.parametrize("ic", [8, 40, 120])
@pytest.mark.parametrize("P", [4, 68, 260])
def test_pair_against_dense(env, clean, P, ic, classes):
    capi, torch = env
    nq = P // 4
    for case in CASES:
        what = "P=%d ic=%d classes=%d case=%s" % (P, ic, classes, case)
        d, s, lst, cnt = run(capi, torch, P, ic, classes, case)
        assert np.array_equal(s[:, :5], d[:, :5]), what + ": box rows differ from the dense launch"
        want = expected(np.ascontiguousarray(d[:, 4]).reshape(3, nq * 4), P)
        if case == "overflow":
            # a counter above the capacity on entry: nothing is appended, the class pass takes every quad
            assert cnt > nq and (lst == LSENT).all(), what
            assert np.array_equal(s, d), what + ": the result is not complete"
            continue
        assert 0 <= cnt <= nq, what
        listed = lst[:cnt]
        assert (lst[cnt:] == LSENT).all(), what + ": list written behind the count"
        assert len(set(listed.tolist())) == cnt and (listed >= 0).all() and (listed < nq).all(), what + ": duplicates or indices outside the tensor"
        on = np.zeros(nq, bool)
        on[listed] = True
        assert on[want == 1].all(), what + ": a passing quad is not listed: %s" % np.nonzero((want == 1) & ~on)[0][:8]
        assert not on[want == 0].any(), what + ": a quad without a passing anchor is listed: %s" % np.nonzero((want == 0) & on)[0][:8]
        assert np.array_equal(s[:, 5:][:, :, on], d[:, 5:][:, :, on]), what + ": class rows of listed quads differ from the dense launch"
        assert (s[:, 5:][:, :, ~on] == SENT).all(), what + ": class rows written outside the list"
        # what each case is there for
        if case == "none":
            assert cnt == 0
        elif case == "all":
            assert cnt == nq
        elif case == "first":
            assert listed.tolist() == [0]
        elif case == "last":
            assert listed.tolist() == [nq - 1]
        elif case == "per_tile":
            assert sorted(listed.tolist()) == sorted(set(range(0, nq, 16)) | {nq - 1})
        elif case == "boundary":
            assert (want[np.arange(nq) % 5 == 3] == 0).all() and (want[np.arange(nq) % 5 == 4] == 1).all(), what + ": the decided values are not decided"
            assert (want[np.arange(nq) % 5 < 3] == -1).all(), what + ": the values one ulp from the boundary count as decided"


@pytest.mark.parametrize("mt", [1, 2, 4])
def test_row_blocks_per_wave(env, clean, mt):
    """the class pass at every MT the layer can be planned with (FFGPU_IGX3_MT; the dense launch follows it too), eight waves per workgroup included"""
    capi, torch = env
    clean.setenv("FFGPU_IGX3_MT", str(mt))
    for nw in ("4", "8"):
        clean.setenv("FFGPU_IGX3_NW", nw)
        d, s, lst, cnt = run(capi, torch, 260, 40, 20, "per_tile")
        on = np.zeros(65, bool)
        on[lst[:cnt]] = True
        assert sorted(lst[:cnt].tolist()) == [0, 16, 32, 48, 64]
        assert np.array_equal(s[:, :5], d[:, :5]) and np.array_equal(s[:, 5:][:, :, on], d[:, 5:][:, :, on]) and (s[:, 5:][:, :, ~on] == SENT).all()
