"""Every instantiation of the fused expand -> depthwise 3x3 -> project blocks (k_irb_thin, k_irbw, k_irbw2, k_irb) against the fp32 reference chain AND a float64
restatement of the block, one test per case of tests/irb_blocks/cases.py (at least two per key of ffgpu_irb_instantiations; tests/test_irb_blocks_ref.py holds
the table to that on the CPU).

Every case: the planner probe confirms the key inside the test; the output lies between guard rows of a fixed bit pattern in one allocation and starts as NaN;
after the launch the guards are unchanged bit for bit, inputs, weights and residual are unchanged, no output is unwritten, and a second launch into a fresh
buffer gives the same bits.

The error criterion has the reference chain as its yardstick, never the kernel: with E_ref = max |chain - float64| and E_k = max |kernel - float64| over the block,
    E_k <= 2 E_ref + 1e-6   and   E_k <= 8e-7 max |y| + 1e-6
(both from tests/test_gpu_round4.py::test_x3_fused_block_is_an_fp32_reorder, where they have held on hardware; E_ref is one summation order's sample of the same
rounding process, maximised over a few hundred to a few thousand outputs -- hence the factor).  cases.FACTOR holds the rows that need more than 2, if any.

The relu cases plant a NaN, a +Inf and a -Inf in the input, bias' = -Inf on one expanded channel and zero weights on the +Inf channel: relu(x) is x > 0 ? x : 0 in
the reference (utils.h:18), so relu(NaN) = relu(-Inf) = 0.  Expected, from the chain: the same NaN positions, equal +-Inf values, an exact 0 (either sign)
where the chain has 0, every other output within the criterion.

The single-layer kernels whose epilogues share the rule (pw_mfma, pw_gemm, conv_igemm, the dense first layer, dw_pair, pw_bf16, dwpw, and the split-bf16
pw_x3, pw_x3s, conv_x3, pw_x3t) are held to the generic
kernel on a NaN and a -Inf pre-activation, both planted through bias' so that they depend on no product.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import numpy as np
import pytest

from irb_blocks import blockref, cases
from irb_blocks.cases import CASES

pytestmark = pytest.mark.gpu

GUARD_BITS = 0x5A5AA5A5


@pytest.fixture(scope="module")
def env():
    import torch
    from ffcnn_amd import capi
    capi.lib()
    return capi, torch


def launch(capi, torch, c, r):
    """one launch of the block into a guarded, NaN-filled output: (the output as float32 bits, host) after the guards and the inputs have been checked"""
    N, W, H, ic, ec, oc, stride = c.shape
    OH, OW = blockref.out_dims(H, W, stride)
    n_out = oc * N * OH * OW
    guard = (2 * OH * OW + 63) & ~63                             # two planes of guard rows on either side
    host = [r["x"], r["f1"], r["fd"], r["f2"]] + ([r["res"]] if r["res"] is not None else [])
    dev = [torch.from_numpy(a.copy()).cuda() for a in host]
    buf = torch.full((guard + n_out + guard,), GUARD_BITS, dtype=torch.int32, device="cuda")
    out = buf[guard:guard + n_out].view(torch.float32)
    out.fill_(float("nan"))
    assert out.data_ptr() == buf.data_ptr() + 4 * guard
    capi.irb_dev(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr() if r["res"] is not None else None, out.data_ptr(),
                 N, W, H, ic, ec, oc, stride, *c.acts)
    torch.cuda.synchronize()
    bits = buf.cpu().numpy()
    assert (bits[:guard] == GUARD_BITS).all() and (bits[guard + n_out:] == GUARD_BITS).all(), "%s: guard rows overwritten" % c.id
    for d, h, name in zip(dev, host, ("input", "w1", "wd", "w2", "residual")):
        assert d.cpu().numpy().tobytes() == h.tobytes(), "%s: %s changed" % (c.id, name)
    return bits[guard:guard + n_out].copy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=cases.IDS)
def test_block(env, i, monkeypatch):
    capi, torch = env
    c = CASES[i]
    cases.set_switches(monkeypatch, c)
    assert cases.plan_line(capi.irb_plan_text, c).split(" ")[0] == c.key
    r = cases.reference(i)
    bits = launch(capi, torch, c, r)
    assert np.array_equal(bits, launch(capi, torch, c, r)), "%s: a second launch gives other bits" % c.id
    got = bits.view(np.float32).reshape(r["y32"].shape)
    y32, y64, ok = r["y32"], r["y64"], r["ok"]
    if c.kind == "relu":
        assert np.array_equal(np.isnan(got), np.isnan(y32)), "%s: NaN at %r, expected at %r" % (c.id, np.argwhere(np.isnan(got))[:4].tolist(), np.argwhere(np.isnan(y32))[:4].tolist())
        inf = np.isinf(y32)
        assert np.array_equal(got[inf], y32[inf]), "%s: +-Inf outputs differ" % c.id
        zero = y32 == 0
        assert (got[zero] == 0).all(), "%s: %d of the chain's %d exact zeros are not zero" % (c.id, int((got[zero] != 0).sum()), int(zero.sum()))
    else:
        assert not np.isnan(got).any(), "%s: unwritten outputs" % c.id
    assert np.isfinite(got[ok]).all(), c.id
    E_k = float(np.abs(got[ok] - y64[ok]).max())
    E_ref, ymax = r["E_ref"], r["ymax"]
    print("RATIO %s %s E_k %.3g E_ref %.3g ymax %.3g E_k/E_ref %.3f E_k/ymax %.3g" % (c.id, c.key, E_k, E_ref, ymax, E_k / max(E_ref, 1e-30), E_k / ymax))
    assert E_k <= cases.FACTOR.get(c.key, 2.0) * E_ref + 1e-6, (c.id, E_k, E_ref)
    assert E_k <= 8e-7 * ymax + 1e-6, (c.id, E_k, ymax)


# ---- the single-layer kernels whose epilogues share the relu rule, against the generic kernel (which follows utils.h:18)
def _conv(capi, torch, x, f, N, iw, ih, ic, groups, pad, stride, fs, fn, act, variant, flags=0):
    ow, oh = (iw + 2 * pad - fs) // stride + 1, (ih + 2 * pad - fs) // stride + 1
    dx, df = torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda()
    dy = torch.full((fn * N, oh, ow), float("nan"), device="cuda")
    capi.groupconv_dev(dx.data_ptr(), df.data_ptr(), dy.data_ptr(), N, iw, ih, ic, groups, pad, stride, fs, fn, act, flags, variant, None)
    torch.cuda.synchronize()
    return dy.cpu().numpy().reshape(fn, N, oh, ow)


def _same_zeros(got, ref, what, tol):
    """ref: the generic kernel under relu -- no NaN anywhere, exact zeros on the two planted channels; tol: relative, or an array of absolute bounds"""
    assert not np.isnan(ref).any() and (ref[0] == 0).all() and (ref[1] == 0).all() and (ref[2:] > 0).any(), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN outputs at %r" % (what, np.argwhere(np.isnan(got))[:4].tolist())
    assert (got[:2] == 0).all(), "%s: %d outputs of the two planted channels are not zero" % (what, int((got[:2] != 0).sum()))
    assert np.all(np.abs(got - ref) <= 1e-3 + (tol * np.abs(ref) if np.isscalar(tol) else tol)), "%s: max |d| %.3g" % (what, float(np.abs(got - ref).max()))


# (name kernel_name must give, variant, flags, switches, N, iw, ih, ic, groups, pad, stride, fs, fn, rtol): the smallest shape each kernel takes
SINGLE = [
    ("pw_mfma", "K_PW_MFMA", 0, {}, 1, 4, 3, 5, 1, 0, 1, 1, 6, 1e-3),
    ("pw_gemm", "K_PW_GEMM", 0, {}, 1, 4, 4, 64, 1, 0, 1, 1, 128, 1e-3),
    ("pw_bf16", "K_PW_BF16", 0, {}, 1, 4, 4, 64, 1, 0, 1, 1, 128, None),                    # (bf16 operands: the bound is worked out from them in the test)
    ("conv_igemm", "K_IGEMM", 0, {}, 1, 8, 5, 8, 1, 1, 1, 3, 8, 1e-3),                         # the vectorised gather (3x3, stride 1, whole quads)
    ("conv_igemm", "K_IGEMM", 0, {}, 2, 7, 5, 8, 1, 1, 2, 3, 8, 1e-3),                         # the general gather
    ("conv_igemm", "K_IGEMM", 0, {"FFGPU_IGEMM_SPLIT": "2"}, 1, 8, 5, 16, 1, 1, 1, 3, 8, 1e-3),   # split K: the activation moves into the reduction kernel
    ("pw_x3", "K_PW_X3", 0, {}, 1, 4, 3, 5, 1, 0, 1, 1, 6, 1e-3),                               # the split-bf16 kernels: pw_mfma's epilogue, and pw_x3t's own
    ("pw_x3s", "K_CONV_X3", 0, {}, 1, 4, 3, 8, 1, 0, 1, 1, 6, 1e-3),
    ("conv_x3", "K_CONV_X3", 0, {}, 1, 8, 5, 8, 1, 1, 1, 3, 8, 1e-3),
    ("pw_x3t", "K_PW_X3T", 0, {}, 1, 4, 3, 5, 1, 0, 1, 1, 6, 1e-3),
    ("conv_dense8", "K_DENSE_SMALL", 0, {"FFGPU_CONV_FIRST_MIN_PX": "1"}, 2, 8, 4, 3, 1, 1, 2, 3, 8, 1e-3),   # the first-layer form (k_conv_first), which a small batch gets only when asked
    ("dw_lds", "K_DW_LDS", 0, {}, 1, 6, 5, 4, 4, 2, 1, 5, 4, 1e-3),                            # 5x5 depthwise, even width 6..40, an even channel count: k_dw_pair
]


@pytest.mark.parametrize("case", SINGLE, ids=["%s-%d" % (s[0], n) for n, s in enumerate(SINGLE)])
def test_single_layer_relu_on_nan_and_minus_inf(env, case, monkeypatch):
    capi, torch = env
    name, variant, flags, switches, N, iw, ih, ic, groups, pad, stride, fs, fn, rtol = case
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    variant = getattr(capi.FFGPU, variant)
    assert capi.kernel_name(N, iw, ih, ic, groups, pad, stride, fs, fn, variant) == name
    rng = np.random.default_rng(len(name) + ic)
    x = rng.uniform(-1, 1, (ic * N, ih, iw)).astype(np.float32)
    K = fs * fs * (ic // groups)
    f = blockref.make_filter(rng, fn, K)
    k4 = (K + 3) & ~3
    f[2:, k4 + 1] = 3.0                                           # the other channels mostly positive: zeros elsewhere would hide nothing, but say little
    f[0, k4 + 1], f[1, k4 + 1] = -np.inf, np.nan
    ref = _conv(capi, torch, x, f, N, iw, ih, ic, groups, pad, stride, fs, fn, 1, capi.FFGPU.K_GENERIC)
    got = _conv(capi, torch, x, f, N, iw, ih, ic, groups, pad, stride, fs, fn, 1, variant, flags)
    if rtol is None:
        # both operands of every product rounded to the nearest bf16 (8 significant bits: relative error <= 2^-9 each, 2^-8 per product), fp32 accumulation:
        # |d| <= 2^-8 scale' sum |w| |x| per output
        aw, ax = np.abs(f[:, :K]).astype(np.float64), np.abs(x.reshape(ic, -1)).astype(np.float64)
        rtol = (2.0 ** -8 * np.abs(f[:, k4]).astype(np.float64)[:, None] * (aw @ ax)).reshape(ref.shape)
    _same_zeros(got, ref, name, rtol)


def test_dwpw_relu_on_nan_and_minus_inf(env):
    """depthwise 3x3 -> pointwise in one kernel (k_dwpw), relu after both: bias' = -Inf and NaN on two depthwise channels (zero into the pointwise layer, as in two
    generic launches) and on two output channels"""
    capi, torch = env
    N, W, H, Cn, OC = 2, 9, 7, 6, 5
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (Cn * N, H, W)).astype(np.float32)
    fd, fp = blockref.make_filter(rng, Cn, 9), blockref.make_filter(rng, OC, Cn)
    fd[0, 13], fd[1, 13] = -np.inf, np.nan
    fp[2:, ((Cn + 3) & ~3) + 1] = 3.0
    fp[0, ((Cn + 3) & ~3) + 1], fp[1, ((Cn + 3) & ~3) + 1] = -np.inf, np.nan
    mid = _conv(capi, torch, x, fd, N, W, H, Cn, Cn, 1, 1, 3, Cn, 1, capi.FFGPU.K_GENERIC)
    assert (mid[:2] == 0).all() and not np.isnan(mid).any()
    ref = _conv(capi, torch, np.ascontiguousarray(mid.reshape(Cn * N, H, W)), fp, N, W, H, Cn, 1, 0, 1, 1, OC, 1, capi.FFGPU.K_GENERIC)
    t = [torch.from_numpy(a).cuda() for a in (x, fd, fp)]
    out = torch.full((OC * N, H, W), float("nan"), device="cuda")
    capi.dwpw_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(), N, W, H, Cn, OC, 3, 1, 1)
    torch.cuda.synchronize()
    _same_zeros(out.cpu().numpy().reshape(OC, N, H, W), ref, "dwpw", 1e-3)
