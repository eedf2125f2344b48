"""Every stand-alone convolution kernel against a float64 restatement of the layer (convref.conv64), one test per case of tests/conv_kernels/cases.py; the
kernel is forced by its FFGPU_K_* id and ffgpu_groupconv_kernel_name must answer the declared name first.  tests/test_conv_kernels_ref.py holds the table, the
bound and the oracle to their purpose on the CPU.

Part A (test_error_bound, test_pair_error_bound), every fp32 kernel and the four split-bf16 kernels (pw_x3, pw_x3t, conv_x3, pw_x3s).  Both must hold:
    per output   |got - ref64| <= gamma(K + 3) (|scale'| sum |w x| + |bias'|)     the hard bound of convref: no correct fp32 evaluation can exceed it
                 split kernels: (gamma(6 K + 3) + 2^-21 + 2^-30 + 2^-38) (...)    convref.bound_x3: six exact partial products per product, three dropped
    per case     E_k <= 2 E_ref + 1e-6  and  E_k <= 8e-7 max |y| + 1e-6            blockref.criterion, E_ref = max |oracle - ref64| the yardstick (cases.FACTOR holds
                                                                                  the kernels that need more than 2, if any, with the measured ratio)
The output lies between guard words in one allocation and starts as NaN: the guards are unchanged, no output is unwritten, inputs and weights are unchanged.  The
two forms of the first layer (k_conv_dense8, k_conv_first) are compared bit for bit.

Part B (test_non_finite_inputs, test_pair_non_finite_inputs), every conv kernel including pw_bf16: +Inf, -Inf and NaN among the inputs where each kernel's
addressing can go wrong (cases.placements), under every activation the kernel takes.  The NaN pattern equals conv64's, every other touched output -- +-Inf, or the
exact 0 / 1 that relu and the sigmoid make of -Inf, NaN and +-Inf (utils.h:15-23) -- is EQUAL to it, and every untouched output is finite and within the part A
bound (pw_bf16: its own 2^-7 bound): nothing leaks into a neighbour's sum, a zero-weight padded k-slot included.  A split kernel's case runs once more without
the planted values: every untouched output keeps its bits (the Inf form of the split is chosen per wave and must not show in a neighbour's finite values).

Part C (test_fused_residual, test_fused_residual_non_finite*): the epilogue act2(act(conv) + residual), reached through an executor whose fused plan absorbs the shortcut into the conv in front of it.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import numpy as np
import pytest

from conv_kernels import cases, convref
from conv_kernels.cases import CASES, NF_CASES, PAIRS, NF_PAIRS
from irb_blocks import blockref

pytestmark = pytest.mark.gpu

GUARD_BITS = 0x5A5AA5A5
GUARD = 256


@pytest.fixture(scope="module")
def env():
    import torch
    from ffcnn_amd import capi
    capi.lib()
    return capi, torch


def _guarded(torch, n_out):
    buf = torch.full((GUARD + n_out + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + n_out].view(torch.float32)
    out.fill_(float("nan"))
    return buf, out


def _collect(torch, buf, n_out, dev, host, what):
    torch.cuda.synchronize()
    bits = buf.cpu().numpy()
    assert (bits[:GUARD] == GUARD_BITS).all() and (bits[GUARD + n_out:] == GUARD_BITS).all(), "%s: guard words overwritten" % what
    for d, h in zip(dev, host):
        assert d.cpu().numpy().tobytes() == h.tobytes(), "%s: an operand changed" % what
    return bits[GUARD:GUARD + n_out].copy().view(np.float32)


def launch(capi, torch, c, x, f):
    """one launch of the case's kernel: (oc, N, OH, OW) float32"""
    N, W, H, ic, groups, pad, stride, fs, oc, OH, OW, K = cases.dims(c)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (x, f)]
    buf, out = _guarded(torch, oc * N * OH * OW)
    capi.groupconv_dev(dev[0].data_ptr(), dev[1].data_ptr(), out.data_ptr(), N, W, H, ic, groups, pad, stride, fs, oc, c.act, c.flags, getattr(capi.FFGPU, c.variant), None)
    return _collect(torch, buf, oc * N * OH * OW, dev, (x, f), c.id).reshape(oc, N, OH, OW)


def launch_pair(capi, torch, p, x, fd, fp):
    N, W, H, C, OC = p.shape
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (x, fd, fp)]
    buf, out = _guarded(torch, OC * N * H * W)
    capi.dwpw_dev(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), out.data_ptr(), N, W, H, C, OC, p.fs, p.actd, p.actp)
    return _collect(torch, buf, OC * N * H * W, dev, (x, fd, fp), p.id).reshape(OC, N, H, W)


def assert_error(what, kernel, got, r, ok=None):
    """both conditions of part A over the outputs `ok` (default: all)"""
    ok = np.ones(got.shape, bool) if ok is None else ok
    assert np.isfinite(got[ok]).all(), "%s: %d outputs are not finite (unwritten, or a non-finite value leaked into them)" % (what, int((~np.isfinite(got[ok])).sum()))
    d = np.abs(got[ok].astype(np.float64) - r["y64"][ok])
    used = float((d / r["bound"][ok]).max())
    E_k, E_ref, ymax = float(d.max()), r["E_ref"], r["ymax"]
    print("RATIO %s %s E_k %.3g E_ref %.3g ymax %.3g E_k/E_ref %.3f bound used %.3f" % (what, kernel, E_k, E_ref, ymax, E_k / max(E_ref, 1e-30), used))
    assert (d <= r["bound"][ok]).all(), "%s: %.3g of the hard bound at %r" % (what, used, np.argwhere(ok)[int(np.argmax(d / r["bound"][ok]))].tolist())
    assert blockref.criterion(E_k, E_ref, ymax, cases.FACTOR.get(kernel, 2.0)), (what, E_k, E_ref, ymax)


def assert_non_finite(what, got, r, inf_only=False):
    """part B: NaN where conv64 has NaN, every other touched output EQUAL to conv64's (+-Inf, or the exact 0 / 1 of relu and the sigmoid; inf_only: the pair, whose
    touched outputs can be ordinary numbers again behind a relu in the middle -- those are held to the bound)"""
    y64, t = r["y64"], r["touched"] & (np.isinf(r["y64"]) | (not inf_only))
    nan = np.isnan(y64)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN at %r, expected at %r" % (what, np.argwhere(np.isnan(got) & ~nan)[:4].tolist(), np.argwhere(nan & ~np.isnan(got))[:4].tolist())
    sel = t & ~nan
    assert np.array_equal(got[sel], y64[sel].astype(np.float32)), "%s: touched outputs differ at %r" % (what, np.argwhere(sel & (got != y64.astype(np.float32)))[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("i", range(len(CASES)), ids=cases.IDS)
def test_error_bound(env, i, monkeypatch):
    capi, torch = env
    c, r = CASES[i], cases.reference(i)
    cases.set_switches(monkeypatch, c)
    assert cases.kernel_name(capi, c) == c.name
    got = launch(capi, torch, c, r["x"], r["f"])
    assert_error(c.id, c.kernel, got, r)
    if c.kernel == "conv_first":
        for k, v in cases.DENSE.items():
            monkeypatch.setenv(k, v)
        assert np.array_equal(got.view(np.uint32), launch(capi, torch, c, r["x"], r["f"]).view(np.uint32)), "%s: k_conv_first and k_conv_dense8 differ" % c.id


@pytest.mark.parametrize("i", range(len(PAIRS)), ids=[p.id for p in PAIRS])
def test_pair_error_bound(env, i):
    capi, torch = env
    p, r = PAIRS[i], cases.pair_reference(i)
    assert_error(p.id, "dwpw", launch_pair(capi, torch, p, r["x"], r["fd"], r["fp"]), r)


# ---------------------------------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("i", range(len(NF_CASES)), ids=cases.NF_IDS)
def test_non_finite_inputs(env, i, monkeypatch):
    capi, torch = env
    c, r = NF_CASES[i], cases.nf_reference(i)
    cases.set_switches(monkeypatch, c)
    assert cases.kernel_name(capi, c) == c.name
    lin, t = r["lin64"], r["touched"]
    assert not np.isfinite(lin[t]).any() and np.isfinite(lin[~t]).all(), "test set-up: every touched output is non-finite in the reference, no other is"
    assert cases.classes(lin) == {"nan", "+inf", "-inf"}, "test set-up: %r" % (cases.classes(lin),)
    got = launch(capi, torch, c, r["x"], r["f"])
    ok = r["ok"]
    leaked = ok & ~np.isfinite(got)
    assert not leaked.any(), "%s: a non-finite value leaked into %d untouched outputs, first at %r" % (c.id, int(leaked.sum()), np.argwhere(leaked)[:4].tolist())
    assert_non_finite(c.id, got, r)
    if c.kernel == "pw_bf16":
        # its own bound (tests/test_gpu_kernels.py::test_pw_bf16): two roundings of relative size 2^-9 per product, worst case, on top of the fp32 bound
        K = c.shape[3]
        k4 = (K + 3) & ~3
        b = 2.0 ** -7 * np.abs(r["f"][:, k4].astype(np.float64))[:, None, None, None] * r["sabs"] + 1e-5 + r["bound"]
        assert (np.abs(got[ok].astype(np.float64) - r["y64"][ok]) <= b[ok]).all(), c.id
    else:
        assert_error(c.id, c.kernel, got, r, ok)
    if c.kernel in cases.X3:
        # the split kernels take the Inf form of the split per WAVE; for a finite value it computes the same three parts, so the same case WITHOUT the planted
        # values must give every untouched output the same bits: a wave-level choice that leaks into its neighbours shows here
        clean = launch(capi, torch, c, r["x0"], r["f"])
        assert np.isfinite(clean).all(), c.id
        diff = ok & (clean.view(np.uint32) != got.view(np.uint32))
        assert not diff.any(), "%s: %d untouched outputs change their bits with the planted values, first at %r" % (c.id, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("i", range(len(NF_PAIRS)), ids=[p.id for p in NF_PAIRS])
def test_pair_non_finite_inputs(env, i):
    capi, torch = env
    p, r = NF_PAIRS[i], cases.pair_reference(i, True)
    assert not np.isfinite(r["lin64"][r["touched"]]).any() and np.isfinite(r["lin64"][~r["touched"]]).all()
    got = launch_pair(capi, torch, p, r["x"], r["fd"], r["fp"])
    assert_non_finite(p.id, got, r, inf_only=True)
    assert_error(p.id, "dwpw", got, r, r["ok"])


# ---------------------------------------------------------------------------------------------------------------------------- part C
def _run_res(capi, orc, tmp_path, monkeypatch, row, made, frames):
    """one forward of the fused plan: (x, f, res, got) -- the executor's OWN copies of the conv's input and of the residual, the conv's filter rows, the shortcut
    layer's tensor, CNHW -- after the plan and the dispatcher have been held to the case"""
    from test_gpu_parity import _write_random_weights
    name, kernel, env, batch, w, h, ic, oc, size, groups, act = row
    g, a, b, c, s = made
    stride = cases.RES_STRIDE.get(name, 1)
    for k in cases.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in cases.SWITCHES, k
        monkeypatch.setenv(k, v)
    assert capi.kernel_name(batch, w, h, ic, groups, size // 2, stride, size, oc) == kernel
    cfg, wts = str(tmp_path / (g.name + ".cfg")), str(tmp_path / (g.name + ".weights"))
    with open(cfg, "w") as fp:
        fp.write(g.cfg_text())
    o = orc.Oracle(cfg=cfg, weights=None)
    _write_random_weights(wts, o, 3 + len(g.name))
    o.close()
    o = orc.Oracle(cfg=cfg, weights=wts)
    f = o.filter_rows(c).copy()
    o.close()
    with capi.Net(cfg, wts) as net:
        with net.executor(batch, capi.FFGPU.KEEP_ALL) as ex:
            model = [lay for lay, _ in ex.step_model()]
            assert s not in model and c in model, "%s: the shortcut (layer %d) has a launch of its own, or its conv (layer %d) has none: %s" % (name, s, c, model)
            assert [lay for lay in model if lay >= 0] == g.steps[True], (name, model)
            ex.forward_host(frames)
            x, res, got = (np.stack([ex.read_layer(lay, n) for n in range(batch)], 1) for lay in (b, a, s))
        with net.executor(batch, capi.FFGPU.KEEP_ALL | capi.FFGPU.NO_FUSE) as ex:
            model = [lay for lay, _ in ex.step_model()]
            assert s in model and [lay for lay in model if lay >= 0] == g.steps[False], (name, model)
    return x.reshape(ic * batch, h, w), f, res.reshape(oc * batch, h // stride, w // stride), got


@pytest.mark.parametrize("row", cases.RES_TABLE, ids=cases.RES_IDS)
def test_fused_residual(env, orc, tmp_path, monkeypatch, row):
    """act2(conv + residual) inside the conv's launch against conv64(..., res, res_act) on the executor's own operands, both conditions of part A"""
    capi, torch = env
    name, kernel, _, batch, w, h, ic, oc, size, groups, act = row
    made = cases.res_cfg(row)
    rng = np.random.default_rng(len(name))
    frames = rng.uniform(-1, 1, (batch, 3, h, w)).astype(np.float32)
    x, f, res, got = _run_res(capi, orc, tmp_path, monkeypatch, row, made, frames)
    ra, K, stride = {"linear": 0, "relu": 1, "leaky": 2}[act], size * size * ic // groups, cases.RES_STRIDE.get(name, 1)
    y64, sabs = convref.conv64(x, f, batch, w, h, ic, groups, size // 2, stride, size, 0, res, ra)
    pre, _ = convref.conv64(x, f, batch, w, h, ic, groups, size // 2, stride, size, 0)
    y32 = convref.oracle32(orc, x, f, batch, w, h, ic, groups, size // 2, stride, size, 0, res, ra)
    bound = convref.bound_x3 if kernel in cases.X3 else convref.bound
    r = dict(y64=y64, bound=bound(f, K, sabs, 0, pre, res, ra), E_ref=float(np.abs(y32 - y64).max()), ymax=float(np.abs(y64).max()))
    assert (np.abs(y32 - y64) <= r["bound"]).all(), "%s: the oracle misses the bound" % name
    assert_error("residual-" + name, kernel, got, r)


def _residual_non_finite(capi, orc, tmp_path, monkeypatch, row, planted):
    """+Inf, -Inf and NaN in the frame (planted: the three pixels) reach both sides of the add: +Inf + -Inf = NaN where the residual and the conv disagree in sign, and
    the relu shortcut makes 0 of it, of every NaN and of every -Inf (utils.h:18) -- NaN pattern (none is left), +Inf and the exact zeros equal to conv64's, the
    untouched pixels within the bound"""
    name, kernel, _, batch, w, h, ic, oc, size, groups, act = row
    rng = np.random.default_rng(11)
    frames = rng.uniform(-1, 1, (batch, ic, h, w)).astype(np.float32)
    (y0, x0), (y1, x1), (y2, x2) = planted
    frames[0, 0, y0, x0], frames[0, ic - 1, y1, x1], frames[0, ic // 2, y2, x2] = np.inf, -np.inf, np.nan
    x, f, res, got = _run_res(capi, orc, tmp_path, monkeypatch, row, cases.res_nf_cfg(row), frames)
    # (the net input itself: its bytes; the average pool's copy of it: its values, a NaN for the NaN)
    assert x.tobytes() == frames[0].tobytes() if row is cases.RES_NF else np.array_equal(x, frames[0], equal_nan=True), "%s: the conv does not read the planted frame" % name
    pad, K = size // 2, size * size * ic
    y64, sabs = convref.conv64(x, f, batch, w, h, ic, 1, pad, 1, size, 0, res, 1)
    pre, _ = convref.conv64(x, f, batch, w, h, ic, 1, pad, 1, size, 0)
    r64 = res.reshape(pre.shape).astype(np.float64)
    t = np.zeros(y64.shape, bool)
    for y, xx in planted:
        t[:, 0, max(0, y - pad):y + pad + 1, max(0, xx - pad):xx + pad + 1] = True
    with np.errstate(invalid="ignore"):
        lin = pre + r64
    # set-up: the residual holds +Inf where the conv holds -Inf (and the other way round), both hold NaN at the third pixel; every touched sum is non-finite, all three kinds
    assert (np.isposinf(r64) & np.isneginf(pre)).any() and (np.isneginf(r64) & np.isposinf(pre)).any() and (np.isnan(r64) & np.isnan(pre)).any()
    assert not np.isfinite(lin[t]).any() and np.isfinite(lin[~t]).all() and cases.classes(lin) == {"nan", "+inf", "-inf"}
    assert not np.isnan(y64).any() and (y64[t] == 0).any() and np.isposinf(y64[t]).any() and np.isin(y64[t], (0.0, np.inf)).all()
    bound = convref.bound_x3 if kernel in cases.X3 else convref.bound
    r = dict(y64=y64, touched=t, bound=bound(f, K, sabs, 0, pre, res, 1), E_ref=0.0, ymax=0.0)
    assert_non_finite(name, got, r)
    ok = ~t
    y32 = convref.oracle32(orc, x, f, batch, w, h, ic, 1, pad, 1, size, 0, res, 1)
    r["E_ref"], r["ymax"] = float(np.abs(y32[ok] - y64[ok]).max()), float(np.abs(y64[ok]).max())
    assert_error("residual-" + name, kernel, got, r, ok)


def test_fused_residual_non_finite(env, orc, tmp_path, monkeypatch):
    """k_pw_mfma's epilogue: the conv reads the net input, the residual is a 1x1 conv of it"""
    _residual_non_finite(env[0], orc, tmp_path, monkeypatch, cases.RES_NF, ((2, 3), (4, 7), (5, 9)))


def test_fused_residual_non_finite_conv_x3(env, orc, tmp_path, monkeypatch):
    """k_conv_x3's scalar epilogue at width 13: three 3x3 windows apart from each other, the last one in the overlapping last quad of its rows.  The residual is
    non-finite in the middle of a window only: around it a finite residual meets +-Inf or NaN from the conv"""
    _residual_non_finite(env[0], orc, tmp_path, monkeypatch, cases.RES_NF_X3, ((2, 3), (4, 7), (5, 11)))
