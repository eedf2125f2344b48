"""One convolution layer of conv.h, restated in float64 for tests/conv_kernels, and the error bound every fp32 kernel is held to against it.

  conv64    float64 throughout on the fp32 operands: per output the sum over input channel, tap row and tap column of w x with the taps outside the plane
            SKIPPED (conv-v0.c:7-31 does not multiply a padding zero: an Inf beside the border meets no 0 x Inf), then scale' * sum + bias', then the
            activation of the reference (utils.h:15-23: x > 0 ? x : 0, x > 0 ? x : 0.1f x, sigmoid, linear), then the optional residual add with its own
            activation (ffcnn.c:418-423).  It also returns sabs = sum |w x| over the same taps, per output.
  oracle32  the fp32 reference: orc.groupconv (and orc.shortcut) frame by frame.
  bound     the hard bound below; bound_x3: the same for the split-bf16 kernels (its derivation stands in front of it).
  model_x3  a numpy model of the split kernels' arithmetic: what tests/test_conv_kernels_ref.py shows the criterion to tell from a kernel that forgets a term.

Tensors are CNHW as the kernels take them, (channels * N, H, W); filters are conv.h rows (blockref.make_filter).

THE BOUND.  u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a sum of K products evaluated in fp32 in ANY
order, with or without fused multiply-adds, partial sums, split-K reductions or matrix-core chains, differs from the exact sum by at most gamma(K) sum |w x|:
every product carries at most one rounding and takes part in at most K - 1 additions).  With K = fs^2 ic / groups roundings for the sum, one for the affine step
scale' * sum + bias' (one if fused, two if not: the spare), one for the leaky product:
    |got - ref64| <= gamma(K + 3) (|scale'| sabs + |bias'|)
Relu, leaky and the identity are 1-Lipschitz, so the bound passes through them.  The sigmoid has slope <= 1/4, and its own evaluation (a double exp rounded
to float, one fp32 add, one fp32 divide: utils.h:21) stays within 4 u of the exact value, which is < 1:
    |got - ref64| <= gamma(K + 3) (|scale'| sabs + |bias'|) / 4 + 4 u
A residual adds one rounding of v + r and one of the second leaky product, on a value of size at most |pre| + |res| (pre: the activated conv output):
    ... + gamma(2) (|pre| + |res|)            (the second activation is 1-Lipschitz again; a sigmoid there: a quarter of everything + 4 u)
This is derived, not measured: a correct fp32 evaluation cannot exceed it, a kernel that drops below fp32 anywhere (bf16 operands: 2^-9 per product) does by
orders of magnitude.  tests/test_conv_kernels_ref.py holds the oracle to it for every case, so a wrong bound or a wrong conv64 shows without a GPU."""
import numpy as np

from irb_blocks import blockref

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def out_dims(H, W, pad, stride, fs):
    return (H + 2 * pad - fs) // stride + 1, (W + 2 * pad - fs) // stride + 1


def act64(v, act):
    if act == 3:
        with np.errstate(over="ignore", invalid="ignore"):
            return 1.0 / (1.0 + np.exp(-v))
    return blockref.act64(v, act)


def conv64(x, f, N, W, H, ic, groups, pad, stride, fs, act, res=None, res_act=0, compat_v6=0):
    """(y, sabs), both (oc, N, OH, OW) float64.  compat_v6: the defect of conv-v6.c:422-441 as the oracle restates it (depthwise 5x5 s1 p2: output row
    OH - 2 never reads tap row 0)."""
    oc = f.shape[0]
    gic, goc = ic // groups, oc // groups
    K = fs * fs * gic
    k4 = (K + 3) & ~3
    OH, OW = out_dims(H, W, pad, stride, fs)
    v6 = bool(compat_v6) and pad == 2 and fs == 5 and stride == 1 and gic == 1 and OH > 2
    x64 = x.reshape(ic, N, H, W).astype(np.float64)
    w64 = f[:, :K].astype(np.float64).reshape(oc, gic, fs, fs)
    s, sabs = np.zeros((oc, N, OH, OW)), np.zeros((oc, N, OH, OW))
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(fs):
            for kx in range(fs):
                # index only what is inside the plane
                ys = [y for y in range(OH) if 0 <= y * stride - pad + ky < H and not (v6 and y == OH - 2 and ky == 0)]
                xs = [c for c in range(OW) if 0 <= c * stride - pad + kx < W]
                if not ys or not xs:
                    continue
                yi = np.array(ys)
                src = x64[:, :, yi * stride - pad + ky][:, :, :, xs[0] * stride - pad + kx:xs[-1] * stride - pad + kx + 1:stride]
                xi = np.arange(xs[0], xs[-1] + 1)
                for g in range(groups):
                    w = w64[g * goc:(g + 1) * goc, :, ky, kx]
                    sg = src[g * gic:(g + 1) * gic].reshape(gic, -1)                                      # 0 x Inf = NaN in the product, as in the reference
                    s[g * goc:(g + 1) * goc, :, yi[:, None], xi[None, :]] += (w @ sg).reshape(goc, N, len(ys), len(xs))
                    sabs[g * goc:(g + 1) * goc, :, yi[:, None], xi[None, :]] += (np.abs(w) @ np.abs(sg)).reshape(goc, N, len(ys), len(xs))
        sc, bi = f[:, k4].astype(np.float64)[:, None, None, None], f[:, k4 + 1].astype(np.float64)[:, None, None, None]
        y = act64(sc * s + bi, act)
        if res is not None:
            y = act64(y + res.reshape(oc, N, OH, OW).astype(np.float64), res_act)
    return y, sabs


def bound(f, K, sabs, act, pre=None, res=None, res_act=0):
    """the hard bound of the module docstring, per output; pre = conv64 without the residual (needed only with one)"""
    k4 = (K + 3) & ~3
    sc, bi = np.abs(f[:, k4].astype(np.float64))[:, None, None, None], np.abs(f[:, k4 + 1].astype(np.float64))[:, None, None, None]
    b = gamma(K + 3) * (sc * sabs + bi)
    if act == 3:
        b = b / 4 + 4 * U
    if res is not None:
        b = b + gamma(2) * (np.abs(pre) + np.abs(res.reshape(pre.shape).astype(np.float64)))
        if res_act == 3:
            b = b / 4 + 4 * U
    return b


# ---- the split-bf16 ("X3") kernels: k_pw_x3, k_pw_x3t, k_conv_x3 (conv_x3 and its pointwise form pw_x3s)
# THE SPLIT BOUND.  Every operand is cut by truncation into three bf16 parts, v = v0 + v1 + v2 exactly, all with the sign of v.  For 2^e <= |v| < 2^(e+1) a bf16
# keeps 8 significand bits, so |v1| <= |v - v0| < 2^(e-7) <= 2^-7 |v| and |v2| < 2^-15 |v|.  The kernels keep the six partial products w_i x_j with i + j <= 2 and
# drop D = w1 x2 + w2 x1 + w2 x2:
#     |D| < (2^-7 2^-15 + 2^-15 2^-7 + 2^-15 2^-15) |w x| = (2^-21 + 2^-30) |w x|        (X3_DROPPED; reached to within 3 %: w = x = 1 + 2^-7 - 2^-23 drops 2^-21.03 |w x|)
# A zero part of a non-zero weight is packed as sign(w) 2^(e-40) (so that an Inf input meets no 0 x Inf): at most two parts, 2^-39 |w x| together, on both the
# value of the sum of the kept terms and its sum of magnitudes.  Every bf16 x bf16 product is exact in fp32 (8 x 8 significand bits), the kept terms of one product
# have one sign and add up to at most (1 + 2^-39) |w x|, and the matrix cores add the 6 K exact terms in fp32 in SOME order (padded k-slots add exact zeros):
#     |sum_kernel - sum_kept| <= gamma(6 K) (1 + 2^-39) sum |w x|
# With the affine step, the leaky product and the spare of the fp32 bound, and 2^-38 for the perturbation and every cross term (gamma x 2^-39, gamma(3) x 2^-21):
#     |got - ref64| <= (gamma(6 K + 3) + 2^-21 + 2^-30 + 2^-38) (|scale'| sabs + |bias'|)
# and from there on (sigmoid, residual) as the fp32 bound.  That is (6 K + 11) / (K + 3) times the fp32 bound -- 5.4 times at K = 8, six times for a long K: the
# dropped terms are worth eight roundings (2^-21 = 8 u) whatever K is.  Derived, not measured; the oracle and the numpy model below are held to it on the CPU.
# It grows like K sum |w x| and a forgotten 2^-16-sized term hides under it from K of about 16 up: what tells a subtly wrong kernel from a right one is the
# criterion against E_ref (tests/test_conv_kernels_ref.py holds the model with one such term left out to FAIL it on every case).
X3_DROPPED = 2.0 ** -21 + 2.0 ** -30
X3_SLACK = 2.0 ** -38


def bound_x3(f, K, sabs, act, pre=None, res=None, res_act=0):
    """the hard bound of a split-bf16 kernel, per output (bound() with the split form's constant)"""
    k4 = (K + 3) & ~3
    sc, bi = np.abs(f[:, k4].astype(np.float64))[:, None, None, None], np.abs(f[:, k4 + 1].astype(np.float64))[:, None, None, None]
    b = (gamma(6 * K + 3) + X3_DROPPED + X3_SLACK) * (sc * sabs + bi)
    if act == 3:
        b = b / 4 + 4 * U
    if res is not None:
        b = b + gamma(2) * (np.abs(pre) + np.abs(res.reshape(pre.shape).astype(np.float64)))
        if res_act == 3:
            b = b / 4 + 4 * U
    return b


def _trunc16(v):
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def split3(v, weights=False):
    """the truncation split of the kernels (tools/sim_split_bf16.py has the same one): three float32 arrays, each a bf16 number, v0 + v1 + v2 == v exactly.
    weights: a zero part of a non-zero weight of exponent e >= 41 (biased) becomes sign(w) 2^(e-40), as irbw_x3_part packs it"""
    v = np.ascontiguousarray(v, np.float32)
    p0 = _trunc16(v)
    with np.errstate(invalid="ignore"):
        r = (v - p0).astype(np.float32)
        p1 = _trunc16(r)
        p2 = (r - p1).astype(np.float32)
    if weights:
        u = v.view(np.uint32)
        ex = (u >> np.uint32(23)) & np.uint32(0xff)
        tiny = (((u >> np.uint32(16)) & np.uint32(0x8000)) | ((ex.astype(np.int64) - 40).clip(0).astype(np.uint32) << np.uint32(7))) << np.uint32(16)
        for p in (p1, p2):
            z = ((p.view(np.uint32) & np.uint32(0x7fff0000)) == 0) & (ex >= 41) & (ex != 255)
            p.view(np.uint32)[z] = tiny[z]
    return p0, p1, p2


X3_TERMS = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))            # (weight part, input part) in the kernels' order: the small terms first
X3_SMALL = ((2, 0), (1, 1), (0, 2))                                    # the three 2^-16-sized ones


def x3_steps(kernel, ic, fs):
    """the k-steps of a split kernel as lists of (channel, ky, kx): what one MFMA chain link adds at once.  k_pw_x3: 32 channels; k_pw_x3t: 16; k_conv_x3: a group
    is four k-units (8 channels, tap row ky) in a row and one k-step per tap column kx"""
    if kernel == "pw_x3":
        return [[(c, 0, 0) for c in range(s, min(s + 32, ic))] for s in range(0, ic, 32)]
    if kernel == "pw_x3t":
        return [[(c, 0, 0) for c in range(s, min(s + 16, ic))] for s in range(0, ic, 16)]
    assert kernel in ("pw_x3s", "conv_x3") and ic % 8 == 0
    units = [(cb, ky) for cb in range(ic // 8) for ky in range(fs)]
    return [[(8 * cb + j, ky, kx) for cb, ky in units[g:g + 4] for j in range(8)] for g in range(0, len(units), 4) for kx in range(fs)]


def model_x3(kernel, x, f, N, W, H, ic, pad, stride, fs, act, drop=None):
    """a numpy model of the split kernels' arithmetic, (oc, N, OH, OW) float32: truncation split of both operands, the six kept terms in the kernels' order,
    every k-step's 32 (16) exact products added exactly and the accumulator rounded to fp32 once per (k-step, term) -- the matrix cores' own order inside
    a k-step is not modelled -- then fp32 scale' * sum + bias' and the activation.  drop = (weight part, input part): the model of a kernel that forgets that term."""
    oc = f.shape[0]
    K = fs * fs * ic
    k4 = (K + 3) & ~3
    OH, OW = out_dims(H, W, pad, stride, fs)
    xp = np.zeros((ic, N, H + 2 * pad, W + 2 * pad), np.float32)
    xp[:, :, pad:pad + H, pad:pad + W] = x.reshape(ic, N, H, W)
    xs = [p.astype(np.float64) for p in split3(xp)]
    ws = [p.astype(np.float64).reshape(oc, ic, fs, fs) for p in split3(f[:, :K], weights=True)]
    acc = np.zeros((oc, N * OH * OW), np.float32)
    for step in x3_steps(kernel, ic, fs):
        ci, ky, kx = (np.array(v) for v in zip(*step))
        cols = [p[ci[:, None, None, None], np.arange(N)[None, :, None, None], (np.arange(OH) * stride)[None, None, :, None] + ky[:, None, None, None],
                  (np.arange(OW) * stride)[None, None, None, :] + kx[:, None, None, None]].reshape(len(step), -1) for p in xs]
        rows = [p[:, ci, ky, kx] for p in ws]
        for wp, xq in X3_TERMS:
            if (wp, xq) != drop:
                acc = (acc.astype(np.float64) + rows[wp] @ cols[xq]).astype(np.float32)
    sc, bi = f[:, k4][:, None], f[:, k4 + 1][:, None]
    v = (acc.astype(np.float64) * sc.astype(np.float64) + bi.astype(np.float64)).astype(np.float32)      # one fused multiply-add
    if act == 3:
        v = (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(np.float32)
    elif act:
        v = np.where(v > 0, v, (np.float32(0.1) * v if act == 2 else np.float32(0.0))).astype(np.float32)
    return v.reshape(oc, N, OH, OW)


def pair64(x, fd, fp, N, W, H, C, fs, actd, actp):
    """the fused depthwise fs x fs (stride 1, same padding) -> pointwise pair: two calls of conv64, and the pair's bound.  The pointwise layer reads a middle
    tensor that is itself off by at most b1 (its own bound; the rounding of the middle tensor to fp32 is the affine rounding b1 already counts), so with
    m = |mid| + b1:   |got - ref64| <= gamma(C + 3) (|scale'| sum |w| m + |bias'|) + |scale'| sum |w| b1"""
    mid, sabs1 = conv64(x, fd, N, W, H, C, C, fs // 2, 1, fs, actd)
    b1 = bound(fd, fs * fs, sabs1, actd)
    b1 = np.where(np.isfinite(mid) & ~np.isfinite(b1), 0.0, b1)          # relu(NaN) = relu(-Inf) = 0 and sigmoid(+-Inf) = 1 / 0 are exact
    midc = mid.reshape(C * N, H, W)
    y, _ = conv64(midc, fp, N, W, H, C, 1, 0, 1, 1, actp)
    aw = np.abs(fp[:, :C].astype(np.float64))
    k4 = (C + 3) & ~3
    sc, bi = np.abs(fp[:, k4].astype(np.float64))[:, None, None, None], np.abs(fp[:, k4 + 1].astype(np.float64))[:, None, None, None]
    with np.errstate(invalid="ignore"):
        m = np.einsum("oc,cnhw->onhw", aw, np.abs(mid) + b1)
        p = np.einsum("oc,cnhw->onhw", aw, b1)
    b = gamma(C + 3) * (sc * m + bi) + sc * p
    if actp == 3:
        b = b / 4 + 4 * U
    return y, b


def oracle32(orc, x, f, N, W, H, ic, groups, pad, stride, fs, act, res=None, res_act=0, compat_v6=0):
    """(oc, N, OH, OW) float32: orc.groupconv and orc.shortcut, one frame at a time"""
    oc = f.shape[0]
    OH, OW = out_dims(H, W, pad, stride, fs)
    xf = x.reshape(ic, N, H, W)
    rf = None if res is None else res.reshape(oc, N, OH, OW)
    out = np.empty((oc, N, OH, OW), np.float32)
    for n in range(N):
        o = orc.groupconv(np.ascontiguousarray(xf[:, n]), f, groups, pad, stride, fs, act, compat_v6)
        if rf is not None:
            o = orc.shortcut(o, np.ascontiguousarray(rf[:, n]), res_act)
        out[:, n] = o
    return out


def pair32(orc, x, fd, fp, N, W, H, C, fs, actd, actp):
    OC = fp.shape[0]
    xf = x.reshape(C, N, H, W)
    out = np.empty((OC, N, H, W), np.float32)
    for n in range(N):
        out[:, n] = orc.groupconv(orc.groupconv(np.ascontiguousarray(xf[:, n]), fd, C, fs // 2, 1, fs, actd), fp, 1, 0, 1, 1, actp)
    return out
