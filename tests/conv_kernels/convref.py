"""One convolution layer of conv.h, restated in float64 for tests/conv_kernels, and the error bound every fp32 kernel is held to against it.

  conv64    float64 throughout on the fp32 operands: per output the sum over input channel, tap row and tap column of w x with the taps outside the plane
            SKIPPED (conv-v0.c:7-31 does not multiply a padding zero: an Inf beside the border meets no 0 x Inf), then scale' * sum + bias', then the
            activation of the reference (utils.h:15-23: x > 0 ? x : 0, x > 0 ? x : 0.1f x, sigmoid, linear), then the optional residual add with its own
            activation (ffcnn.c:418-423).  It also returns sabs = sum |w x| over the same taps, per output.
  oracle32  the fp32 reference: orc.groupconv (and orc.shortcut) frame by frame.
  bound     the hard bound below.

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
