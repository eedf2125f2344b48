"""The fused expand -> depthwise 3x3 -> project [+ shortcut] block, restated twice for tests/irb_blocks:

  block64   float64 throughout: three stages of scale' * sum(w x) + bias' on the fp32 operands, each followed by the activation of the reference
            (utils.h:15-23: relu is x > 0 ? x : 0, so relu(NaN) = relu(-Inf) = 0; leaky is x > 0 ? x : 0.1f x), then the optional shortcut
            add with its own activation.  It is the yardstick's yardstick: errors are measured against it.
  chain32   the fp32 reference chain: the oracle's three groupconv calls and its shortcut, frame by frame (conv-v0.c:7-31, ffcnn.c:418-423).

Tensors are CNHW as the kernels take them: (channels * N, H, W).  Filters are conv.h rows: K weights padded to a multiple of four, then scale',
bias' and two unused floats.  Inputs are drawn as everywhere else in the suite: make_filter and uniform(-1, 1)."""
import numpy as np

LEAKY = np.float64(np.float32(0.1))


def make_filter(rng, fn, K):
    k4 = (K + 3) & ~3
    f = np.zeros((fn, k4 + 4), np.float32)
    f[:, :K] = rng.uniform(-0.5, 0.5, (fn, K))
    f[:, k4] = rng.uniform(0.5, 1.5, fn)
    f[:, k4 + 1] = rng.uniform(-0.1, 0.1, fn)
    return f


def out_dims(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def make_inputs(seed, N, W, H, ic, ec, oc, stride):
    """x, f1, fd, f2, res: the residual is always drawn (a case without one does not pass it), so that a case and its twin share everything else"""
    rng = np.random.default_rng(seed)
    OH, OW = out_dims(H, W, stride)
    x = rng.uniform(-1, 1, (ic * N, H, W)).astype(np.float32)
    f1, fd, f2 = make_filter(rng, ec, ic), make_filter(rng, ec, 9), make_filter(rng, oc, ec)
    res = rng.uniform(-1, 1, (oc * N, OH, OW)).astype(np.float32)
    return x, f1, fd, f2, res


def act64(v, act):
    with np.errstate(invalid="ignore"):
        if act == 1:
            return np.where(v > 0, v, 0.0)
        if act == 2:
            return np.where(v > 0, v, LEAKY * v)
    assert act == 0, act
    return v


def _affine(s, f, K):
    k4 = (K + 3) & ~3
    sc, bi = f[:, k4].astype(np.float64), f[:, k4 + 1].astype(np.float64)
    return s * sc[:, None, None, None] + bi[:, None, None, None]


def block64(x, f1, fd, f2, res, N, W, H, ic, ec, oc, stride, acts):
    """(oc, N, OH, OW) float64"""
    act1, actd, act2, res_act = acts
    OH, OW = out_dims(H, W, stride)
    with np.errstate(invalid="ignore", over="ignore"):
        x64 = x.reshape(ic, N, H, W).astype(np.float64)
        e = act64(_affine(np.einsum("ei,inhw->enhw", f1[:, :ic].astype(np.float64), x64), f1, ic), act1)
        taps = fd[:, :9].astype(np.float64).reshape(ec, 3, 3)            # [row j, column k]: input (y s - 1 + j, x s - 1 + k)
        d = np.zeros((ec, N, OH, OW))
        for j in range(3):
            for k in range(3):
                # the reference skips taps outside the plane (it does not multiply a padding zero): index only what is inside
                ys = [y for y in range(OH) if 0 <= y * stride - 1 + j < H]
                xs = [c for c in range(OW) if 0 <= c * stride - 1 + k < W]
                if not ys or not xs:
                    continue
                src = e[:, :, ys[0] * stride - 1 + j:ys[-1] * stride + j:stride, xs[0] * stride - 1 + k:xs[-1] * stride + k:stride]
                d[:, :, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] += src * taps[:, j, k][:, None, None, None]
        d = act64(_affine(d, fd, 9), actd)
        y = act64(_affine(np.einsum("oe,enhw->onhw", f2[:, :ec].astype(np.float64), d), f2, ec), act2)
        if res is not None:
            y = act64(y + res.reshape(oc, N, OH, OW).astype(np.float64), res_act)
    return y


def chain32(orc, x, f1, fd, f2, res, N, W, H, ic, ec, oc, stride, acts):
    """(oc, N, OH, OW) float32: orc.groupconv three times and orc.shortcut, one frame at a time"""
    act1, actd, act2, res_act = acts
    OH, OW = out_dims(H, W, stride)
    xf = x.reshape(ic, N, H, W)
    rf = None if res is None else res.reshape(oc, N, OH, OW)
    out = np.empty((oc, N, OH, OW), np.float32)
    for n in range(N):
        o1 = orc.groupconv(np.ascontiguousarray(xf[:, n]), f1, 1, 0, 1, 1, act1)
        o2 = orc.groupconv(o1, fd, ec, 1, stride, 3, actd)
        o3 = orc.groupconv(o2, f2, 1, 0, 1, 1, act2)
        if rf is not None:
            o3 = orc.shortcut(o3, np.ascontiguousarray(rf[:, n]), res_act)
        out[:, n] = o3
    return out


def criterion(E_k, E_ref, ymax, factor=2.0):
    """both parts of tests/test_gpu_round4.py::test_x3_fused_block_is_an_fp32_reorder, with the reference chain's own error as the yardstick"""
    return E_k <= factor * E_ref + 1e-6 and E_k <= 8e-7 * ymax + 1e-6
