"""The net's first four layers -- dense 3x3 stride-2 convolution 3 -> 8, then 1x1 8 -> 8, depthwise 3x3, 1x1 8 -> 4, what k_front (ffgpu_front.inc) runs
as one launch -- restated for tests/front:

  front64   float64 throughout on the fp32 operands: convref.conv64 for layer 0 (its padding taps contribute nothing, as im2row's zeros times finite weights do),
            then blockref.block64 without a residual.  Errors are measured against it.
  front32   the fp32 reference: the oracle's four groupconv calls, frame by frame.
  bound     the hard bound per output, below.
  u8_input  net_input for frames of the net's own size: plane 0 / 1 / 2 = ((float)R - mean[0]) * norm[0], (G ...), (B ...) with two fp32 roundings.

Frames are (N, 3, 2 H, 2 W) as forward_host takes them; outputs are (4, N, H, W) as read_layer(3, n) stacks; W x H is the 8-channel plane.
Filters are conv.h rows (blockref.make_filter): f0 (8, 32) with 27 taps, scale' at 28, bias' at 29; f1 (8, 12), fd (8, 16), f2 (4, 12).

THE BOUND.  convref's bound for one layer is gamma(K + 3) (|scale'| sum |w x| + |bias'|) with K roundings for the sum in any order, one or two for the affine step
and one for the leaky product.  A later layer reads a tensor that is itself off by at most b (its producer's bound; rounding it to fp32 is the affine rounding that
b already counts).  With S(m) = |scale'| sum |w| m over the layer's taps, m = |x| + b the largest value an input can have, the layer's own roundings act on inputs of
size m, and the inherited error passes through the sum with the weights' absolute values:
    b_next = gamma(K + 3) (S(|x| + b) + |bias'|) + S(b)
exactly as convref.pair64 carries a depthwise layer's bound through the pointwise layer behind it.  Relu, leaky and the identity are 1-Lipschitz, so b_next holds
behind the activation.  Four stages, K = 27, 8, 9, 8, b = 0 for the net input (the fp32 frames are the operands).  Where relu makes an exact 0 of a NaN or a -Inf
(utils.h:18) the value carries no error: b = 0 there, although the formula's terms are not finite.  Derived, not measured: no correct fp32 evaluation of the four
layers can exceed it, in whatever order a kernel sums."""
import numpy as np

from conv_kernels import convref
from irb_blocks import blockref

KS = (27, 8, 9, 8)


def cnhw(frames):
    """(N, 3, 2H, 2W) frames as the CNHW tensor conv64 takes: (3 N, 2H, 2W)"""
    N, C, IH, IW = frames.shape
    return np.ascontiguousarray(frames.transpose(1, 0, 2, 3)).reshape(C * N, IH, IW)


def front64(frames, f0, f1, fd, f2, acts):
    N, _, IH, IW = frames.shape
    W, H = IW // 2, IH // 2
    y0, _ = convref.conv64(cnhw(frames), f0, N, IW, IH, 3, 1, 1, 2, 3, acts[0])
    return blockref.block64(y0.reshape(8 * N, H, W), f1, fd, f2, None, N, W, H, 8, 8, 4, 1, (acts[1], acts[2], acts[3], 0))


def front32(orc, frames, f0, f1, fd, f2, acts):
    N, _, IH, IW = frames.shape
    out = np.empty((4, N, IH // 2, IW // 2), np.float32)
    for n in range(N):
        o = orc.groupconv(np.ascontiguousarray(frames[n]), f0, 1, 1, 2, 3, acts[0])
        o = orc.groupconv(o, f1, 1, 0, 1, 1, acts[1])
        o = orc.groupconv(o, fd, 8, 1, 1, 3, acts[2])
        out[:, n] = orc.groupconv(o, f2, 1, 0, 1, 1, acts[3])
    return out


def _abs_rows(f, K):
    """the filter with |w|, scale' = |scale'|, bias' = 0: conv64 of it is S(.)"""
    k4 = (K + 3) & ~3
    g = np.zeros(f.shape, np.float64)
    g[:, :K] = np.abs(f[:, :K].astype(np.float64))
    g[:, k4] = np.abs(f[:, k4].astype(np.float64))
    return g


def bound(frames, f0, f1, fd, f2, acts):
    """(4, N, H, W) float64: the module docstring's bound, carried through the four stages"""
    N, _, IH, IW = frames.shape
    W, H = IW // 2, IH // 2
    # (input tensor geometry, channels, groups, padding, stride, filter size) per stage
    geo = ((IW, IH, 3, 1, 1, 2, 3), (W, H, 8, 1, 0, 1, 1), (W, H, 8, 8, 1, 1, 3), (W, H, 8, 1, 0, 1, 1))
    x = cnhw(frames).astype(np.float64)
    b = np.zeros(x.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for f, K, act, (w, h, ic, groups, pad, stride, fs) in zip((f0, f1, fd, f2), KS, acts, geo):
            k4 = (K + 3) & ~3
            y, _ = convref.conv64(x, f, N, w, h, ic, groups, pad, stride, fs, act)
            fa = _abs_rows(f, K)
            s_m, _ = convref.conv64(np.abs(x) + b, fa, N, w, h, ic, groups, pad, stride, fs, 0)
            s_b, _ = convref.conv64(b, fa, N, w, h, ic, groups, pad, stride, fs, 0)
            bn = convref.gamma(K + 3) * (s_m + np.abs(f[:, k4 + 1].astype(np.float64))[:, None, None, None]) + s_b
            bn = np.where(np.isfinite(y) & ~np.isfinite(bn), 0.0, bn)            # relu(NaN) = relu(-Inf) = 0 is exact
            x, b = y.reshape(-1, y.shape[2], y.shape[3]), bn.reshape(-1, y.shape[2], y.shape[3])
    return b.reshape(4, N, H, W)


def u8_input(u8, mean, norm):
    """u8: (N, 2H, 2W, 3) B G R bytes -> (N, 3, 2H, 2W) float32, planes R G B (ffcnn.c:259-289 without the resize)"""
    out = np.empty((u8.shape[0], 3) + u8.shape[1:3], np.float32)
    for ci in range(3):
        out[:, ci] = (u8[..., 2 - ci].astype(np.float32) - np.float32(mean[ci])) * np.float32(norm[ci])
    return out
