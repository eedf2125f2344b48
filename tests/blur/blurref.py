"""numpy restatement of the blur contract of include/ffcnn_hip.h (ffgpu_blur_boxes_*_dev, ffgpu_exec_blur_*): the covered set S is the redact
contract's (tests/redact/redactref.py: `covered`, `chroma_covered`), a pass replaces every byte of S by the rounded integer mean of its clipped
(2 r + 1)-square window over the plane as the pass found it, and the scratch surface ends up holding the final values at the positions of S.  The
window sums come from an integral image of the whole plane; tests/test_blur_abi.py holds them against loops that visit every pixel of every
window.  The operator has no counterpart in the reference project: nothing here is pinned to it.  Nothing here knows how the device parallelises
beyond the 64-pixel blocks that the statistics name."""
import numpy as np

from overlay import drawref
from redact import redactref

BOX_DTYPE = redactref.BOX_DTYPE
BLOCK = 64


class Spec:
    """ffgpu_blur_spec: classes is None or a sequence of flags; margin = (num, den)"""

    def __init__(self, radius, passes=1, outside=False, min_score=0.0, classes=None, margin=(0, 1)):
        self.radius, self.passes, self.outside, self.min_score, self.classes = int(radius), int(passes), bool(outside), min_score, classes
        self.num, self.den = margin


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(n)


def extents(n, r):
    """the clipped window [lo, hi] of every position 0 .. n - 1"""
    i = np.arange(n)
    return np.maximum(i - r, 0), np.minimum(i + r, n - 1)


def box_mean(plane, r):
    """every pixel's (sum over its clipped window + n / 2) / n; plane (h, w) of any integer type, result uint8"""
    h, w = plane.shape
    I = np.zeros((h + 1, w + 1), np.int64)
    I[1:, 1:] = plane.astype(np.int64).cumsum(0).cumsum(1)
    (x0, x1), (y0, y1) = extents(w, r), extents(h, r)
    s = I[(y1 + 1)[:, None], (x1 + 1)[None, :]] - I[y0[:, None], (x1 + 1)[None, :]] - I[(y1 + 1)[:, None], x0[None, :]] + I[y0[:, None], x0[None, :]]
    n = (y1 - y0 + 1)[:, None] * (x1 - x0 + 1)[None, :]
    return ((s + n // 2) // n).astype(np.uint8)


def _window_stats(S, r, stats):
    """what the windows of the covered pixels do: clipped by the frame's edge, reaching into a neighbouring 64-pixel block, spanning three blocks or
    more (a window is at most 63 pixels wide, so it touches at most two blocks along an axis: three or more means across a corner, four), larger
    than the whole target"""
    if stats is None:
        return
    h, w = S.shape
    (x0, x1), (y0, y1) = extents(w, r), extents(h, r)
    clip = ((y1 - y0 < 2 * r)[:, None]) | ((x1 - x0 < 2 * r)[None, :])
    nblocks = (y1 // BLOCK - y0 // BLOCK + 1)[:, None] * (x1 // BLOCK - x0 // BLOCK + 1)[None, :]
    _bump(stats, "win_clipped", np.count_nonzero(S & clip))
    _bump(stats, "win_neighbour", np.count_nonzero(S & (nblocks >= 2)))
    _bump(stats, "win_three_blocks", np.count_nonzero(S & (nblocks >= 3)))
    _bump(stats, "win_whole", np.count_nonzero(S) if 2 * r + 1 > w and 2 * r + 1 > h else 0)


def blur_bgr(buf, base, sbase, w, h, pitch, spitch, boxes, spec, stats=None):
    """blurs in the flat uint8 array `buf`, whose byte `base` is row 0 of a w x h BGR target with `pitch` bytes between rows and whose byte `sbase`
    is row 0 of its scratch surface (pitch `spitch`).  stats (a dict) accumulates redactref's counts (boxes, pixels / covered), the windows'
    (win_*) and `changed`: covered bytes of the target that differ from what they were"""
    px = drawref._view(buf, base, (h, w, 3), (pitch, 3, 1))
    sc = drawref._view(buf, sbase, (h, w, 3), (spitch, 3, 1))
    S = redactref.covered(w, h, boxes, spec, stats)
    _window_stats(S, spec.radius, stats)
    before = px.copy()
    for _ in range(spec.passes):
        m = np.stack([box_mean(px[:, :, c], spec.radius) for c in range(3)], -1)
        px[S] = m[S]
        sc[S] = m[S]
    _bump(stats, "changed", np.count_nonzero(px != before))
    return buf


def blur_nv12(buf, base_y, base_uv, sbase_y, sbase_uv, w, h, pitch_y, pitch_uv, spitch_y, spitch_uv, boxes, spec, stats=None):
    """the NV12 form: luma with radius r, the ((h + 1) / 2, (w + 1) / 2) chroma plane with (r + 1) / 2, U and V apart, written to the samples of the
    redact FILL rule (redactref.chroma_covered)"""
    cw, ch, rc = (w + 1) // 2, (h + 1) // 2, (spec.radius + 1) // 2
    Y, UV = drawref._view(buf, base_y, (h, w), (pitch_y, 1)), drawref._view(buf, base_uv, (ch, cw, 2), (pitch_uv, 2, 1))
    sY, sUV = drawref._view(buf, sbase_y, (h, w), (spitch_y, 1)), drawref._view(buf, sbase_uv, (ch, cw, 2), (spitch_uv, 2, 1))
    S = redactref.covered(w, h, boxes, spec, stats)
    Cs = redactref.chroma_covered(S, stats)
    _window_stats(S, spec.radius, stats)
    before = (Y.copy(), UV.copy())
    for _ in range(spec.passes):
        my = box_mean(Y, spec.radius)
        muv = np.stack([box_mean(UV[:, :, c], rc) for c in range(2)], -1)
        Y[S] = my[S]
        sY[S] = my[S]
        UV[Cs] = muv[Cs]
        sUV[Cs] = muv[Cs]
    _bump(stats, "changed", np.count_nonzero(Y != before[0]) + np.count_nonzero(UV != before[1]))
    return buf
