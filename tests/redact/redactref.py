"""numpy restatement of the redaction contract of include/ffcnn_hip.h (ffgpu_redact_boxes_*_dev, ffgpu_exec_redact_*): which pixels of a target are
covered (the crop contract's qualifying rule and region, tests/crops/cropref.py, on the draw contract's corners, tests/overlay/drawref.py), and what
FILL and MOSAIC leave in a uint8 buffer with pitch, for BGR and NV12 targets.  The covered set and the cells' means are computed as whole arrays;
tests/test_redact_abi.py holds them against loops that take one pixel at a time.  The operator has no counterpart in the reference project: nothing
here is pinned to it.  Nothing here knows how the device parallelises."""
import numpy as np

from crops import cropref
from overlay import drawref

BOX_DTYPE = drawref.BOX_DTYPE
FILL, MOSAIC = 0, 1


class Spec:
    """ffgpu_redact_spec: classes is None or a sequence of flags; margin = (num, den); color = B G R or Y U V"""

    def __init__(self, mode, cell=0, outside=False, min_score=0.0, classes=None, margin=(0, 1), color=(0, 0, 0)):
        self.mode, self.cell, self.outside, self.min_score, self.classes = mode, cell, bool(outside), min_score, classes
        self.num, self.den = margin
        self.color = tuple(int(c) for c in color[:3])


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int(n)


def regions(w, h, boxes, spec, stats=None):
    """the clipped regions (X0, Y0, X1, Y1) of the qualifying boxes of a w x h target.  stats counts the boxes: qualifying, empty (qualifying, no
    region), rejected_score, rejected_class"""
    out = []
    for box in boxes:
        assert drawref.corners(box) == cropref.corners(box)
        if not cropref.qualifies(box, spec):
            by_score = not (np.float32(box["score"]) >= np.float32(spec.min_score))
            _bump(stats, "rejected_score" if by_score else "rejected_class")
            continue
        _bump(stats, "qualifying")
        r = cropref.region(box, w, h, spec.num, spec.den)
        if r is None:
            _bump(stats, "empty")
            continue
        out.append(r[:4])
    return out


def covered(w, h, boxes, spec, stats=None):
    """S as an (h, w) bool array"""
    u = np.zeros((h, w), bool)
    for X0, Y0, X1, Y1 in regions(w, h, boxes, spec, stats):
        u[Y0:Y1 + 1, X0:X1 + 1] = True
    s = ~u if spec.outside else u
    _bump(stats, "pixels", w * h)
    _bump(stats, "covered", np.count_nonzero(s))
    return s


def _cells(a, s, fill):
    """an (h, w) array as (cells down, s, cells across, s), the cells of the last row and column padded with `fill`"""
    h, w = a.shape
    p = np.full((-(-h // s) * s, -(-w // s) * s), fill, a.dtype)
    p[:h, :w] = a
    return p.reshape(p.shape[0] // s, s, p.shape[1] // s, s)


def cell_means(plane, s):
    """every pixel's cell mean m = (sum + n / 2) / n over the clipped cell, cells of side s anchored at (0, 0); (h, w) uint8"""
    h, w = plane.shape
    sums = _cells(plane.astype(np.int64), s, 0).sum((1, 3))
    n = _cells(np.ones((h, w), np.int64), s, 0).sum((1, 3))
    m = (sums + n // 2) // n
    return np.repeat(np.repeat(m, s, 0), s, 1)[:h, :w].astype(np.uint8)


def _cell_stats(S, s, stats):
    if stats is None:
        return
    h, w = S.shape
    some, full = _cells(S, s, False).any((1, 3)), _cells(S, s, True).all((1, 3))
    _bump(stats, "cells_full", np.count_nonzero(full))
    _bump(stats, "cells_partial", np.count_nonzero(some & ~full))
    if w % s:
        _bump(stats, "cells_cut_right", np.count_nonzero(some[:, -1]))
    if h % s:
        _bump(stats, "cells_cut_bottom", np.count_nonzero(some[-1, :]))


def chroma_covered(S, stats=None):
    """the FILL rule's view of a sample: ((h + 1) / 2, (w + 1) / 2) bool, a sample is covered when any of its luma pixels inside w x h is"""
    q = _cells(S, 2, False)
    c = q.any((1, 3))
    _bump(stats, "chroma_mixed", np.count_nonzero(c & ~_cells(S, 2, True).all((1, 3))))
    return c


def redact_bgr(buf, base, w, h, pitch, boxes, spec, stats=None):
    """redacts in the flat uint8 array `buf`, whose byte `base` is row 0 of a w x h BGR target with `pitch` bytes between rows.  stats (a dict)
    accumulates the boxes' counts (regions), pixels / covered, and for MOSAIC the cells with a covered pixel: full, partial, cut by the right /
    bottom edge of the frame"""
    px = drawref._view(buf, base, (h, w, 3), (pitch, 3, 1))
    S = covered(w, h, boxes, spec, stats)
    if spec.mode == FILL:
        px[S] = spec.color
    else:
        _cell_stats(S, spec.cell, stats)
        m = np.stack([cell_means(px[:, :, c], spec.cell) for c in range(3)], -1)
        px[S] = m[S]
    return buf


def redact_nv12(buf, base_y, base_uv, w, h, pitch_y, pitch_uv, boxes, spec, stats=None):
    """the NV12 form: byte base_y of `buf` is row 0 of the Y plane, byte base_uv row 0 of the interleaved U V plane; color is (Y, U, V); also
    counts chroma_mixed: covered samples with a luma pixel (inside w x h) that is not in S"""
    Y = drawref._view(buf, base_y, (h, w), (pitch_y, 1))
    UV = drawref._view(buf, base_uv, ((h + 1) // 2, (w + 1) // 2, 2), (pitch_uv, 2, 1))
    S = covered(w, h, boxes, spec, stats)
    C = chroma_covered(S, stats)
    if spec.mode == FILL:
        Y[S] = spec.color[0]
        UV[C] = spec.color[1:]
    else:
        assert spec.cell % 2 == 0
        _cell_stats(S, spec.cell, stats)
        my = cell_means(Y, spec.cell)
        muv = np.stack([cell_means(UV[:, :, c], spec.cell // 2) for c in range(2)], -1)
        Y[S] = my[S]
        UV[C] = muv[C]
    return buf
