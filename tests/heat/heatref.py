"""Heat maps: a numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_heat_boxes_dev, ffgpu_heat_blend_bgr_dev / _nv12_dev, ffgpu_heat_palette),
in the contract's own words.

Accumulate, one frame of one video stream at a time:
    1. the record's list in list order: a box qualifies when score >= min_score (NaN never) and its type is allowed; until DETS boxes are considered,
       the rest is `dropped`;
    2. decay: v - ((v + (1 << k) - 1) >> k) for every cell, read clamped to MAX;
    3. deposit: ANCHOR -- the fp32 anchor converted, outside the extent counted, else gain >> d to the cells at Chebyshev distance d <= spread;
       BOX -- the integer corners clipped to the extent, gain to every cell from (X0 >> k, Y0 >> k) to (X1 >> k, Y1 >> k); cells saturate at MAX;
    4. peak, frames += 1.
Blend, one target at a time: the cells' levels min(255, cell 255 / F), the pixel's level (NEAREST, or SMOOTH: bilinear between cell centres in integers),
the alpha, new = (old (255 - a) + pal[level][ch] a + 127) / 255; NV12 chroma sample (i, j) follows luma pixel (2 i, 2 j).

GPU results are compared with THIS, byte for byte.  tests/test_heat_abi.py pins it to a naive second implementation: Python loops per pixel and per box
over a dict of cells.  `trace`, where given, is a dict in which the functions count what they met (tests/heat/fuzzcases.py holds the fuzz's seeds to it)."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])
MAX = 2 ** 31 - 1
DETS, ROW, STATE_HEADER = 128, 8, 16
ANCHOR, BOX = 0, 1
NEAREST, SMOOTH = 0, 1
RAMP_ALPHA = 1
HEADER = ("considered", "dropped", "outside", "frame", "peak", "saturated")
F32 = np.float32
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1
PALETTE_ANCHORS = ((0, (255, 0, 0)), (64, (255, 255, 0)), (128, (0, 255, 0)), (192, (0, 255, 255)), (255, (0, 0, 255)))


class Spec:
    def __init__(self, gw, gh, cell_log2, mode=ANCHOR, anchor=0, spread=0, gain=1, decay_shift=0, min_score=0.0, classes=None):
        self.gw, self.gh, self.cell_log2, self.mode, self.anchor, self.spread, self.gain, self.decay_shift = gw, gh, cell_log2, mode, anchor, spread, gain, decay_shift
        self.min_score, self.classes = F32(min_score), None if classes is None else [bool(v) for v in classes]

    def allowed(self, type_):
        return self.classes is None or (0 <= int(type_) < len(self.classes) and self.classes[int(type_)])


class BlendSpec:
    def __init__(self, gw, gh, cell_log2, full_scale=0, floor=0, opacity=128, smooth=False, ramp_alpha=False, palette=None):
        self.gw, self.gh, self.cell_log2, self.full_scale, self.floor, self.opacity = gw, gh, cell_log2, full_scale, floor, opacity
        self.smooth, self.ramp_alpha, self.palette = bool(smooth), bool(ramp_alpha), None if palette is None else np.asarray(palette, np.uint8).reshape(256, -1)[:, :3].copy()

    def pal(self, nv12):
        return (palette(nv12)[:, :3] if self.palette is None else self.palette).astype(np.int64)


def stream_nbytes(gw, gh):
    return (STATE_HEADER + 4 * gw * gh + 15) & ~15


def state_nbytes(nstreams, gw, gh):
    return nstreams * stream_nbytes(gw, gh)


class State:
    """nstreams blocks of a header { frames, peak, reserved x 2 }, gh x gw cells and the bytes that round the block up to 16 (never written); all zero: empty"""

    def __init__(self, nstreams, gw, gh, raw=None):
        self.nstreams, self.gw, self.gh = nstreams, gw, gh
        self.raw = np.zeros((nstreams, stream_nbytes(gw, gh)), np.uint8)
        if raw is not None:
            self.raw[:] = np.ascontiguousarray(raw, np.uint8).reshape(self.raw.shape)
        self.hdr = self.raw[:, :STATE_HEADER].view("<u4")
        self.cells = self.raw[:, STATE_HEADER:STATE_HEADER + 4 * gw * gh].view("<u4").reshape(nstreams, gh, gw)

    def tobytes(self):
        return self.raw.tobytes()

    def copy(self):
        return State(self.nstreams, self.gw, self.gh, self.raw)


def f2i(v):
    """the draw contract's conversion of one fp32: toward zero, saturating, NaN -> 0"""
    v = F32(v)
    if np.isnan(v):
        return 0
    if v >= F32(2147483648.0):
        return IMAX
    if v <= F32(-2147483648.0):
        return IMIN
    return int(v)


def anchors(boxes, anchor):
    """the converted anchors of the boxes (step 2 of the trails contract): two int lists"""
    x1, y1, x2, y2 = (np.asarray(boxes[c], F32) for c in ("x1", "y1", "x2", "y2"))
    with np.errstate(all="ignore"):
        px = (x1 + x2) * F32(0.5)
        py = y2.copy() if anchor != 0 else (y1 + y2) * F32(0.5)
    assert px.dtype == np.float32 and py.dtype == np.float32
    return [f2i(v) for v in px], [f2i(v) for v in py]


def count(trace, key, n=1):
    if trace is not None and n:
        trace[key] = trace.get(key, 0) + int(n)


def frame(boxes, spec, hdr, cells, trace=None):
    """one frame of one stream: boxes is the record's list (clamped), hdr the stream's 4 words and cells its gh x gw grid, both updated in place;
    returns the row"""
    k, gw, gh, c = spec.cell_log2, spec.gw, spec.gh, 1 << spec.cell_log2
    ew, eh = gw * c, gh * c
    with np.errstate(invalid="ignore"):
        ok = [i for i in range(len(boxes)) if boxes[i]["score"] >= spec.min_score and spec.allowed(boxes[i]["type"])]
    dropped, ok = max(0, len(ok) - DETS), ok[:DETS]
    cons = boxes[ok]
    v = np.minimum(cells.astype(np.int64), MAX)
    before = v.copy()
    if spec.decay_shift:
        v = v - ((v + (1 << spec.decay_shift) - 1) >> spec.decay_shift)
        count(trace, "decay_to_zero", ((before > 0) & (v == 0)).sum())
    add = np.zeros((gh, gw), np.int64)
    outside = 0
    if spec.mode == ANCHOR:
        ax, ay = anchors(cons, spec.anchor)
        s = spec.spread
        for x, y in zip(ax, ay):
            if x < 0 or x > ew - 1 or y < 0 or y > eh - 1:
                outside += 1
                count(trace, "anchor_negative", x < 0 or y < 0)
                count(trace, "anchor_beyond", x > ew - 1 or y > eh - 1)
                continue
            i, j = x >> k, y >> k
            count(trace, "anchor_border_lo", x % c == c - 1 and i + 1 < gw)
            count(trace, "anchor_border_hi", x % c == 0 and i > 0)
            count(trace, "spread_over_edge", i - s < 0 or j - s < 0 or i + s > gw - 1 or j + s > gh - 1)
            for jj in range(max(j - s, 0), min(j + s, gh - 1) + 1):
                for ii in range(max(i - s, 0), min(i + s, gw - 1) + 1):
                    add[jj, ii] += spec.gain >> max(abs(ii - i), abs(jj - j))
    else:
        for b in cons:
            a_, b_, c_, d_ = f2i(b["x1"]), f2i(b["y1"]), f2i(b["x2"]), f2i(b["y2"])
            X0, Y0, X1, Y1 = max(a_, 0), max(b_, 0), min(c_, ew - 1), min(d_, eh - 1)
            if a_ > c_ or b_ > d_ or X0 > X1 or Y0 > Y1:
                outside += 1
                count(trace, "box_outside", a_ <= c_ and b_ <= d_)
                continue
            count(trace, "box_clipped", (X0, Y0, X1, Y1) != (a_, b_, c_, d_))
            count(trace, "box_several_cells", (X1 >> k) > (X0 >> k) and (Y1 >> k) > (Y0 >> k))
            add[Y0 >> k:(Y1 >> k) + 1, X0 >> k:(X1 >> k) + 1] += spec.gain
    v = np.minimum(v + add, MAX)
    count(trace, "reached_max", ((v == MAX) & (before < MAX)).sum())
    cells[:] = v.astype(np.uint32)
    peak, fr = int(v.max()), int(hdr[0])
    row = [len(ok), min(dropped, IMAX), outside, (fr + 2 ** 31) % 2 ** 32 - 2 ** 31, peak, int((v == MAX).sum()), 0, 0]
    hdr[0], hdr[1] = (fr + 1) % 2 ** 32, peak
    return row


def accumulate(recs, flat, stride, first, streams, spec, state, trace=None):
    """ffgpu_heat_boxes_dev: record t is the next frame of stream streams[t] (-1: ignored, a zero row); flat None: the records' own boxes (stride
    MAX_DET).  state is updated in place; returns the rows, (n, ROW) int32"""
    n = len(streams)
    rows = np.zeros((n, ROW), "<i4")
    for t in range(n):
        s = streams[t]
        if s < 0:
            continue
        if flat is None:
            nb = max(0, min(int(recs[t]["count"]), MAX_DET))
            boxes = recs[t]["box"][:nb]
        else:
            nb = max(0, min(int(recs[t]["nfull"]), stride))
            f0 = t * stride if first is None else first[t]
            boxes = flat[f0:f0 + nb]
        count(trace, "top_bit", (state.cells[s] >> 31).any())
        rows[t] = frame(boxes, spec, state.hdr[s], state.cells[s], trace)
    return rows


def palette(nv12):
    """ffgpu_heat_palette: (256, 4) uint8, B G R 0 or Y U V 0"""
    out = np.zeros((256, 4), np.uint8)
    for (v0, c0), (v1, c1) in zip(PALETTE_ANCHORS[:-1], PALETTE_ANCHORS[1:]):
        for v in range(v0, v1 + 1):
            ch = [(c0[i] * (v1 - v) + c1[i] * (v - v0) + (v1 - v0) // 2) // (v1 - v0) for i in range(3)]
            if nv12:
                B, G, R = ch
                ch = [(29 * B + 150 * G + 77 * R + 128) >> 8, ((128 * B - 85 * G - 43 * R + 128) >> 8) + 128, ((-21 * B - 107 * G + 128 * R + 128) >> 8) + 128]
                ch = [max(0, min(255, x)) for x in ch]
            out[v, :3] = ch
    return out


def levels(hdr, cells, bs, trace=None):
    """the cells' levels (gh x gw int64), or None when nothing is drawn (automatic full_scale, peak 0)"""
    F = bs.full_scale if bs.full_scale >= 1 else min(int(hdr[1]), MAX)
    if F == 0:
        count(trace, "auto_peak_zero")
        return None
    q = np.minimum(cells.astype(np.int64), MAX) * 255 // F
    count(trace, "level_clamped", (q > 255).sum())
    return np.minimum(q, 255)


def pixel_levels(L, bs, W, H, trace=None):
    """the levels of pixels (0 .. W - 1) x (0 .. H - 1), inside the extent: (H, W) int64"""
    k, c = bs.cell_log2, 1 << bs.cell_log2
    x, y = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
    if not bs.smooth:
        return L[(y >> k)[:, None], (x >> k)[None, :]]
    h = c // 2
    i0, j0, fx, fy = (x - h) >> k, (y - h) >> k, ((x - h) & (c - 1))[None, :], ((y - h) & (c - 1))[:, None]
    count(trace, "smooth_i0_negative", (i0 < 0).sum())
    count(trace, "smooth_i1_clamped", (i0 + 1 > bs.gw - 1).sum())
    ia, ib, ja, jb = np.clip(i0, 0, bs.gw - 1)[None, :], np.clip(i0 + 1, 0, bs.gw - 1)[None, :], np.clip(j0, 0, bs.gh - 1)[:, None], np.clip(j0 + 1, 0, bs.gh - 1)[:, None]
    return (L[ja, ia] * (c - fx) * (c - fy) + L[ja, ib] * fx * (c - fy) + L[jb, ia] * (c - fx) * fy + L[jb, ib] * fx * fy + c * c // 2) >> (2 * k)


def alphas(lev, bs, trace=None):
    """the alpha of every pixel level; 0: not written"""
    a = (lev * bs.opacity + 127) // 255 if bs.ramp_alpha else np.full(lev.shape, bs.opacity, np.int64)
    drawn = lev >= max(bs.floor, 1)
    count(trace, "ramp_alpha_zero", (drawn & (a == 0)).sum())
    return np.where(drawn, a, 0)


def covered(w, h, bs, trace=None):
    W, H = min(w, bs.gw << bs.cell_log2), min(h, bs.gh << bs.cell_log2)
    count(trace, "right_of_extent", W < w)
    count(trace, "below_extent", H < h)
    return W, H


def block_trace(lev, bs, trace):
    """a 64 x 64 block wholly below the floor next to one that is not"""
    if trace is None:
        return
    H, W = lev.shape
    on = np.array([[bool((lev[y:y + 64, x:x + 64] >= max(bs.floor, 1)).any()) for x in range(0, W, 64)] for y in range(0, H, 64)])
    count(trace, "block_below_next_to_drawn", (on[:, 1:] != on[:, :-1]).sum() + (on[1:] != on[:-1]).sum())


def mix(old, colour, a):
    return (old.astype(np.int64) * (255 - a) + colour * a + 127) // 255


def blend_bgr(buf, off, w, h, pitch, hdr, cells, bs, trace=None):
    """ffgpu_heat_blend_bgr_dev on one target whose pixel (0, 0) lies at buf[off]; buf (flat uint8) is updated in place"""
    L = levels(hdr, cells, bs, trace)
    W, H = covered(w, h, bs, trace)
    if L is None:
        return
    lev = pixel_levels(L, bs, W, H, trace)
    a = alphas(lev, bs, trace)
    block_trace(lev, bs, trace)
    px = np.lib.stride_tricks.as_strided(buf[off:], (H, W, 3), (pitch, 3, 1))
    new = mix(px, bs.pal(False)[lev], a[:, :, None])
    px[:] = np.where(a[:, :, None] > 0, new, px).astype(np.uint8)


def blend_nv12(buf, off_y, off_uv, w, h, pitch_y, pitch_uv, hdr, cells, bs, trace=None):
    """ffgpu_heat_blend_nv12_dev on one target: luma per pixel, chroma sample (i, j) with the level and alpha of luma pixel (2 i, 2 j)"""
    L = levels(hdr, cells, bs, trace)
    W, H = covered(w, h, bs, trace)
    if L is None:
        return
    lev = pixel_levels(L, bs, W, H, trace)
    a = alphas(lev, bs, trace)
    block_trace(lev, bs, trace)
    pal = bs.pal(True)
    py = np.lib.stride_tricks.as_strided(buf[off_y:], (H, W), (pitch_y, 1))
    py[:] = np.where(a > 0, mix(py, pal[lev][:, :, 0], a), py).astype(np.uint8)
    lc, ac = lev[::2, ::2], a[::2, ::2]
    puv = np.lib.stride_tricks.as_strided(buf[off_uv:], ((H + 1) // 2, (W + 1) // 2, 2), (pitch_uv, 2, 1))
    puv[:] = np.where(ac[:, :, None] > 0, mix(puv, pal[lc][:, :, 1:3], ac[:, :, None]), puv).astype(np.uint8)
