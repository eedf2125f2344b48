"""Motion maps: a numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_motion_update_bgr_dev / _nv12_dev, ffgpu_motion_gate_dev,
ffgpu_motion_state_bytes), in the contract's own words.

State, per stream: a header { frames, reserved x 3 }, the background plane (h rows of ALIGN(w, 8) shorts, luma in 8.8 fixed point) and gw x gh cells
rounded up to 16 bytes.
Update, one frame of one stream: luma (NV12: the Y byte; BGR: (29 B + 150 G + 77 R + 128) >> 8); cur = y << 8, d = cur - bg; with frames == 0 nothing
is changed and bg = cur; else changed when |d| > threshold << 8, k = learn_shift_changed or learn_shift, bg += sgn(d) ((|d| + (1 << k) - 1) >> k)
(k == 16: bg stays); every cell = its changed pixels; frames += 1; the row { frame, changed, active, x0, y0, x1, y1, warm, 0 x 8 }.
Gate, one record of one stream: the qualifying boxes in list order up to DETS; the integer corners clipped to w x h; touched and active cells; warm =
frames > warmup; MOVING = not warm, or touched >= 1 and active 256 >= cover touched; the words and the gated record.

GPU results are compared with THIS, byte for byte.  tests/test_motion_abi.py pins it to a naive second implementation: Python loops per pixel and per
box.  `trace`, where given, is a dict in which the functions count what they met (tests/motion/fuzzcases.py holds the fuzz's seeds to it)."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])
DETS, ROW, WORDS, STATE_HEADER, MAX_SIDE = 128, 16, 8, 16, 8192
GATE_INVERT = 1
ROW_HEADER = ("frame", "changed", "active", "x0", "y0", "x1", "y1", "warm")
WORDS_HEADER = ("considered", "dropped", "outside", "moving", "warm", "frames")
F32 = np.float32
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


class Spec:
    def __init__(self, w, h, cell_log2, threshold=16, learn_shift=4, learn_shift_changed=8, min_pixels=1, cover=64, warmup=0, invert=False, min_score=0.0, classes=None):
        self.w, self.h, self.cell_log2, self.threshold, self.learn_shift, self.learn_shift_changed = w, h, cell_log2, threshold, learn_shift, learn_shift_changed
        self.min_pixels, self.cover, self.warmup, self.invert = min_pixels, cover, warmup, bool(invert)
        self.min_score, self.classes = F32(min_score), None if classes is None else [bool(v) for v in classes]

    def allowed(self, type_):
        return self.classes is None or (0 <= int(type_) < len(self.classes) and self.classes[int(type_)])

    @property
    def c(self):
        return 1 << self.cell_log2

    @property
    def gw(self):
        return (self.w + self.c - 1) >> self.cell_log2

    @property
    def gh(self):
        return (self.h + self.c - 1) >> self.cell_log2


def plane_pitch(w):
    return (w + 7) & ~7


def cells_offset(w, h):
    return STATE_HEADER + 2 * plane_pitch(w) * h


def stream_nbytes(w, h, cell_log2):
    c = 1 << cell_log2
    return cells_offset(w, h) + ((4 * ((w + c - 1) // c) * ((h + c - 1) // c) + 15) & ~15)


def state_nbytes(nstreams, w, h, cell_log2):
    if not (1 <= nstreams <= 65536 and 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE and 2 <= cell_log2 <= 6):
        return 0
    return nstreams * stream_nbytes(w, h, cell_log2)


class State:
    """nstreams blocks of a header, the plane and the cells; the padding shorts of the plane's rows and the bytes that round the cells up to 16 are
    never written; all zero: empty"""

    def __init__(self, nstreams, w, h, cell_log2, raw=None):
        self.nstreams, self.w, self.h, self.cell_log2 = nstreams, w, h, cell_log2
        c = 1 << cell_log2
        gw, gh, co = (w + c - 1) // c, (h + c - 1) // c, cells_offset(w, h)
        self.raw = np.zeros((nstreams, stream_nbytes(w, h, cell_log2)), np.uint8)
        if raw is not None:
            self.raw[:] = np.ascontiguousarray(raw, np.uint8).reshape(self.raw.shape)
        self.hdr = self.raw[:, :STATE_HEADER].view("<u4")
        self.plane = self.raw[:, STATE_HEADER:co].view("<u2").reshape(nstreams, h, plane_pitch(w))[:, :, :w]
        self.cells = self.raw[:, co:co + 4 * gw * gh].view("<u4").reshape(nstreams, gh, gw)
        assert np.shares_memory(self.plane, self.raw) and np.shares_memory(self.cells, self.raw)

    def tobytes(self):
        return self.raw.tobytes()

    def copy(self):
        return State(self.nstreams, self.w, self.h, self.cell_log2, self.raw)


def luma_bgr(img):
    """the luma of an h x w x 3 array of B G R bytes"""
    p = np.asarray(img).astype(np.int64)
    return (29 * p[:, :, 0] + 150 * p[:, :, 1] + 77 * p[:, :, 2] + 128) >> 8


def count(trace, key, n=1):
    if trace is not None and n:
        trace[key] = trace.get(key, 0) + int(n)


def s32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def update_frame(luma, spec, hdr, plane, cells, trace=None):
    """one frame of one stream: luma is h x w (0..255), hdr the stream's 4 words, plane its h x w shorts and cells its gh x gw grid, all updated in
    place; returns the row"""
    w, h, k, c = spec.w, spec.h, spec.cell_log2, spec.c
    luma = np.asarray(luma).astype(np.int64)
    assert luma.shape == (h, w) and plane.shape == (h, w) and cells.shape == (spec.gh, spec.gw)
    frames = int(hdr[0])
    cur, bg = luma << 8, plane.astype(np.int64)
    d = cur - bg
    ad = np.abs(d)
    if frames == 0:
        changed = np.zeros((h, w), bool)
        new = cur
    else:
        changed = ad > (spec.threshold << 8)
        ks = np.where(changed, spec.learn_shift_changed, spec.learn_shift)
        step = np.where(ks >= 16, 0, (ad + (1 << np.minimum(ks, 15)) - 1) >> np.minimum(ks, 15))
        new = bg + np.sign(d) * step
        count(trace, "at_threshold", (ad == (spec.threshold << 8)).sum())
        count(trace, "one_above", (ad == (spec.threshold << 8) + 1).sum())
        count(trace, "reached_cur", ((new == cur) & (bg != cur)).sum())
        count(trace, "frozen_changed", (changed & (new == bg)).sum())
        count(trace, "changed", changed.sum())
        count(trace, "unchanged", (~changed).sum())
    assert new.min() >= 0 and new.max() <= 65535
    plane[:] = new.astype(np.uint16)
    cnt = np.zeros((spec.gh * c, spec.gw * c), np.int64)
    cnt[:h, :w] = changed
    cell = cnt.reshape(spec.gh, c, spec.gw, c).sum(axis=(1, 3))
    cells[:] = cell.astype(np.uint32)
    active = cell >= spec.min_pixels
    if frames != 0:
        count(trace, "active_cells", active.sum())
        count(trace, "inactive_cells", (~active).sum())
    hdr[0] = (frames + 1) % 2 ** 32
    row = [0] * ROW
    row[0], row[1], row[2] = s32(frames), int(changed.sum()), int(active.sum())
    if active.any():
        jj, ii = np.nonzero(active)
        row[3], row[4], row[5], row[6] = c * int(ii.min()), c * int(jj.min()), min(c * (int(ii.max()) + 1), w) - 1, min(c * (int(jj.max()) + 1), h) - 1
    else:
        row[3], row[4], row[5], row[6] = 0, 0, -1, -1
    row[7] = int((frames + 1) % 2 ** 32 > spec.warmup)
    return row


def update(lumas, streams, spec, state, trace=None):
    """frame t (an h x w luma array, or None: a NULL pixel address) is the next frame of stream streams[t] (-1: ignored); the state is updated in
    place, in the order given; returns the rows, n x ROW int32"""
    rows = np.zeros((len(streams), ROW), np.int32)
    for t, s in enumerate(streams):
        if s < 0 or lumas[t] is None:
            continue
        rows[t] = update_frame(lumas[t], spec, state.hdr[s], state.plane[s], state.cells[s], trace)
    return rows


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


def gate_record(boxes, spec, hdr, cells, trace=None):
    """one record of one stream: boxes is the record's list (clamped), hdr and cells the stream's, only read; returns the 8 header words, the list of
    (list index, touched, active) of the considered boxes and the list indices of the selected ones"""
    k, w, h = spec.cell_log2, spec.w, spec.h
    with np.errstate(invalid="ignore"):
        ok = [i for i in range(len(boxes)) if boxes[i]["score"] >= spec.min_score and spec.allowed(boxes[i]["type"])]
    dropped, ok = max(0, len(ok) - DETS), ok[:DETS]
    frames = int(hdr[0])
    warm = frames > spec.warmup
    active_map = cells.astype(np.int64) >= spec.min_pixels
    per, sel, outside, nmoving = [], [], 0, 0
    for i in ok:
        b = boxes[i]
        a_, b_, c_, d_ = f2i(b["x1"]), f2i(b["y1"]), f2i(b["x2"]), f2i(b["y2"])
        X0, Y0, X1, Y1 = max(a_, 0), max(b_, 0), min(c_, w - 1), min(d_, h - 1)
        if a_ > c_ or b_ > d_ or X0 > X1 or Y0 > Y1:
            outside += 1
            touched = act = 0
            count(trace, "inverted", a_ > c_ or b_ > d_)
            count(trace, "beyond", a_ <= c_ and b_ <= d_)
        else:
            sub = active_map[Y0 >> k:(Y1 >> k) + 1, X0 >> k:(X1 >> k) + 1]
            touched, act = int(sub.size), int(sub.sum())
            count(trace, "ends_on_boundary", (X1 + 1) % spec.c == 0 and X1 + 1 < w)
            count(trace, "one_past_boundary", X1 % spec.c == 0 and X1 > 0)
            count(trace, "clipped", (X0, Y0, X1, Y1) != (a_, b_, c_, d_))
        moving = (not warm) or (touched >= 1 and act * 256 >= spec.cover * touched)
        nmoving += moving
        count(trace, "moving" if moving else "still")
        if warm and touched:
            count(trace, "cover_exact", act * 256 == spec.cover * touched)
        per.append((i, touched, act))
        if moving != spec.invert:
            sel.append(i)
    return [len(ok), min(dropped, IMAX), outside, nmoving, int(warm), s32(frames), 0, 0], per, sel


def gate(recs, flat, stride, first, streams, spec, state, want_records=True, want_lists=True, trace=None):
    """record t belongs to stream streams[t] (-1: ignored); flat None: the records' own boxes (stride MAX_DET); first: the lists' starts (None: t x
    stride); the state is only read.  Returns the words (n x (WORDS + 2 stride) int32), the gated records (DETS_DTYPE, or None) and the gated lists
    (n x stride boxes, or None)."""
    n = len(streams)
    words = np.zeros((n, WORDS + 2 * stride), np.int32)
    out_recs = np.zeros(n, DETS_DTYPE) if want_records else None
    out_lists = np.zeros((n, stride), BOX_DTYPE) if want_lists else None
    for t, s in enumerate(streams):
        if s < 0:
            continue
        r = recs[t]
        if flat is None:
            boxes = r["box"][:max(0, min(int(r["count"]), stride))]
        else:
            f0 = first[t] if first is not None else t * stride
            boxes = flat[f0:f0 + max(0, min(int(r["nfull"]), stride))]
        head, per, sel = gate_record(boxes, spec, state.hdr[s], state.cells[s], trace)
        words[t, :WORDS] = head
        for i, touched, act in per:
            words[t, WORDS + 2 * i], words[t, WORDS + 2 * i + 1] = touched, act
        nt = len(sel)
        count(trace, "selected", nt)
        count(trace, "rejected", head[0] - nt)
        if out_recs is not None:
            o = out_recs[t]
            o["count"], o["ncand"], o["overflow"], o["nfull"] = min(nt, MAX_DET), r["ncand"], (int(r["overflow"]) & 1) | (4 if nt > MAX_DET else 0), nt
            o["box"][:min(nt, MAX_DET)] = boxes[sel[:MAX_DET]]
        if out_lists is not None:
            out_lists[t, :nt] = boxes[sel]
    return words, out_recs, out_lists
