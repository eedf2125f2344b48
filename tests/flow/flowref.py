"""Flow maps: a numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_flow_update_bgr_dev / _nv12_dev, ffgpu_flow_boxes_dev,
ffgpu_flow_state_bytes), in the contract's own words.  GPU results are compared with THIS, byte for byte (tests/flow/test_gpu_fuzz_input.py).

State, per stream: a header { frames, gdx, gdy, support }, two luma planes (h rows of ALIGN(w, 16) bytes) and gw x gh records { dx, dy, cost,
spread } rounded up to 16 bytes.  Update: cur into P[f & 1], prev = P[(f & 1) ^ 1]; per block the legal candidate least under (cost, vx^2 + vy^2,
vy, vx), its cost and the spread to the largest cost; the vector most reliable blocks hold; the row.  Boxes: the motion gate's considered boxes and
clip, then per box the touched and the reliable blocks and the sums of their vectors less the global one."""
import numpy as np

from motion.motionref import BOX_DTYPE, DETS_DTYPE, f2i, luma_bgr, s32  # noqa: F401  (the record layouts and the draw contract's conversion)

DETS, ROW, WORDS, STATE_HEADER, MAX_SIDE = 128, 16, 8, 16, 8192
RECORD = np.dtype([("dx", "<i2"), ("dy", "<i2"), ("cost", "<u2"), ("spread", "<u2")])


class Spec:
    def __init__(self, w, h, block_log2, range_, min_spread=0, min_score=0.0, classes=None):
        self.w, self.h, self.block_log2, self.range, self.min_spread = w, h, block_log2, range_, min_spread
        self.min_score, self.classes = np.float32(min_score), None if classes is None else [bool(v) for v in classes]
        self.b = 1 << block_log2
        self.gw, self.gh = (w + self.b - 1) >> block_log2, (h + self.b - 1) >> block_log2
        # the candidates in the tie order: the first of equals is the least
        r = range(-range_, range_ + 1)
        self.cands = sorted(((vx, vy) for vy in r for vx in r), key=lambda v: (v[0] * v[0] + v[1] * v[1], v[1], v[0]))

    def allowed(self, type_):
        return self.classes is None or (0 <= int(type_) < len(self.classes) and self.classes[int(type_)])


def stream_nbytes(w, h, block_log2):
    b = 1 << block_log2
    return STATE_HEADER + 2 * ((w + 15) & ~15) * h + ((8 * ((w + b - 1) // b) * ((h + b - 1) // b) + 15) & ~15)


def state_nbytes(nstreams, w, h, block_log2):
    if not (1 <= nstreams <= 65536 and 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE and 3 <= block_log2 <= 4):
        return 0
    return nstreams * stream_nbytes(w, h, block_log2)


class State:
    """nstreams blocks of a header, the two planes and the records, as views of `raw`; all zero: empty"""

    def __init__(self, nstreams, w, h, block_log2, raw=None):
        b, pitch = 1 << block_log2, (w + 15) & ~15
        gw, gh, ro = (w + b - 1) // b, (h + b - 1) // b, STATE_HEADER + 2 * pitch * h
        self.raw = np.zeros((nstreams, stream_nbytes(w, h, block_log2)), np.uint8)
        if raw is not None:
            self.raw[:] = np.ascontiguousarray(raw, np.uint8).reshape(self.raw.shape)
        self.hdr = self.raw[:, :STATE_HEADER].view("<i4")
        self.planes = self.raw[:, STATE_HEADER:ro].reshape(nstreams, 2, h, pitch)[:, :, :, :w]
        self.recs = self.raw[:, ro:ro + 8 * gw * gh].view(RECORD).reshape(nstreams, gh, gw)
        assert np.shares_memory(self.planes, self.raw) and np.shares_memory(self.recs, self.raw)

    def tobytes(self):
        return self.raw.tobytes()


def reliable(spread, spec):
    return spread.astype(np.int64) >= max(spec.min_spread, 1)


def update_frame(luma, spec, hdr, planes, recs):
    """one frame of one stream: luma is h x w (0..255); hdr, planes and recs are the stream's, updated in place; returns the row"""
    w, h, b, gw, gh = spec.w, spec.h, spec.b, spec.gw, spec.gh
    f = int(hdr[0]) & 0xffffffff
    cur = np.asarray(luma).astype(np.int64)
    assert cur.shape == (h, w)
    planes[f & 1][:] = cur.astype(np.uint8)
    prev = planes[(f & 1) ^ 1].astype(np.int64)
    recs[:] = np.zeros((), RECORD)
    if f != 0:
        big = 1 << 40
        cost = np.full((len(spec.cands), gh, gw), big, np.int64)
        bx, by = np.arange(gw) * b, np.arange(gh) * b
        for n, (vx, vy) in enumerate(spec.cands):
            x0, x1, y0, y1 = max(0, vx), min(w, w + vx), max(0, vy), min(h, h + vy)          # the pixels p with p - v inside the frame
            if x0 >= x1 or y0 >= y1:
                continue
            d = np.zeros((gh * b, gw * b), np.int64)
            d[y0:y1, x0:x1] = np.abs(cur[y0:y1, x0:x1] - prev[y0 - vy:y1 - vy, x0 - vx:x1 - vx])
            legal = ((by >= y0) & (np.minimum(by + b, h) <= y1))[:, None] & ((bx >= x0) & (np.minimum(bx + b, w) <= x1))[None, :]
            cost[n] = np.where(legal, d.reshape(gh, b, gw, b).sum(axis=(1, 3)), big)
        win = cost.argmin(axis=0)                                                            # (the first of equal costs: the least in the tie order)
        least = cost.min(axis=0)
        most = np.where(cost == big, -1, cost).max(axis=0)
        cands = np.array(spec.cands)
        recs["dx"], recs["dy"], recs["cost"], recs["spread"] = cands[win, 0], cands[win, 1], least, np.minimum(most - least, 65535)
    rel = reliable(recs["spread"], spec)
    votes = [int((rel & (recs["dx"] == vx) & (recs["dy"] == vy)).sum()) for vx, vy in spec.cands]
    g = int(np.argmax(votes))                                                                # (the first of equal counts)
    support = votes[g]
    gdx, gdy = spec.cands[g] if support else (0, 0)
    hdr[:] = (s32((f + 1) % 2 ** 32), gdx, gdy, support)
    return [s32(f), gw * gh, int(rel.sum()), int(rel.sum()) - support, gdx, gdy, support] + [0] * 9


def update(lumas, streams, spec, state):
    """frame t (an h x w luma array, or None: a NULL pixel address) is the next frame of stream streams[t] (-1: ignored); the state is updated in
    place, in the order given; returns the rows, n x ROW int32"""
    rows = np.zeros((len(streams), ROW), np.int32)
    for t, s in enumerate(streams):
        if s >= 0 and lumas[t] is not None:
            rows[t] = update_frame(lumas[t], spec, state.hdr[s], state.planes[s], state.recs[s])
    return rows


def boxes(recs, flat, stride, first, streams, spec, state):
    """record t belongs to stream streams[t] (-1: ignored); flat None: the records' own boxes; first: the lists' starts (None: t x stride); the state
    is only read.  Returns the words, n x (WORDS + 4 stride) int32."""
    k, w, h = spec.block_log2, spec.w, spec.h
    words = np.zeros((len(streams), WORDS + 4 * stride), np.int32)
    for t, s in enumerate(streams):
        if s < 0:
            continue
        r = recs[t]
        if flat is None:
            lst = r["box"][:max(0, min(int(r["count"]), stride))]
        else:
            f0 = first[t] if first is not None else t * stride
            lst = flat[f0:f0 + max(0, min(int(r["nfull"]), stride))]
        with np.errstate(invalid="ignore"):
            ok = [i for i in range(len(lst)) if lst[i]["score"] >= spec.min_score and spec.allowed(lst[i]["type"])]
        hdr, br = state.hdr[s], state.recs[s]
        rel = reliable(br["spread"], spec)
        outside = 0
        for i in ok[:DETS]:
            a_, b_, c_, d_ = (f2i(lst[i][n]) for n in ("x1", "y1", "x2", "y2"))
            X0, Y0, X1, Y1 = max(a_, 0), max(b_, 0), min(c_, w - 1), min(d_, h - 1)
            if a_ > c_ or b_ > d_ or X0 > X1 or Y0 > Y1:
                outside += 1
                continue
            sub = (slice(Y0 >> k, (Y1 >> k) + 1), slice(X0 >> k, (X1 >> k) + 1))
            m = rel[sub]
            words[t, WORDS + 4 * i:WORDS + 4 * i + 4] = (m.size, int(m.sum()), s32(int((br["dx"][sub].astype(np.int64) - int(hdr[1]))[m].sum())),
                                                         s32(int((br["dy"][sub].astype(np.int64) - int(hdr[2]))[m].sum())))
        words[t, :WORDS] = (min(len(ok), DETS), min(max(0, len(ok) - DETS), 2 ** 31 - 1), outside, hdr[0], hdr[1], hdr[2], hdr[3], 0)
    return words
