#!/usr/bin/env python3
"""Device time of the blur launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12) with seeded boxes, the
operator forms, 20 warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  The workload is
tools/redact_bench.py's, and in the same run the redact MOSAIC 16 is timed on the same cases as the yardstick whose code the blur does not touch:
every blur time is also given as a multiple of it.  Next to each time its byte model per call, computed here from the boxes: per pass the tile
(bw + 2 r)(bh + 2 r) x channels of every 64 x 64 block with a covered pixel, clipped to the frame (read), |S| written to the scratch, |S| read and
written again by the copy-back.
Prints one JSON object; with a path argument it is written there too:  python tools/blur_bench.py [profiles/blur_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, CELL, NBOX, PEAK, BLOCK = 64, 1920, 1080, 16, 8, 8e12, 64
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"frames": B, "size": [W, H], "boxes_per_frame": NBOX, "warmup": 20, "timed": 100, "peak_bytes_per_s": PEAK, "yardstick": "redact MOSAIC %d" % CELL}


def timed(busy, fn):
    """median device time of fn's launches: `busy` is enqueued in front of every sample, so the host runs ahead of the device and the two events
    bracket fn's kernels alone, not the host's enqueue pace"""
    for _ in range(20):
        busy()
        assert fn() == 0, F.last_error()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for a, b in ev:
        busy()
        a.record(st)
        fn()
        b.record(st)
    st.synchronize()
    us = sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)
    return {"median_us": round(us[50], 2), "min_us": round(us[0], 2), "p90_us": round(us[90], 2)}


def covered(b, qualifies, outside):
    u = np.zeros((H, W), bool)
    if qualifies:
        for x1, y1, x2, y2 in b:
            u[max(y1, 0):min(y2, H - 1) + 1, max(x1, 0):min(x2, W - 1) + 1] = True
    return ~u if outside else u


def tile_bytes(mask, r, nc):
    """the bytes of the tiles of the blocks of `mask` (a plane's covered pixels) that have a set pixel: block +- r, clipped to the plane"""
    h, w = mask.shape
    total = 0
    for by in range(0, h, BLOCK):
        for bx in range(0, w, BLOCK):
            if mask[by:by + BLOCK, bx:bx + BLOCK].any():
                total += (min(bx + BLOCK + r, w) - max(bx - r, 0)) * (min(by + BLOCK + r, h) - max(by - r, 0)) * nc
    return total


def byte_model(boxes, qualifies, outside, r, passes, nv12):
    """(bytes read, bytes written) of one call by the kernel's structure"""
    rd = wr = 0
    for b in boxes:
        s = covered(b, qualifies, outside)
        if nv12:
            c = s.reshape(H // 2, 2, W // 2, 2).any((1, 3))                       # the chroma samples the FILL rule covers (even sizes)
            # a chroma block is the 32 x 32 samples of a luma block: tile_bytes on the sample mask with blocks of 64 would merge four of them
            tiles = tile_bytes(s, r, 1) + sum((min(bx + 32 + (r + 1) // 2, W // 2) - max(bx - (r + 1) // 2, 0)) * (min(by + 32 + (r + 1) // 2, H // 2) - max(by - (r + 1) // 2, 0)) * 2
                                             for by in range(0, H // 2, 32) for bx in range(0, W // 2, 32) if c[by:by + 32, bx:bx + 32].any())
            cov = int(s.sum()) + 2 * int(c.sum())
        else:
            tiles, cov = tile_bytes(s, r, 3), 3 * int(s.sum())
        rd += passes * (tiles + cov)
        wr += passes * 2 * cov
    return rd, wr


rng = np.random.default_rng(522)
boxes = []                                                                         # 8 boxes of about 200 x 200 per frame, anywhere inside (tools/redact_bench.py's)
for t in range(B):
    x1, y1 = rng.integers(0, W - 230, NBOX), rng.integers(0, H - 230, NBOX)
    boxes.append([(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in zip(x1, y1, rng.integers(170, 230, NBOX), rng.integers(170, 230, NBOX))])
recs = np.zeros(B, F.DETS_DTYPE)
for t in range(B):
    recs[t]["count"] = recs[t]["nfull"] = NBOX
    recs[t]["box"]["score"][:NBOX] = 0.5
    for k, (a, b, c, d) in enumerate(boxes[t]):
        recs[t]["box"][k]["x1"], recs[t]["box"][k]["y1"], recs[t]["box"][k]["x2"], recs[t]["box"][k]["y2"] = a + 0.5, b + 0.5, c + 0.5, d + 0.5
d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()

with torch.cuda.stream(st):
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    bgr = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    bgr_s = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    nv = [(torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device="cuda")) for _ in range(B)]
    nv_s = [(torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros((H // 2, W), dtype=torch.uint8, device="cuda")) for _ in range(B)]
st.synchronize()
tabs = {False: F.bgr_frame_table(bgr), True: F.nv12_frame_table(nv)}
stabs = {False: F.bgr_frame_table(bgr_s), True: F.nv12_frame_table(nv_s)}
blur = {False: L.ffgpu_blur_boxes_bgr_dev, True: L.ffgpu_blur_boxes_nv12_dev}
redact = {False: L.ffgpu_redact_boxes_bgr_dev, True: L.ffgpu_redact_boxes_nv12_dev}


def busy():
    with torch.cuda.stream(st):
        flush.zero_()


CASES = (("a_no_qualifying_box", dict(min_score=0.9), False, False), ("b_8_boxes", dict(), True, False), ("c_outside", dict(outside=True), True, True))
for nv12 in (False, True):
    fmt = "nv12_" if nv12 else "bgr_"
    for name, kw, qualifies, outside in CASES:
        spec = F.redact_spec(F.REDACT_MOSAIC, CELL, **kw)
        m = timed(busy, lambda: redact[nv12](d_recs.data_ptr(), None, 0, None, tabs[nv12], B, spec, S))
        out[fmt + name + "_mosaic16"] = m
        for r in (8, 31):
            for passes in (1, 3):
                spec = F.blur_spec(r, passes, **kw)
                t = timed(busy, lambda: blur[nv12](d_recs.data_ptr(), None, 0, None, tabs[nv12], stabs[nv12], B, spec, S))
                rd, wr = byte_model(boxes, qualifies, outside, r, passes, nv12)
                t["model_bytes_read"], t["model_bytes_written"] = rd, wr
                t["model_GB_per_s"] = round((rd + wr) / (t["median_us"] * 1e-6) / 1e9, 1)
                t["fraction_of_peak"] = round((rd + wr) / (t["median_us"] * 1e-6) / PEAK, 4)
                t["times_mosaic16"] = round(t["median_us"] / m["median_us"], 2)
                out["%s%s_r%d_p%d" % (fmt, name, r, passes)] = t
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
