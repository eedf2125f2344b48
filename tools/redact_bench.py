#!/usr/bin/env python3
"""Device time of the redact launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12) with seeded boxes, the
operator forms, 20 warm-up + 100 timed calls, median.  Next to each time its byte model, computed here from the boxes: the bytes of the cells that
have a covered pixel (read; MOSAIC only) plus the covered bytes (written), and what that is in GB/s and as a fraction of the 8 TB/s peak.
Prints one JSON object; with a path argument it is written there too:  python tools/redact_bench.py [profiles/redact_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, CELL, NBOX, PEAK = 64, 1920, 1080, 16, 8, 8e12
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"frames": B, "size": [W, H], "cell": CELL, "boxes_per_frame": NBOX, "warmup": 20, "timed": 100, "peak_bytes_per_s": PEAK}


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


def cells_any(mask, s):
    """(cells down, cells across) bool: the cell of side s has a set pixel; and every cell's clipped pixel count"""
    h, w = mask.shape
    p = np.zeros((-(-h // s) * s, -(-w // s) * s), bool)
    p[:h, :w] = mask
    n = np.zeros(p.shape, np.int64)
    n[:h, :w] = 1
    return p.reshape(p.shape[0] // s, s, p.shape[1] // s, s).any((1, 3)), n.reshape(p.shape[0] // s, s, p.shape[1] // s, s).sum((1, 3))


def byte_model(boxes, qualifies, outside, mosaic, nv12):
    """(bytes read, bytes written) of one call by the contract: per frame the covered set S from the integer boxes, the cells with a pixel in S"""
    rd = wr = 0
    for b in boxes:
        u = np.zeros((H, W), bool)
        if qualifies:
            for x1, y1, x2, y2 in b:
                u[max(y1, 0):min(y2, H - 1) + 1, max(x1, 0):min(x2, W - 1) + 1] = True
        s = ~u if outside else u
        c = s.reshape(H // 2, 2, W // 2, 2).any((1, 3))                            # the chroma samples the FILL rule covers (even sizes)
        wr += int(s.sum()) * (1 if nv12 else 3) + (2 * int(c.sum()) if nv12 else 0)
        if mosaic:
            some, n = cells_any(s, CELL)
            rd += int(n[some].sum()) * (1 if nv12 else 3)
            if nv12:
                some, n = cells_any(c, CELL // 2)
                rd += 2 * int(n[some].sum())
    return rd, wr


rng = np.random.default_rng(522)
boxes = []                                                                         # 8 boxes of about 200 x 200 per frame, anywhere inside, not aligned to the cells
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
    scratch = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    bgr = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    nv = [(torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device="cuda")) for _ in range(B)]
st.synchronize()
tabs = {False: F.bgr_frame_table(bgr), True: F.nv12_frame_table(nv)}
fns = {False: L.ffgpu_redact_boxes_bgr_dev, True: L.ffgpu_redact_boxes_nv12_dev}


def busy():
    with torch.cuda.stream(st):
        scratch.zero_()


CASES = (("a_no_qualifying_box_mosaic16", F.redact_spec(F.REDACT_MOSAIC, CELL, min_score=0.9), False, False, True),
         ("b_8_boxes_mosaic16", F.redact_spec(F.REDACT_MOSAIC, CELL), True, False, True),
         ("b_8_boxes_fill", F.redact_spec(F.REDACT_FILL, color=(16, 128, 128)), True, False, False),
         ("c_outside_mosaic16", F.redact_spec(F.REDACT_MOSAIC, CELL, outside=True), True, True, True))
for nv12 in (False, True):
    for name, spec, qualifies, outside, mosaic in CASES:
        r = timed(busy, lambda: fns[nv12](d_recs.data_ptr(), None, 0, None, tabs[nv12], B, spec, S))
        rd, wr = byte_model(boxes, qualifies, outside, mosaic, nv12)
        r["model_bytes_read"], r["model_bytes_written"] = rd, wr
        r["model_GB_per_s"] = round((rd + wr) / (r["median_us"] * 1e-6) / 1e9, 1)
        r["fraction_of_peak"] = round((rd + wr) / (r["median_us"] * 1e-6) / PEAK, 4)
        out[("nv12_" if nv12 else "bgr_") + name] = r
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
