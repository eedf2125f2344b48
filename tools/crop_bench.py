#!/usr/bin/env python3
"""Device time of the cut: 64 slots of 320 x 320 fp32 from 64 regions of 1920 x 1080 BGR frames through ffgpu_crop_boxes_bgr_dev
(k_crop_select + k_crop_pixels) beside the staging launch of ffgpu_exec_forward_bgr_frames_dev (k_input4 over a frame table) for the same 64
regions given as host descriptors.  HIP events on one stream, one process, the three measurements alternating over `repeats` rounds of 20 warm-up +
100 timed launches, a forward enqueued in front of every sample so that the events bracket device work and not the host's pace.  The staging
launch has no entry point of its own: it is the staged forward_bgr_frames_dev (FFGPU_NO_U8_FRONT=1, table unchanged) minus forward_dev on the same
executor and graph.  Prints one JSON object; with a path argument it is written there too:  python tools/crop_bench.py [profiles/crop_bench.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

os.environ["FFGPU_NO_U8_FRONT"] = "1"                                  # the frame table is staged by k_input4, not read by the first kernel
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, REPEATS = 64, 1920, 1080, 3
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
rng = np.random.default_rng(518)
out = {"batch": B, "frame": [W, H], "slot": [320, 320], "warmup": 20, "timed": 100, "repeats": REPEATS}


def timed(busy, fn):
    for _ in range(20):
        busy()
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for a, b in ev:
        busy()
        a.record(st)
        fn()
        b.record(st)
    st.synchronize()
    return sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)


frames = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(B)]
ftab = F.bgr_frame_table(frames)
recs = np.zeros(B, F.DETS_DTYPE)
regions = []
for t in range(B):                                                       # one box per frame: 120 .. 900 pixels wide, 90 .. 700 high, anywhere in the frame
    w, h = int(rng.integers(120, 901)), int(rng.integers(90, 701))
    x0, y0 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
    recs[t]["count"] = recs[t]["nfull"] = 1
    recs[t]["box"][0] = (0, 0.9, x0, y0, x0 + w - 1 + 0.5, y0 + h - 1 + 0.5)
    regions.append((frames[t].data_ptr() + y0 * 3 * W + 3 * x0, w, h, 3 * W))
rtab = F.bgr_frame_table(regions)
d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
spec = F.crop_spec(320, 320, F.CROP_F32, per_target=1)
slots = torch.zeros(B * 3 * 320 * 320, dtype=torch.float32, device="cuda")
table = torch.zeros(F.crop_table_bytes(B), dtype=torch.uint8, device="cuda")
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
net = F.Net()
with net.executor(B) as ex:
    fwd_dev = lambda: L.ffgpu_exec_forward_dev(ex.h, slots.data_ptr(), S)
    fwd_frames = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, rtab, B, mean, norm, S)
    crop = lambda: L.ffgpu_crop_boxes_bgr_dev(d_recs.data_ptr(), None, 0, None, ftab, B, spec, slots.data_ptr(), table.data_ptr(), B, S)
    assert crop() == 0 and fwd_frames() == 0 and fwd_dev() == 0
    st.synchronize()
    hdr, ent = F.crop_table(table.cpu().numpy())
    assert hdr["taken"] == B and [(int(e["w"]), int(e["h"])) for e in ent] == [(r[1], r[2]) for r in regions]
    samples = {"cut": [], "staged_forward": [], "forward": []}
    for _ in range(REPEATS):
        samples["cut"] += timed(fwd_dev, crop)
        samples["staged_forward"] += timed(fwd_dev, fwd_frames)
        samples["forward"] += timed(fwd_dev, fwd_dev)
    for k, v in samples.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
    out["staging_launch_us"] = round(out["staged_forward"]["median_us"] - out["forward"]["median_us"], 2)
    out["cut_over_staging"] = round(out["cut"]["median_us"] / out["staging_launch_us"], 3)
    out["bytes_written"] = B * 3 * 320 * 320 * 4
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
