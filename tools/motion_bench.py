#!/usr/bin/env python3
"""Device time of the motion map launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12), one video stream each,
the operator forms, 20 warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  The update call (k_motion_update and
the small k_motion_row launch behind it) for cells of 8, 16 and 64 pixels, with its algorithmic bytes -- 3 + 2 + 2 a pixel in BGR, 1 + 2 + 2 in NV12
-- as bytes/s and as a fraction of 8 TB/s.  In the same run, on the same frames and ALTERNATING with it sample by sample, the yardstick whose code
the motion maps do not touch: ffgpu_redact_boxes_*_dev MOSAIC 16 with OUTSIDE, which reads every pixel once and writes it once (6 and 3 bytes a
pixel); every update time is also given as a multiple of it.  The gate on 64 records of 8 boxes, 64 streams.
Prints one JSON object; with a path argument it is written there too:  python tools/motion_bench.py [profiles/motion_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, NBOX, PEAK = 64, 1920, 1080, 8, 8e12
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"frames": B, "size": [W, H], "warmup": 20, "timed": 100, "peak_bytes_per_s": PEAK, "yardstick": "redact MOSAIC 16 OUTSIDE, alternating with the update"}


def summary(us):
    us = sorted(us)
    return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "p90_us": round(us[(9 * len(us)) // 10], 2)}


def timed(busy, fns):
    """median device time of each of fns' launches, taken alternating: `busy` is enqueued in front of every sample, so the host runs ahead of the
    device and the two events bracket the function's kernels alone, not the host's enqueue pace"""
    for _ in range(20):
        for fn in fns:
            busy()
            assert fn() == 0, F.last_error()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(100)]
    for sample in ev:
        for fn, (a, b) in zip(fns, sample):
            busy()
            a.record(st)
            fn()
            b.record(st)
    st.synchronize()
    return [summary([sample[i][0].elapsed_time(sample[i][1]) * 1000.0 for sample in ev]) for i in range(len(fns))]


rng = np.random.default_rng(530)
recs = np.zeros(B, F.DETS_DTYPE)                                                   # 8 boxes of about 200 x 200 per frame, anywhere inside (tools/heat_bench.py's)
for t in range(B):
    x1, y1 = rng.integers(0, W - 230, NBOX), rng.integers(0, H - 230, NBOX)
    recs[t]["count"] = recs[t]["nfull"] = NBOX
    recs[t]["box"]["score"][:NBOX] = 0.5
    for k, (a, b, c, d) in enumerate(zip(x1, y1, rng.integers(170, 230, NBOX), rng.integers(170, 230, NBOX))):
        recs[t]["box"][k]["x1"], recs[t]["box"][k]["y1"], recs[t]["box"][k]["x2"], recs[t]["box"][k]["y2"] = a + 0.5, b + 0.5, a + c + 0.5, b + d + 0.5
d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()

with torch.cuda.stream(st):
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    bgr = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    nv = [(torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device="cuda")) for _ in range(B)]
st.synchronize()
tabs = {False: F.bgr_frame_table(bgr), True: F.nv12_frame_table(nv)}
update = {False: L.ffgpu_motion_update_bgr_dev, True: L.ffgpu_motion_update_nv12_dev}
redact = {False: L.ffgpu_redact_boxes_bgr_dev, True: L.ffgpu_redact_boxes_nv12_dev}
streams = (F.C.c_int * B)(*range(B))


def busy():
    with torch.cuda.stream(st):
        flush.zero_()


d_rows = torch.zeros(4 * F.MOTION_ROW * B, dtype=torch.uint8, device="cuda")
for k in (3, 4, 6):
    ms = F.motion_spec(W, H, k, 16, 4, 8, max(1, (1 << (2 * k)) // 8), 64, 30)
    nstate = F.motion_state_bytes(B, W, H, k)
    d_state = torch.zeros(nstate, dtype=torch.uint8, device="cuda")
    for nv12 in (False, True):
        rspec = F.redact_spec(F.REDACT_MOSAIC, 16, outside=True)
        t, y = timed(busy, [lambda: update[nv12](tabs[nv12], B, streams, ms, d_state.data_ptr(), B, d_rows.data_ptr(), S),
                            lambda: redact[nv12](d_recs.data_ptr(), None, 0, None, tabs[nv12], B, rspec, S)])
        nbytes = B * W * H * ((1 if nv12 else 3) + 2 + 2)
        t["algorithmic_bytes"] = nbytes
        t["GB_per_s"] = round(nbytes / (t["median_us"] * 1e-6) / 1e9, 1)
        t["fraction_of_peak"] = round(nbytes / (t["median_us"] * 1e-6) / PEAK, 4)
        t["times_yardstick"] = round(t["median_us"] / y["median_us"], 2)
        ybytes = B * W * H * (3 if nv12 else 6)
        y["algorithmic_bytes"], y["fraction_of_peak"] = ybytes, round(ybytes / (y["median_us"] * 1e-6) / PEAK, 4)
        t["state_bytes"] = nstate
        name = "%s_cell%d" % ("nv12" if nv12 else "bgr", 1 << k)
        out["update_" + name], out["yardstick_" + name] = t, y
    if k == 4:                                                                     # the gate on the state the updates left: 64 records of 8 boxes
        d_words = torch.zeros(4 * B * (F.MOTION_WORDS + 2 * 128), dtype=torch.uint8, device="cuda")
        d_orecs = torch.zeros(B * F.DETS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        out["gate_64_records_x_8_boxes"] = timed(busy, [lambda: L.ffgpu_motion_gate_dev(d_recs.data_ptr(), None, 0, None, streams, B, ms, d_state.data_ptr(), B,
                                                                                          d_words.data_ptr(), d_orecs.data_ptr(), None, S)])[0]
        out["gate_64_records_x_8_boxes_words_only"] = timed(busy, [lambda: L.ffgpu_motion_gate_dev(d_recs.data_ptr(), None, 0, None, streams, B, ms, d_state.data_ptr(), B,
                                                                                                     d_words.data_ptr(), None, None, S)])[0]
    del d_state
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
