#!/usr/bin/env python3
"""Device time of the flow map launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12), one video stream each,
the operator forms, 20 warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  The update call (k_flow_match and
the small k_flow_row launch behind it) at (block, range) = (8, 8) and (16, 16), next to the ARITHMETIC FLOOR it derives -- candidates x pixels / 16
byte differences a lane instruction (one v_qsad_pk_u16_u8), over 256 CUs x 64 lanes x 2.4 GHz lane instructions a second -- and, in the same run, on
the same frames and ALTERNATING with it sample by sample, the motion update (cells of 16) whose code the flow maps do not touch: from this library,
or from the library named by a second argument (a build of the parent commit).  The box operator on 64 records of 8 boxes, 64 streams.
Prints one JSON object; with a path argument it is written there too:  python tools/flow_bench.py [profiles/flow_bench.json [parent libffcnn_hip.so]]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, NBOX, LANE_RATE = 64, 1920, 1080, 8, 256 * 64 * 2.4e9
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
M = L
if len(sys.argv) > 2:                                                              # the motion update of another build, with this library's argument types
    M = F.C.CDLL(sys.argv[2])
    for name in ("ffgpu_motion_update_bgr_dev", "ffgpu_motion_update_nv12_dev"):
        getattr(M, name).argtypes = getattr(L, name).argtypes
out = {"frames": B, "size": [W, H], "warmup": 20, "timed": 100, "lane_instructions_per_s": LANE_RATE,
       "yardstick": "motion update, cells of 16, alternating with the flow update; library: %s" % (sys.argv[2] if len(sys.argv) > 2 else "this one")}


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


rng = np.random.default_rng(535)
recs = np.zeros(B, F.DETS_DTYPE)                                                   # 8 boxes of about 200 x 200 per frame, anywhere inside (tools/motion_bench.py's)
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
flow = {False: L.ffgpu_flow_update_bgr_dev, True: L.ffgpu_flow_update_nv12_dev}
motion = {False: M.ffgpu_motion_update_bgr_dev, True: M.ffgpu_motion_update_nv12_dev}
streams = (F.C.c_int * B)(*range(B))


def busy():
    with torch.cuda.stream(st):
        flush.zero_()


d_rows = torch.zeros(4 * 16 * B, dtype=torch.uint8, device="cuda")
ms = F.motion_spec(W, H, 4, 16, 4, 8, 32, 64, 30)
d_mstate = torch.zeros(F.motion_state_bytes(B, W, H, 4), dtype=torch.uint8, device="cuda")
for k, r in ((3, 8), (4, 16)):
    fs = F.flow_spec(W, H, k, r, 64)
    nstate = F.flow_state_bytes(B, W, H, k)
    d_state = torch.zeros(nstate, dtype=torch.uint8, device="cuda")
    for nv12 in (False, True):
        t, y = timed(busy, [lambda: flow[nv12](tabs[nv12], B, streams, fs, d_state.data_ptr(), B, d_rows.data_ptr(), S),
                            lambda: motion[nv12](tabs[nv12], B, streams, ms, d_mstate.data_ptr(), B, d_rows.data_ptr(), S)])
        floor_us = (2 * r + 1) ** 2 * B * W * H / 16 / LANE_RATE * 1e6
        t["candidates"], t["floor_us"], t["times_floor"] = (2 * r + 1) ** 2, round(floor_us, 1), round(t["median_us"] / floor_us, 2)
        t["byte_differences_per_s"] = round((2 * r + 1) ** 2 * B * W * H / (t["median_us"] * 1e-6), -9)
        t["times_motion_update"], t["state_bytes"] = round(t["median_us"] / y["median_us"], 2), nstate
        name = "%s_block%d_range%d" % ("nv12" if nv12 else "bgr", 1 << k, r)
        out["update_" + name], out["motion_update_" + name] = t, y
    if k == 3:                                                                     # the box operator on the state the updates left: 64 records of 8 boxes
        d_words = torch.zeros(4 * B * (F.FLOW_WORDS + 4 * 128), dtype=torch.uint8, device="cuda")
        out["boxes_64_records_x_8_boxes"] = timed(busy, [lambda: L.ffgpu_flow_boxes_dev(d_recs.data_ptr(), None, 0, None, streams, B, fs, d_state.data_ptr(), B,
                                                                                         d_words.data_ptr(), S)])[0]
    del d_state
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
