#!/usr/bin/env python3
"""Device time of the zones pass: ffgpu_exec_zones behind a batch-64 forward of data/test.bmp (3 boxes per entry) and the tracker whose
ids it reads, as 64 video streams x 1 frame and as 1 video stream x 64 frames, every scene with 8 zones of 8 vertices and 8 lines, beside
ffgpu_exec_track on the same executor in the same run (the yardstick: the existing per-stream post-pass of the same idiom).  HIP events on one
stream, one process, the measurements alternating over `repeats` rounds of 20 warm-up + 100 timed launches, a forward enqueued in front of every
sample so that the events bracket device work and not the host's pace (tools/track_bench.py's sampling).  Prints one JSON object; with a path
argument it is written there too:  python tools/zones_bench.py [profiles/zones_bench.json]"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, REPEATS = 64, 3
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"batch": B, "warmup": 20, "timed": 100, "repeats": REPEATS}


def timed(busy, fn):
    for _ in range(20):
        busy()
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for a, b in ev:
        busy()
        a.record(st)
        assert fn() == 0
        b.record(st)
    st.synchronize()
    return sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)


def dev_zeros(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
pic = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
ftab = F.bgr_frame_table([(pic.data_ptr(), w, h, rows.shape[1])] * B)
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
# 8 octagons round points spread over the picture (every box's anchor is inside some of them), 8 lines across it
octagon = lambda cx, cy, r: [(round(cx + r * math.cos(k * math.pi / 4)), round(cy + r * math.sin(k * math.pi / 4))) for k in range(8)]   # noqa: E731
scene = F.scene([(octagon(80 + 70 * z, 212, 60 + 25 * z), 2) for z in range(8)],
                [((-10, 40 + 45 * l), (w + 10, 40 + 45 * l)) if l % 2 else ((40 + 70 * l, -10), (40 + 70 * l, h + 10)) for l in range(8)])
F.scene_check([scene])
tspec = F.track_spec(32, max_missed=2, min_hits=1, iou_thresh=0.3)
zspec = F.zones_spec(32, max_missed=2, identity=F.ZONES_IDS, gate_zone=0xff)
net = F.Net()
with net.executor(B) as ex:
    cap = ex.cand_capacity
    ids, orecs, olists = dev_zeros(4 * B * (8 + cap)), dev_zeros(F.DETS_DTYPE.itemsize * B), dev_zeros(24 * B * cap)
    events, grecs, glists = dev_zeros(4 * B * (F.ZONES_ROW + 2 * cap)), dev_zeros(F.DETS_DTYPE.itemsize * B), dev_zeros(24 * B * cap)
    scenes = torch.from_numpy(np.frombuffer(F.scenes_bytes([scene] * B), np.uint8).copy()).cuda()
    tstate64, tstate1 = dev_zeros(F.track_state_bytes(B, 32)), dev_zeros(F.track_state_bytes(1, 32))
    zstate64, zstate1 = dev_zeros(F.zones_state_bytes(B, 32)), dev_zeros(F.zones_state_bytes(1, 32))
    each, one = (C.c_int * B)(*range(B)), (C.c_int * B)(*([0] * B))
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)                                                        # noqa: E731
    t64 = lambda: L.ffgpu_exec_track(ex.h, 0, each, B, tspec, tstate64.data_ptr(), B, ids.data_ptr(), orecs.data_ptr(), olists.data_ptr(), S)   # noqa: E731
    t1 = lambda: L.ffgpu_exec_track(ex.h, 0, one, B, tspec, tstate1.data_ptr(), 1, ids.data_ptr(), orecs.data_ptr(), olists.data_ptr(), S)      # noqa: E731
    z64 = lambda: L.ffgpu_exec_zones(ex.h, 0, each, B, zspec, scenes.data_ptr(), zstate64.data_ptr(), B, ids.data_ptr(), events.data_ptr(),   # noqa: E731
                                     grecs.data_ptr(), glists.data_ptr(), S)
    z1 = lambda: L.ffgpu_exec_zones(ex.h, 0, one, B, zspec, scenes.data_ptr(), zstate1.data_ptr(), 1, ids.data_ptr(), events.data_ptr(),     # noqa: E731
                                    grecs.data_ptr(), glists.data_ptr(), S)
    z1_events = lambda: L.ffgpu_exec_zones(ex.h, 0, one, B, zspec, scenes.data_ptr(), zstate1.data_ptr(), 1, ids.data_ptr(), events.data_ptr(),   # noqa: E731
                                           None, None, S)
    assert fwd() == 0 and t64() == 0 and z64() == 0 and z1() == 0, F.last_error()
    st.synchronize()
    got = events.cpu().numpy().view("<i4").reshape(B, F.ZONES_ROW + 2 * cap)
    assert (got[:, 0] == 3).all() and (got[1:, 1] == 3).all() and got[:, 16:48:4].sum() > 0, got[:, :10]      # 3 boxes, known from the second frame on, inside something
    out["boxes_per_entry"], out["list_stride"], out["zones"], out["lines"], out["verts"] = 3, cap, 8, 8, 8
    samples = {"zones_64_streams_x_1_frame": [], "zones_1_stream_x_64_frames": [], "zones_1_stream_x_64_frames_events_only": [],
               "track_64_streams_x_1_frame": [], "track_1_stream_x_64_frames": [], "forward": []}
    for _ in range(REPEATS):
        samples["zones_64_streams_x_1_frame"] += timed(fwd, z64)
        samples["track_64_streams_x_1_frame"] += timed(fwd, t64)
        samples["zones_1_stream_x_64_frames"] += timed(fwd, z1)
        samples["track_1_stream_x_64_frames"] += timed(fwd, t1)
        samples["zones_1_stream_x_64_frames_events_only"] += timed(fwd, z1_events)
        samples["forward"] += timed(fwd, fwd)
    for k, v in samples.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
    for shape in ("64_streams_x_1_frame", "1_stream_x_64_frames"):
        out["ratio_zones_over_track_" + shape] = round(out["zones_" + shape]["median_us"] / out["track_" + shape]["median_us"], 3)
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
