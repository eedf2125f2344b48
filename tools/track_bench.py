#!/usr/bin/env python3
"""Device time of the tracker: ffgpu_exec_track behind a batch-64 forward of data/test.bmp (3 boxes per entry), as 64 video streams
x 1 frame and as 1 video stream x 64 frames, beside ffgpu_exec_merge_tiles on the same executor (64 pictures of one tile: the existing one-launch
post-pass of the same idiom), and the operator's worst cases on one record: 128 tracks x 128 detections, all distinct (one matching round) and all
identical (every pair ties: 128 rounds).  HIP events on one stream, one process, the measurements alternating over `repeats` rounds of 20 warm-up +
100 timed launches, a forward enqueued in front of every sample so that the events bracket device work and not the host's pace.  Prints one JSON
object; with a path argument it is written there too:  python tools/track_bench.py [profiles/track_bench.json]"""
import ctypes as C
import json
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
spec = F.track_spec(32, max_missed=2, min_hits=2, iou_thresh=0.3)
net = F.Net()
with net.executor(B) as ex:
    cap = ex.cand_capacity
    ids, orecs, olists = dev_zeros(4 * B * (8 + cap)), dev_zeros(F.DETS_DTYPE.itemsize * B), dev_zeros(24 * B * cap)
    state64, state1 = dev_zeros(F.track_state_bytes(B, 32)), dev_zeros(F.track_state_bytes(1, 32))
    each, one = (C.c_int * B)(*range(B)), (C.c_int * B)(*([0] * B))
    tiles = F.tile_table([(t, 0, 0) for t in range(B)])
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)
    t64 = lambda: L.ffgpu_exec_track(ex.h, 0, each, B, spec, state64.data_ptr(), B, ids.data_ptr(), orecs.data_ptr(), olists.data_ptr(), S)
    t1 = lambda: L.ffgpu_exec_track(ex.h, 0, one, B, spec, state1.data_ptr(), 1, ids.data_ptr(), orecs.data_ptr(), olists.data_ptr(), S)
    t1_ids = lambda: L.ffgpu_exec_track(ex.h, 0, one, B, spec, state1.data_ptr(), 1, ids.data_ptr(), None, None, S)
    mrg = lambda: L.ffgpu_exec_merge_tiles(ex.h, tiles, B, B, S)
    assert fwd() == 0 and t64() == 0 and t1() == 0 and mrg() == 0, F.last_error()
    st.synchronize()
    got = ids.cpu().numpy().view("<i4").reshape(B, 8 + cap)
    assert (got[:, 0] == 3).all() and (got[1:, 1] == 3).all(), got[:, :8]
    out["boxes_per_entry"], out["list_stride"] = 3, cap
    # the worst cases, on the operator: one record of 128 boxes against a state that holds their 128 tracks
    worst = {}
    for name in ("distinct", "ties"):
        recs = np.zeros(1, F.DETS_DTYPE)
        recs[0]["count"] = recs[0]["nfull"] = 128
        for k in range(128):
            x, y = (40.0 * (k % 16), 40.0 * (k // 16)) if name == "distinct" else (10.0, 10.0)
            recs[0]["box"][k] = (1, 0.5, x, y, x + 30.0, y + 30.0)
        d = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
        wspec = F.track_spec(128, max_missed=2, min_hits=1, iou_thresh=0.5)
        wstate, wids, wrec = dev_zeros(F.track_state_bytes(1, 128)), dev_zeros(4 * (8 + 128)), dev_zeros(F.DETS_DTYPE.itemsize)
        zero = (C.c_int * 1)(0)
        worst[name] = (lambda d=d, wspec=wspec, wstate=wstate, wids=wids, wrec=wrec, zero=zero:
                       L.ffgpu_track_boxes_dev(d.data_ptr(), None, 0, None, zero, 1, wspec, wstate.data_ptr(), 1, wids.data_ptr(), wrec.data_ptr(), None, S))
        assert worst[name]() == 0 and worst[name]() == 0
        st.synchronize()
        assert list(wids.cpu().numpy().view("<i4")[:3]) == [128, 128, 0]
    samples = {"track_64_streams_x_1_frame": [], "track_1_stream_x_64_frames": [], "track_1_stream_x_64_frames_ids_only": [], "merge_tiles_64_pictures": [],
               "worst_128x128_distinct": [], "worst_128x128_all_ties": [], "forward": []}
    for _ in range(REPEATS):
        samples["track_64_streams_x_1_frame"] += timed(fwd, t64)
        samples["track_1_stream_x_64_frames"] += timed(fwd, t1)
        samples["track_1_stream_x_64_frames_ids_only"] += timed(fwd, t1_ids)
        samples["merge_tiles_64_pictures"] += timed(fwd, mrg)
        samples["worst_128x128_distinct"] += timed(fwd, worst["distinct"])
        samples["worst_128x128_all_ties"] += timed(fwd, worst["ties"])
        samples["forward"] += timed(fwd, fwd)
    for k, v in samples.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
