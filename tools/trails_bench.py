#!/usr/bin/env python3
"""Device time of the track trails: ffgpu_trails_boxes_dev on 64 video streams with one record each per call, capacity 128, points 32
and full lists (128 boxes per record, every one an owner that moves a few pixels per call, so every call appends 128 points per stream and the rings
are full and wrapping from the 32nd call on), the items written (16 regions of 32 into rows of 512) and not; ffgpu_draw_segments_bgr_dev on those
items into 64 frames of 1280 x 720; and beside them ffgpu_zones_boxes_dev on the same records, ids and streams with scenes of 8 octagons and 8 lines
and capacity 128 (the yardstick: the existing per-stream post-pass of the same shape).  The records cycle through 48 prepared positions.  A forward
of data/test.bmp is enqueued in front of every sample so that the events bracket device work and not the host's pace (tools/zones_bench.py's
sampling).  HIP events on one stream, one process, the measurements alternating over `repeats` rounds of 20 warm-up + 100 timed launches.  Prints
one JSON object; with a path argument it is written there too:  python tools/trails_bench.py [profiles/trails_bench.json]"""
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

B, REPEATS, W, H, CAP, POINTS, LIST, STRIDE, STEPS = 64, 3, 1280, 720, 128, 32, 128, 512, 48
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"streams": B, "records_per_call": B, "boxes_per_record": LIST, "capacity": CAP, "points": POINTS, "items_stride": STRIDE, "frame": [W, H], "warmup": 20,
       "timed": 100, "repeats": REPEATS}


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


rng = np.random.default_rng(5780)
# 128 objects per stream on a random walk of up to 6 pixels per call; the list is the objects in a fixed order, ids 1..128
pos = rng.uniform(40, [W - 40, H - 40], (B, LIST, 2))
recs = np.zeros(B, F.DETS_DTYPE)
recs["count"], recs["nfull"], recs["ncand"] = 128, LIST, LIST
ids = np.zeros((B, 8 + LIST), "<i4")
ids[:, 8:] = np.arange(1, LIST + 1)
flats = []
for k in range(STEPS):
    pos = np.clip(pos + rng.integers(-6, 7, pos.shape), 8, [W - 8, H - 8])
    fl = np.zeros((B, LIST), F.BOX_DTYPE)
    fl["type"], fl["score"] = np.arange(LIST) % 80, 0.9
    fl["x1"], fl["y1"], fl["x2"], fl["y2"] = pos[..., 0] - 12, pos[..., 1] - 20, pos[..., 0] + 12, pos[..., 1] + 20
    flats.append(dev(fl))
d_recs, d_ids = dev(recs), dev(ids)
octagon = lambda cx, cy, r: [(round(cx + r * math.cos(k * math.pi / 4)), round(cy + r * math.sin(k * math.pi / 4))) for k in range(8)]   # noqa: E731
scene = F.scene([(octagon(160 + 140 * z, H // 2, 120 + 40 * z), 2) for z in range(8)],
                [((-10, 80 + 70 * l), (W + 10, 80 + 70 * l)) if l % 2 else ((80 + 140 * l, -10), (80 + 140 * l, H + 10)) for l in range(8)])
F.scene_check([scene])
scenes = dev(np.frombuffer(F.scenes_bytes([scene] * B), np.uint8))
pal = [(37 * k % 256 or 1, 91 * k % 256 or 1, 53 * k % 256 or 1) for k in range(1, 21)]
tspec = F.trails_spec(CAP, max_missed=2, identity=F.ZONES_IDS, points=POINTS, thickness=2, taper=True, palette=pal)
zspec = F.zones_spec(CAP, max_missed=2, identity=F.ZONES_IDS, gate_zone=0xff)
t_state = torch.zeros(F.trails_state_bytes(B, CAP), dtype=torch.uint8, device="cuda")
z_state = torch.zeros(F.zones_state_bytes(B, CAP), dtype=torch.uint8, device="cuda")
t_rows = torch.zeros(4 * B * (F.TRAILS_ROW + 4 * LIST), dtype=torch.uint8, device="cuda")
z_events = torch.zeros(4 * B * (F.ZONES_ROW + 2 * LIST), dtype=torch.uint8, device="cuda")
items = torch.zeros(B * STRIDE * 32, dtype=torch.uint8, device="cuda")
bgr = torch.zeros(B * H * W * 3, dtype=torch.uint8, device="cuda")
tb = F.bgr_frame_table([(bgr.data_ptr() + t * H * W * 3, W, H, 3 * W) for t in range(B)])
streams = (C.c_int * B)(*range(B))
rows_, w_, h_ = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
pic = torch.from_numpy(np.ascontiguousarray(rows_)).cuda()
ftab = F.bgr_frame_table([(pic.data_ptr(), w_, h_, rows_.shape[1])] * B)
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
step = [0]


def lists():
    step[0] += 1
    return flats[step[0] % STEPS].data_ptr()


net = F.Net()
with net.executor(B) as ex:
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)                                                       # noqa: E731
    calls = {
        "trails": lambda: L.ffgpu_trails_boxes_dev(d_recs.data_ptr(), lists(), LIST, None, streams, B, tspec, t_state.data_ptr(), B, d_ids.data_ptr(), t_rows.data_ptr(),
                                                   items.data_ptr(), STRIDE, 0, STRIDE, S),
        "trails_rows_only": lambda: L.ffgpu_trails_boxes_dev(d_recs.data_ptr(), lists(), LIST, None, streams, B, tspec, t_state.data_ptr(), B, d_ids.data_ptr(),
                                                             t_rows.data_ptr(), None, 0, 0, 0, S),
        "zones": lambda: L.ffgpu_zones_boxes_dev(d_recs.data_ptr(), lists(), LIST, None, streams, B, zspec, scenes.data_ptr(), z_state.data_ptr(), B, d_ids.data_ptr(),
                                                 z_events.data_ptr(), None, None, S),
        "draw_segments_bgr": lambda: L.ffgpu_draw_segments_bgr_dev(items.data_ptr(), STRIDE, tb, B, S),
    }
    assert fwd() == 0, F.last_error()
    for _ in range(POINTS + 8):                                                       # the rings fill and wrap before anything is timed
        assert calls["trails"]() == 0 and calls["zones"]() == 0, F.last_error()
    assert calls["draw_segments_bgr"]() == 0, F.last_error()
    st.synchronize()
    rows = t_rows.cpu().numpy().view("<i4").reshape(B, F.TRAILS_ROW + 4 * LIST)
    assert (rows[:, 0] == LIST).all() and (rows[:, 1] == LIST).all() and (rows[:, 8] == CAP).all() and (rows[:, 11] == STRIDE // POINTS).all(), rows[:2, :16]
    assert (rows[:, F.TRAILS_ROW::4] == POINTS).all()
    got = items.cpu().numpy().view(F.SEG_ITEM_DTYPE).reshape(B, STRIDE)
    out["items_per_frame"] = int((got["thickness"] > 0).sum()) // B
    out["segment_pixels_per_frame"] = int((bgr.view(B, H, W, 3) != 0).any(dim=3).sum().item()) // B
    ev = z_events.cpu().numpy().view("<i4").reshape(B, F.ZONES_ROW + 2 * LIST)
    assert (ev[:, 0] == LIST).all() and (ev[:, 1] == LIST).all()
    samples = {k: [] for k in calls}
    samples["forward"] = []
    for _ in range(REPEATS):
        for k, c in calls.items():
            samples[k] += timed(fwd, c)
    for _ in range(REPEATS):
        samples["forward"] += timed(fwd, fwd)
    for k, v in samples.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
    out["ratio_trails_over_zones"] = round(out["trails"]["median_us"] / out["zones"]["median_us"], 3)
    out["ratio_trails_rows_only_over_zones"] = round(out["trails_rows_only"]["median_us"] / out["zones"]["median_us"], 3)
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
