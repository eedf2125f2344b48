#!/usr/bin/env python3
"""Device time of the outlines: ffgpu_outline_scene_dev and ffgpu_draw_segments_bgr_dev / _nv12_dev on 64 frames of 1920 x 1080 with a
scene of 8 octagons and 8 lines (shafts dashed, forward ticks), 32 anchor markers and thickness 2 (items_stride 144), beside ffgpu_draw_boxes_bgr_dev
with 32 boxes per frame on the same frames in the same run (the yardstick: the existing post-pass of the same idiom, thickness 2).  The pixels each
writes per frame are counted once, from the frames, so the two can be compared per written pixel.  A forward of data/test.bmp is enqueued in front of
every sample so that the events bracket device work and not the host's pace (tools/captions_bench.py's sampling).  HIP events on one stream, one
process, the measurements alternating over `repeats` rounds of 20 warm-up + 100 timed launches.  Prints one JSON object; with a path argument it is
written there too:  python tools/outlines_bench.py [profiles/outlines_bench.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, REPEATS, W, H, STRIDE, LIST, CAP, MARKERS = 64, 3, 1920, 1080, 144, 32, 32, 32
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"batch": B, "frame": [W, H], "warmup": 20, "timed": 100, "repeats": REPEATS, "items_stride": STRIDE, "thickness": 2, "zones": 8, "zone_verts": 8, "lines": 8,
       "markers": MARKERS}


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


def scene(rng):
    """8 octagons of radius 120..260 and 8 lines across the frame"""
    zones = []
    for z in range(8):
        cx, cy, r = rng.uniform(300, W - 300), rng.uniform(300, H - 300), rng.uniform(120, 260)
        zones.append(([(cx + r * np.cos(2 * np.pi * k / 8), cy + r * np.sin(2 * np.pi * k / 8)) for k in range(8)], 1))
    lines = [((rng.uniform(0, W / 4), rng.uniform(0, H)), (rng.uniform(3 * W / 4, W), rng.uniform(0, H))) for _ in range(8)]
    return F.scene(zones, lines)


def records(rng, nboxes):
    recs, flat = np.zeros(B, F.DETS_DTYPE), np.zeros(B * LIST, F.BOX_DTYPE)
    recs["nfull"] = recs["count"] = nboxes
    for t in range(B):
        b = flat[t * LIST:t * LIST + nboxes]
        b["type"], b["score"] = rng.integers(0, 80, nboxes), rng.uniform(0.3, 1.0, nboxes)
        b["x1"], b["y1"] = rng.uniform(0, W - 300, nboxes), rng.uniform(20, H - 300, nboxes)
        b["x2"], b["y2"] = b["x1"] + rng.uniform(60, 300, nboxes), b["y1"] + rng.uniform(60, 300, nboxes)
    return recs, flat


rng = np.random.default_rng(6300)
rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
pic = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
ftab = F.bgr_frame_table([(pic.data_ptr(), w, h, rows.shape[1])] * B)
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
bgr = torch.zeros(B * H * W * 3, dtype=torch.uint8, device="cuda")
nv12 = torch.zeros(B * H * W * 3 // 2, dtype=torch.uint8, device="cuda")
tb = F.bgr_frame_table([(bgr.data_ptr() + t * H * W * 3, W, H) for t in range(B)])
tn = F.nv12_frame_table([(nv12.data_ptr() + t * (H * W * 3 // 2), 0, W, H) for t in range(B)])
# one video stream per frame: its scene, a state whose MARKERS slots were seen in the last frame, an event row with two loitered zones
scenes = dev(np.frombuffer(F.scenes_bytes([scene(rng) for _ in range(B)]), np.uint8))
state = np.zeros((B, F.ZONES_STATE_HEADER + 64 * CAP), np.uint8)
for t in range(B):
    state[t, :4] = np.frombuffer(np.uint32(5).tobytes(), np.uint8)
    sl = np.zeros(CAP, F.ZONE_SLOT_DTYPE)
    sl["id"][:MARKERS], sl["last"][:MARKERS] = np.arange(1, MARKERS + 1), 4
    sl["px"][:MARKERS], sl["py"][:MARKERS] = rng.uniform(50, W - 50, MARKERS), rng.uniform(50, H - 50, MARKERS)
    state[t, F.ZONES_STATE_HEADER:] = sl.view(np.uint8)
d_state = dev(state)
events = np.zeros((B, F.ZONES_ROW + 2 * LIST), "<i4")
events[:, [19, 31]] = 1
d_events = dev(events)
streams = (C.c_int * B)(*range(B))
items = torch.zeros(B * STRIDE * 32, dtype=torch.uint8, device="cuda")
pal = [(37 * k % 256 or 1, 91 * k % 256 or 1, 53 * k % 256 or 1) for k in range(1, 21)]
spec = F.outline_spec(True, True, True, True, True, thickness=2, line_dash=3, marker=6, alarm=(1, 1, 255), palette=pal)
style = F.draw_style(palette=pal, thickness=2)
recs, flat = (dev(a) for a in records(rng, LIST))
net = F.Net()
with net.executor(B) as ex:
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)                                                       # noqa: E731
    it = items.data_ptr()
    calls = {
        "outline_scene": lambda: L.ffgpu_outline_scene_dev(scenes.data_ptr(), d_state.data_ptr(), B, CAP, d_events.data_ptr(), F.ZONES_ROW + 2 * LIST, streams, B, spec, it,
                                                           STRIDE, S),
        "draw_segments_bgr": lambda: L.ffgpu_draw_segments_bgr_dev(it, STRIDE, tb, B, S),
        "draw_segments_nv12": lambda: L.ffgpu_draw_segments_nv12_dev(it, STRIDE, tn, B, S),
        "draw_boxes_bgr_32": lambda: L.ffgpu_draw_boxes_bgr_dev(recs.data_ptr(), flat.data_ptr(), LIST, None, tb, B, style, S),
    }
    # what each writes, counted from the frames: the segments first, the boxes into cleared frames
    assert fwd() == 0 and calls["outline_scene"]() == 0 and calls["draw_segments_bgr"]() == 0 and calls["draw_segments_nv12"]() == 0, F.last_error()
    st.synchronize()
    got = items.cpu().numpy().view(F.SEG_ITEM_DTYPE).reshape(B, STRIDE)
    assert ((got["thickness"] > 0).sum(axis=1) == 64 + 16 + 2 * MARKERS).all() and nv12.any()
    out["items_per_frame"] = int((got["thickness"] > 0).sum()) // B
    out["segment_pixels_per_frame"] = int((bgr.view(B, H, W, 3) != 0).any(dim=3).sum().item()) // B
    bgr.zero_()
    assert calls["draw_boxes_bgr_32"]() == 0
    st.synchronize()
    out["box_pixels_per_frame"] = int((bgr.view(B, H, W, 3) != 0).any(dim=3).sum().item()) // B
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
    out["ns_per_pixel"] = {"draw_segments_bgr": round(1000.0 * out["draw_segments_bgr"]["median_us"] / (B * out["segment_pixels_per_frame"]), 3),
                           "draw_boxes_bgr_32": round(1000.0 * out["draw_boxes_bgr_32"]["median_us"] / (B * out["box_pixels_per_frame"]), 3)}
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
