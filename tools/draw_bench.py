#!/usr/bin/env python3
"""Device time of the draw launches: HIP events on the forward's stream, batch 64, 20 warm-up + 100 timed launches, median, beside the
same executor's step times and k_nms time (ffgpu_exec_profile_steps) measured in the same process.  Prints one JSON object; with a path
argument it is written there too:  python tools/draw_bench.py [profiles/draw_bench.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402


def bgr_to_nv12(img):
    """BT.601 limited range, chroma = mean of each 2 x 2 block (even sizes)"""
    h, w = img.shape[:2]
    b, g, r = (img[..., k].astype(np.float64) for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    uv = np.stack([p.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)) for p in (u, v)], -1).reshape(h // 2, w)
    return np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(uv), 0, 255).astype(np.uint8)


B = 64
rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
img = np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))
st = torch.cuda.Stream()
out = {"batch": B, "warmup": 20, "timed": 100}


def timed(busy, fn):
    """median device time of fn's launches: `busy` (a forward, ~0.3 ms) is enqueued in front of every sample, so the host runs ahead of the
    device and the two events bracket fn's kernels alone, not the host's enqueue pace"""
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
    us = sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)
    return {"median_us": round(us[50], 2), "min_us": round(us[0], 2), "p90_us": round(us[90], 2)}


def host_paced(fn):
    """the same launches back to back with nothing in front: what a caller sees who rebuilds the tables in Python every step"""
    for _ in range(20):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for a, b in ev:
        a.record(st)
        fn()
        b.record(st)
    st.synchronize()
    us = sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)
    return {"median_us": round(us[50], 2)}


L = F.lib()
S = st.cuda_stream
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
net = F.Net()
with net.executor(B) as ex:
    # BGR: 64 copies of the 640 x 424 picture, each its own buffer; the tables are built once
    bgr = [torch.from_numpy(img).cuda() for _ in range(B)]
    tab = F.bgr_frame_table(bgr)
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, tab, B, mean, norm, S)
    assert fwd() == 0
    out["boxes_per_frame"] = len(ex.read_boxes(0))
    for T in (1, 2, 8):
        sty = F.draw_style(thickness=T)
        out["draw_bgr_entries_64x640x424_T%d" % T] = timed(fwd, lambda: L.ffgpu_exec_draw_bgr(ex.h, 0, tab, B, sty, S))
    out["host_paced_python_helper_draw_bgr"] = host_paced(lambda: ex.draw_bgr(bgr, F.DRAW_ENTRIES, stream=S))
    sty1 = F.draw_style()
    out["host_paced_prebuilt_tables_draw_bgr"] = host_paced(lambda: L.ffgpu_exec_draw_bgr(ex.h, 0, tab, B, sty1, S))
    # the operator with a few dozen outlines per frame: 32 seeded boxes inside each frame, 80 colours
    rng = np.random.default_rng(1)
    recs = np.zeros(B, F.DETS_DTYPE)
    for t in range(B):
        x1, y1 = rng.uniform(0, 500, 32), rng.uniform(0, 300, 32)
        recs[t]["count"] = recs[t]["nfull"] = 32
        recs[t]["box"]["type"][:32] = rng.integers(0, 80, 32)
        recs[t]["box"]["x1"][:32], recs[t]["box"]["y1"][:32] = x1, y1
        recs[t]["box"]["x2"][:32], recs[t]["box"]["y2"][:32] = x1 + rng.uniform(20, 139, 32), y1 + rng.uniform(20, 123, 32)
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    pal = F.draw_style(palette=rng.integers(0, 256, (80, 3)), thickness=2)
    out["draw_bgr_operator_64x640x424_32boxes_T2"] = timed(fwd, lambda: L.ffgpu_draw_boxes_bgr_dev(d_recs.data_ptr(), None, 0, None, tab, B, pal, S))
    # NV12
    Y, UV = bgr_to_nv12(img)
    nv = [(torch.from_numpy(Y).cuda(), torch.from_numpy(UV).cuda()) for _ in range(B)]
    ntab = F.nv12_frame_table(nv)
    nfwd = lambda: L.ffgpu_exec_forward_nv12_frames_dev(ex.h, ntab, B, mean, norm, S)
    assert nfwd() == 0
    out["boxes_per_frame_nv12"] = len(ex.read_boxes(0))
    for T in (1, 2, 8):
        sty = F.draw_style((81, 90, 240), thickness=T)
        out["draw_nv12_entries_64x640x424_T%d" % T] = timed(nfwd, lambda: L.ffgpu_exec_draw_nv12(ex.h, 0, ntab, B, sty, S))
    out["draw_nv12_operator_64x640x424_32boxes_T2"] = timed(nfwd, lambda: L.ffgpu_draw_boxes_nv12_dev(d_recs.data_ptr(), None, 0, None, ntab, B, pal, S))
    # merged: 4 pictures of 1280 x 848 (2 x 2 copies), 16 tiles each
    plan = None
    for tw, th, ox, oy in ((400, 280, 100, 80), (416, 288, 128, 96), (384, 256, 80, 56), (320, 212, 0, 0)):
        p = F.tile_plan(1280, 848, tw, th, ox, oy, 1)
        if len(p) == 16:
            plan = p
            out["tile_plan"] = [tw, th, ox, oy]
            break
    assert plan is not None
    pics = [torch.from_numpy(np.ascontiguousarray(np.tile(img, (2, 2, 1)))).cuda() for _ in range(4)]
    frames, tiles = [], []
    for g, pic in enumerate(pics):
        f, t = F.tiles_of(pic, plan, g)
        frames += f
        tiles += t
    ttab, ptab, tl = F.bgr_frame_table(frames), F.bgr_frame_table(pics), F.tile_table(tiles)
    tfwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ttab, B, mean, norm, S)

    def fwd_merge():
        tfwd()
        L.ffgpu_exec_merge_tiles(ex.h, tl, B, 4, S)
    tfwd()
    ex.merge_tiles(tiles, 4, stream=S)                            # (the helper: it sizes read_merged_boxes' buffer)
    out["merged_boxes_per_picture"] = [len(ex.read_merged_boxes(g)) for g in range(4)]
    for T in (1, 2):
        sty = F.draw_style(thickness=T)
        out["draw_bgr_merged_4x1280x848_T%d" % T] = timed(fwd_merge, lambda: L.ffgpu_exec_draw_bgr(ex.h, 1, ptab, 4, sty, S))
    out["merge_tiles_4x16"] = timed(tfwd, lambda: L.ffgpu_exec_merge_tiles(ex.h, tl, B, 4, S))
    # the same executor's step times (eager, events between the launches), the picture's own fp32 input
    net.set_input_image(rows, w, h)
    x = torch.from_numpy(np.stack([net.input.copy()] * B)).cuda()
    torch.cuda.synchronize()
    steps = ex.profile_steps(x.data_ptr())
    out["forward_sum_of_steps_us"] = round(float(sum(u for _, u in steps)), 1)
    out["k_nms_us"] = round(float(steps[-1][1]), 2)
    out["nsteps"] = len(steps)
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
