#!/usr/bin/env python3
"""Device time of the motion blobs launch: HIP events on one stream, 64 video streams of 1920 x 1080 at cells of 8 (240 x 135 cells, one
workgroup of k_blobs per stream), 20 warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  Three scenes, written
into the states' cells: about twenty rectangular blobs, 10 % random active cells, and the serpentine (full rows joined at alternating ends: one
component with the longest path the grid has).  Each with and without the label plane.  In the same run and ALTERNATING with it sample by sample,
the yardstick: ffgpu_motion_update_bgr_dev on 64 frames of the same streams, the call the blobs launch follows; every blobs time is also given as a
multiple of it.  (The update rewrites the cells, so it runs on a state of its own.)
Prints one JSON object; with a path argument it is written there too:  python tools/blobs_bench.py [profiles/blobs_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, K = 64, 1920, 1080, 3
GW, GH = (W + 7) >> K, (H + 7) >> K
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"streams": B, "size": [W, H], "cells": [GW, GH], "warmup": 20, "timed": 100, "yardstick": "ffgpu_motion_update_bgr_dev, cells of 8, alternating with blobs"}


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


def scene(name, rng):
    m = np.zeros((GH, GW), bool)
    if name == "rectangles":
        for _ in range(20):
            x, y, w, h = rng.integers(0, GW - 24), rng.integers(0, GH - 16), rng.integers(4, 24), rng.integers(4, 16)
            m[y:y + h, x:x + w] = True
    elif name == "random_10pct":
        m = rng.random((GH, GW)) < 0.10
    else:
        m[::2], m[1::4, -1], m[3::4, 0] = True, True, True
    return m


with torch.cuda.stream(st):
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    bgr = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
st.synchronize()


def busy():
    with torch.cuda.stream(st):
        flush.zero_()


tab, streams = F.bgr_frame_table(bgr), (F.C.c_int * B)(*range(B))
nstate = F.motion_state_bytes(B, W, H, K)
ms, bs = F.motion_spec(W, H, K, 16, 4, 8, 8, 64, 30), F.blobs_spec(W, H, K, 8, warmup=30, min_cells=2)
d_ystate, d_rows = torch.zeros(nstate, dtype=torch.uint8, device="cuda"), torch.zeros(4 * F.MOTION_ROW * B, dtype=torch.uint8, device="cuda")
d_words, d_recs = torch.zeros(4 * F.BLOBS_WORDS * B, dtype=torch.uint8, device="cuda"), torch.zeros(B * F.DETS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
d_labels = torch.zeros(2 * B * ((GW * GH + 7) & ~7), dtype=torch.uint8, device="cuda")
rng = np.random.default_rng(536)
for name in ("rectangles", "random_10pct", "serpentine"):
    raw = np.zeros((B, nstate // B), np.uint8)
    hdr, cells = raw[:, :4].view("<u4"), raw[:, nstate // B - ((4 * GW * GH + 15) & ~15):][:, :4 * GW * GH].view("<u4").reshape(B, GH, GW)
    hdr[:] = 100
    for s in range(B):
        cells[s] = np.where(scene(name, rng), 40, 0)
    d_state = torch.from_numpy(raw.reshape(-1)).cuda()
    for lab in (True, False):
        t, y = timed(busy, [lambda: L.ffgpu_blobs_dev(streams, B, bs, d_state.data_ptr(), B, d_words.data_ptr(), d_recs.data_ptr(), d_labels.data_ptr() if lab else None, S),
                            lambda: L.ffgpu_motion_update_bgr_dev(tab, B, streams, ms, d_ystate.data_ptr(), B, d_rows.data_ptr(), S)])
        t["times_yardstick"] = round(t["median_us"] / y["median_us"], 3)
        words = d_words.cpu().numpy().view(np.int32).reshape(B, F.BLOBS_WORDS)
        t["stream_0"] = dict(zip(F.BLOBS_WORDS_HEADER, words[0].tolist()))
        out["blobs_%s%s" % (name, "" if lab else "_no_labels")], out["yardstick_%s%s" % (name, "" if lab else "_no_labels")] = t, y
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
