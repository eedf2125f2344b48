#!/usr/bin/env python3
"""Device time of the preview launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12) scaled in one call, 20
warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  Each format into 64 panes of 480 x 270 on surfaces of
their own and into one 1920 x 1080 wall of 8 x 8 panes (ffgpu_preview_grid, no gap), each with aligned pitches (frames at 256-byte addresses, the
pitch the row's bytes) and with unaligned ones (frames at odd addresses -- NV12: the Y planes --, pitches of the row's bytes + 1, NV12's U V pitch
+ 2).  With its algorithmic bytes -- every source byte read once, every pane byte written once -- as bytes/s and as a fraction of 8 TB/s.  The
yardstick for a streaming frame reader of this tree is the motion update: run tools/motion_bench.py on the same box in the same sitting.
Prints one JSON object; with a path argument it is written there too:  python tools/preview_bench.py [profiles/preview_bench.json]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, PW, PH, PEAK = 64, 1920, 1080, 480, 270, 8e12
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"frames": B, "size": [W, H], "warmup": 20, "timed": 100, "peak_bytes_per_s": PEAK, "tile": list(F.preview_tile())}


def summary(us):
    us = sorted(us)
    return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "p90_us": round(us[(9 * len(us)) // 10], 2)}


def timed(busy, fn):
    """median device time of fn's launches: `busy` is enqueued in front of every sample, so the host runs ahead of the device and the two events
    bracket the function's kernels alone, not the host's enqueue pace"""
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
    return summary([a.elapsed_time(b) * 1000.0 for a, b in ev])


def planes(n, w, h, nv12, unaligned):
    """n frames of w x h in one buffer of random bytes: (the buffer, the frames as the wrappers take them)"""
    off = 1 if unaligned else 0
    if not nv12:
        pitch = 3 * w + off
        one = (pitch * h + 255 + 256) & ~255
        buf = torch.randint(0, 256, (n * one,), dtype=torch.uint8, device="cuda")
        return buf, [(buf.data_ptr() + k * one + off, w, h, pitch) for k in range(n)]
    py, puv = w + off, 2 * ((w + 1) // 2) + 2 * off
    ny = (py * h + 255 + 256) & ~255
    one = ny + ((puv * ((h + 1) // 2) + 255) & ~255)
    buf = torch.randint(0, 256, (n * one,), dtype=torch.uint8, device="cuda")
    return buf, [(buf.data_ptr() + k * one + off, buf.data_ptr() + k * one + ny, w, h, py, puv) for k in range(n)]


with torch.cuda.stream(st):
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")


def busy():
    with torch.cuda.stream(st):
        flush.zero_()


spec = F.preview_spec(F.PREVIEW_STRETCH)
for nv12 in (False, True):
    fn = L.ffgpu_preview_nv12_dev if nv12 else L.ffgpu_preview_bgr_dev
    table = F.nv12_frame_table if nv12 else F.bgr_frame_table
    bpp = 1.5 if nv12 else 3
    for unaligned in (False, True):
        with torch.cuda.stream(st):
            src_buf, srcs = planes(B, W, H, nv12, unaligned)
            pane_buf, small = planes(B, PW, PH, nv12, unaligned)
            wall_buf, wall = planes(1, W, H, nv12, unaligned)
        st.synchronize()
        whole = (F.PreviewPane * B)()
        grid = F.preview_grid(B, 8, W, H, 0, nv12)
        cells = (F.PreviewPane * B)(*grid)
        ts, td, tw = table(srcs), table(small), table(wall * B)
        for name, dsts, panes, written in (("panes_480x270", td, whole, B * PW * PH * bpp), ("wall_8x8", tw, cells, B * grid[0].dw * grid[0].dh * bpp)):
            t = timed(busy, lambda: fn(ts, dsts, panes, B, spec, S))
            nbytes = int(B * W * H * bpp + written)
            t["algorithmic_bytes"] = nbytes
            t["GB_per_s"] = round(nbytes / (t["median_us"] * 1e-6) / 1e9, 1)
            t["fraction_of_peak"] = round(nbytes / (t["median_us"] * 1e-6) / PEAK, 4)
            out["%s_%s_%s" % ("nv12" if nv12 else "bgr", name, "unaligned" if unaligned else "aligned")] = t
        del src_buf, pane_buf, wall_buf
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
