#!/usr/bin/env python3
"""Device time of the warp launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12) warped in one call, 20
warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  Each format through the identity mesh, through orient 1
(a rotation by 90 degrees into 1080 x 1920) and through a Brown lens mesh with k1 = -0.3, BILINEAR and FILL, cells of 16, a mesh of its own per
frame; each with aligned pitches (frames at 256-byte addresses, the pitch the row's bytes) and with unaligned ones (frames at odd addresses -- NV12:
the Y planes --, pitches of the row's bytes + 1, NV12's U V pitch + 2).  With its algorithmic bytes -- the source once plus the destination once --
as bytes/s and as a fraction of 8 TB/s.  The yardsticks for a frame reader of this tree are the motion update and the preview: run
tools/motion_bench.py and tools/preview_bench.py on the same box in the same sitting.
Prints one JSON object; with a path argument it is written there too:  python tools/warp_bench.py [profiles/warp_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, CELL, PEAK = 64, 1920, 1080, 16, 8e12
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"frames": B, "size": [W, H], "cell": CELL, "warmup": 20, "timed": 100, "peak_bytes_per_s": PEAK, "tile": list(F.warp_tile())}


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


LENS = F.warp_lens(F.WARP_LENS_BROWN, (1000.0, 1000.0, 959.5, 539.5), (1000.0, 1000.0, 959.5, 539.5), (-0.3, 0, 0, 0))
MESHES = {"identity": ((W, H), F.warp_mesh_orient(W, H, 0, CELL)[1]), "orient90": F.warp_mesh_orient(W, H, 1, CELL), "lens_k1_-0.3": ((W, H), F.warp_mesh_lens(W, H, CELL, LENS))}
spec = F.warp_spec(F.WARP_BILINEAR, F.WARP_FILL, (16, 128, 128))
for nv12 in (False, True):
    fn = L.ffgpu_warp_nv12_dev if nv12 else L.ffgpu_warp_bgr_dev
    table = F.nv12_frame_table if nv12 else F.bgr_frame_table
    bpp = 1.5 if nv12 else 3
    for unaligned in (False, True):
        for name, ((dw, dh), xy) in MESHES.items():
            with torch.cuda.stream(st):
                src_buf, srcs = planes(B, W, H, nv12, unaligned)
                dst_buf, dsts = planes(B, dw, dh, nv12, unaligned)
                d_xy = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(xy, (B,) + xy.shape))).cuda()       # a mesh per frame
            st.synchronize()
            assert d_xy.data_ptr() % 8 == 0 and xy.nbytes % 8 == 0
            ms = (F.WarpMesh * B)(*[F.warp_mesh(d_xy.data_ptr() + k * xy.nbytes, dw, dh, CELL) for k in range(B)])
            ts, td = table(srcs), table(dsts)
            t = timed(busy, lambda: fn(ts, td, ms, B, spec, S))
            nbytes = int(2 * B * W * H * bpp)
            t["algorithmic_bytes"] = nbytes
            t["GB_per_s"] = round(nbytes / (t["median_us"] * 1e-6) / 1e9, 1)
            t["fraction_of_peak"] = round(nbytes / (t["median_us"] * 1e-6) / PEAK, 4)
            out["%s_%s_%s" % ("nv12" if nv12 else "bgr", name, "unaligned" if unaligned else "aligned")] = t
            print("%-36s %9.1f us  %8.1f GB/s  %5.1f %%" % ("%s_%s_%s" % ("nv12" if nv12 else "bgr", name, "unaligned" if unaligned else "aligned"), t["median_us"], t["GB_per_s"],
                                                          100 * t["fraction_of_peak"]), file=sys.stderr, flush=True)
            del src_buf, dst_buf, d_xy
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
