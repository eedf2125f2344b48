#!/usr/bin/env python3
"""Device time of the captions: ffgpu_caption_boxes_dev and ffgpu_draw_text_bgr_dev / _nv12_dev on 64 frames of 1920 x 1080 with 8 and
with 32 boxes per frame ("name 93% #12" tags, opaque, scale 2, items_stride 32), beside ffgpu_draw_boxes_bgr_dev on the same records and frames in the
same run (the yardstick: the existing per-box post-pass of the same idiom, thickness 2).  Seeded synthetic records; a forward of data/test.bmp
enqueued in front of every sample so that the events bracket device work and not the host's pace (tools/zones_bench.py's sampling).  HIP events on
one stream, one process, the measurements alternating over `repeats` rounds of 20 warm-up + 100 timed launches.  Prints one JSON object; with a
path argument it is written there too:  python tools/captions_bench.py [profiles/captions_bench.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, REPEATS, W, H, STRIDE, LIST = 64, 3, 1920, 1080, 32, 32
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"batch": B, "frame": [W, H], "warmup": 20, "timed": 100, "repeats": REPEATS, "items_stride": STRIDE, "scale": 2}


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


def records(rng, nboxes):
    """B records whose lists hold nboxes boxes spread over the frame, classes 0..79, scores 0.3..1"""
    recs, flat = np.zeros(B, F.DETS_DTYPE), np.zeros(B * LIST, F.BOX_DTYPE)
    recs["nfull"] = recs["count"] = nboxes
    for t in range(B):
        b = flat[t * LIST:t * LIST + nboxes]
        b["type"], b["score"] = rng.integers(0, 80, nboxes), rng.uniform(0.3, 1.0, nboxes)
        b["x1"], b["y1"] = rng.uniform(0, W - 300, nboxes), rng.uniform(20, H - 300, nboxes)
        b["x2"], b["y2"] = b["x1"] + rng.uniform(60, 300, nboxes), b["y1"] + rng.uniform(60, 300, nboxes)
    return recs, flat


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


rng = np.random.default_rng(6000)
rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
pic = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
ftab = F.bgr_frame_table([(pic.data_ptr(), w, h, rows.shape[1])] * B)
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
bgr = torch.zeros(B * H * W * 3, dtype=torch.uint8, device="cuda")
nv12 = torch.zeros(B * H * W * 3 // 2, dtype=torch.uint8, device="cuda")
tb = F.bgr_frame_table([(bgr.data_ptr() + t * H * W * 3, W, H) for t in range(B)])
tn = F.nv12_frame_table([(nv12.data_ptr() + t * (H * W * 3 // 2), 0, W, H) for t in range(B)])
names = dev(F.names_bytes(["class %d" % k for k in range(80)]))
ids = dev(np.tile(np.arange(8 + LIST, dtype="<i4"), (B, 1)))
items = torch.zeros(B * STRIDE * 64, dtype=torch.uint8, device="cuda")
pal = [(37 * k % 256, 91 * k % 256, 53 * k % 256) for k in range(20)]
spec = F.caption_spec(True, True, True, True, 0.25, F.ZONES_IDS, 2, palette=pal, d_names=names.data_ptr(), nnames=80)
style = F.draw_style(palette=pal, thickness=2)
net = F.Net()
with net.executor(B) as ex:
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)                                                       # noqa: E731
    samples = {"forward": []}
    for nboxes in (8, 32):
        recs, flat = (dev(a) for a in records(rng, nboxes))
        r, f, it = recs.data_ptr(), flat.data_ptr(), items.data_ptr()
        calls = {
            "caption_boxes_%d" % nboxes: lambda: L.ffgpu_caption_boxes_dev(r, f, LIST, None, B, spec, ids.data_ptr(), it, STRIDE, S),
            "draw_text_bgr_%d" % nboxes: lambda: L.ffgpu_draw_text_bgr_dev(it, STRIDE, None, tb, B, S),
            "draw_text_nv12_%d" % nboxes: lambda: L.ffgpu_draw_text_nv12_dev(it, STRIDE, None, tn, B, S),
            "draw_boxes_bgr_%d" % nboxes: lambda: L.ffgpu_draw_boxes_bgr_dev(r, f, LIST, None, tb, B, style, S),
        }
        assert fwd() == 0 and all(c() == 0 for c in calls.values()), F.last_error()
        st.synchronize()
        got = items.cpu().numpy().view(F.TEXT_ITEM_DTYPE).reshape(B, STRIDE)
        assert ((got["len"] > 0).sum(axis=1) == nboxes).all() and bgr.any() and nv12.any()
        out["characters_per_frame_%d" % nboxes] = round(float(got["len"].sum()) / B, 1)
        for k in calls:
            samples[k] = []
        for _ in range(REPEATS):
            for k, c in calls.items():
                samples[k] += timed(fwd, c)
    for _ in range(REPEATS):
        samples["forward"] += timed(fwd, fwd)
    for k, v in samples.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
