#!/usr/bin/env python3
"""Device time of the heat map launches: HIP events on one stream, 64 frames of 1920 x 1080 (u8 BGR and NV12), the operator forms,
20 warm-up + 100 timed calls, a 256 MB memset in front of every sample; median, min and p90.  The blend on (a) an empty grid -- its floor: the levels
of every block's cells and nothing else --, (b) a grid with a tenth of its cells hot, floor 1, and (c) every cell hot, floor 0: every byte inside the
extent read and written; NEAREST and SMOOTH; cells of 8, 16 and 32 pixels (a grid has 128 cells a side at most, so cells of 8 cover 1024 x 1024 of
the frame; 120 x 68 cells of 16 and 60 x 34 of 32 cover all of it).  The accumulate launch on its own: 8 boxes per frame on a 120 x 68 grid, 64
streams of one record and one stream of 64 records.  In the same run, on the same frames, the yardstick whose code the heat maps do not touch:
ffgpu_redact_boxes_*_dev MOSAIC 16 with OUTSIDE, which also reads every pixel once and writes it once; every blend time is also given as a multiple
of it.  Next to each blend time its byte model per call, computed here from the grid: the bytes of every 64 x 64 block (inside the extent) that has a
cell at or above the floor are read, the bytes of the pixels that are drawn are written, and the cells a block can reach are read.
Prints one JSON object; with a path argument it is written there too:  python tools/heat_bench.py [profiles/heat_bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ffcnn_amd import capi as F  # noqa: E402
from heat import heatref  # noqa: E402  (the byte model follows the contract's restatement)

B, W, H, CELL, NBOX, PEAK, BLOCK = 64, 1920, 1080, 16, 8, 8e12, 64
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"frames": B, "size": [W, H], "warmup": 20, "timed": 100, "peak_bytes_per_s": PEAK, "yardstick": "redact MOSAIC %d OUTSIDE" % CELL}


def timed(busy, fn):
    """median device time of fn's launches: `busy` is enqueued in front of every sample, so the host runs ahead of the device and the two events
    bracket fn's kernels alone, not the host's enqueue pace"""
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
    us = sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)
    return {"median_us": round(us[50], 2), "min_us": round(us[0], 2), "p90_us": round(us[90], 2)}


def byte_model(cells, bs):
    """{ nv12: (bytes read, bytes written) } of one call on B frames by the kernel's structure"""
    hdr = np.array([0, int(cells.max()), 0, 0], np.uint32)
    Lv = heatref.levels(hdr, cells, bs)
    w, h = min(W, bs.gw << bs.cell_log2), min(H, bs.gh << bs.cell_log2)
    lev = heatref.pixel_levels(Lv, bs, w, h)
    drawn = heatref.alphas(lev, bs) > 0
    thr, k = max(bs.floor, 1), bs.cell_log2
    half, more = ((1 << k) >> 1, 1) if bs.smooth else (0, 0)
    rd, wr = {False: 0, True: 0}, {False: 0, True: 0}
    for by in range(0, h, BLOCK):
        for bx in range(0, w, BLOCK):
            bw, bh = min(BLOCK, w - bx), min(BLOCK, h - by)
            i0, i1 = max((bx - half) >> k, 0), min(((bx + bw - 1 - half) >> k) + more, bs.gw - 1)
            j0, j1 = max((by - half) >> k, 0), min(((by + bh - 1 - half) >> k) + more, bs.gh - 1)
            for nv12 in (False, True):
                rd[nv12] += 4 * (i1 - i0 + 1) * (j1 - j0 + 1)
            if (Lv[j0:j1 + 1, i0:i1 + 1] >= thr).any():
                d = drawn[by:by + bh, bx:bx + bw]
                rd[True] += bw * bh + 2 * ((bw + 1) // 2) * ((bh + 1) // 2)
                wr[True] += int(d.sum()) + 2 * int(d[::2, ::2].sum())
                rd[False] += 3 * bw * bh
                wr[False] += 3 * int(d.sum())
    return {nv12: (B * rd[nv12], B * wr[nv12]) for nv12 in (False, True)}


rng = np.random.default_rng(529)
boxes = []                                                                         # 8 boxes of about 200 x 200 per frame, anywhere inside (tools/redact_bench.py's)
for t in range(B):
    x1, y1 = rng.integers(0, W - 230, NBOX), rng.integers(0, H - 230, NBOX)
    boxes.append([(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in zip(x1, y1, rng.integers(170, 230, NBOX), rng.integers(170, 230, NBOX))])
recs = np.zeros(B, F.DETS_DTYPE)
for t in range(B):
    recs[t]["count"] = recs[t]["nfull"] = NBOX
    recs[t]["box"]["score"][:NBOX] = 0.5
    for k, (a, b, c, d) in enumerate(boxes[t]):
        recs[t]["box"][k]["x1"], recs[t]["box"][k]["y1"], recs[t]["box"][k]["x2"], recs[t]["box"][k]["y2"] = a + 0.5, b + 0.5, c + 0.5, d + 0.5
d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()

with torch.cuda.stream(st):
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    bgr = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    nv = [(torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (H // 2, W), dtype=torch.uint8, device="cuda")) for _ in range(B)]
st.synchronize()
tabs = {False: F.bgr_frame_table(bgr), True: F.nv12_frame_table(nv)}
blend = {False: L.ffgpu_heat_blend_bgr_dev, True: L.ffgpu_heat_blend_nv12_dev}
redact = {False: L.ffgpu_redact_boxes_bgr_dev, True: L.ffgpu_redact_boxes_nv12_dev}
zeros = (F.C.c_int * B)(*([0] * B))


def busy():
    with torch.cuda.stream(st):
        flush.zero_()


def grid_state(gw, gh, kind):
    """one stream's state: (a) empty, (b) a tenth of the cells hot, (c) every cell hot"""
    stt = heatref.State(1, gw, gh)
    if kind == "b":
        stt.cells[0] = np.where(rng.random((gh, gw)) < 0.1, rng.integers(100, 1000, (gh, gw)), 0)
    elif kind == "c":
        stt.cells[0] = rng.integers(100, 1000, (gh, gw))
    stt.hdr[0, 1] = stt.cells.max()
    return stt


yard = {}
for nv12 in (False, True):
    spec = F.redact_spec(F.REDACT_MOSAIC, CELL, outside=True)
    yard[nv12] = timed(busy, lambda: redact[nv12](d_recs.data_ptr(), None, 0, None, tabs[nv12], B, spec, S))
    out[("nv12_" if nv12 else "bgr_") + "yardstick_mosaic16_outside"] = yard[nv12]

for k, gw, gh in ((3, 128, 128), (4, 120, 68), (5, 60, 34)):
    for kind, floor in (("a", 1), ("b", 1), ("c", 0)):
        stt = grid_state(gw, gh, kind)
        d_state = torch.from_numpy(stt.raw.reshape(-1).copy()).cuda()
        for smooth in (False, True):
            bsr = heatref.BlendSpec(gw, gh, k, 1000, floor, 128, smooth)
            bs = F.heat_blend_spec(gw, gh, k, 1000, floor, 128, smooth)
            model = byte_model(stt.cells[0], bsr)
            for nv12 in (False, True):
                t = timed(busy, lambda: blend[nv12](d_state.data_ptr(), 1, zeros, tabs[nv12], B, bs, S))
                rd, wr = model[nv12]
                t["model_bytes_read"], t["model_bytes_written"] = rd, wr
                t["model_GB_per_s"] = round((rd + wr) / (t["median_us"] * 1e-6) / 1e9, 1)
                t["fraction_of_peak"] = round((rd + wr) / (t["median_us"] * 1e-6) / PEAK, 4)
                t["times_yardstick"] = round(t["median_us"] / yard[nv12]["median_us"], 2)
                out["%s%s_cell%d_%s" % ("nv12_" if nv12 else "bgr_", kind, 1 << k, "smooth" if smooth else "nearest")] = t

# the accumulate launch on its own: 8 boxes per frame, a 120 x 68 grid of cells of 16
for name, nstreams, streams in (("accumulate_64_streams_x_1_record", B, list(range(B))), ("accumulate_1_stream_x_64_records", 1, [0] * B)):
    for mode, spread in ((F.HEAT_ANCHOR, 2), (F.HEAT_BOX, 0)):
        d_state = torch.zeros(F.heat_state_bytes(nstreams, 120, 68), dtype=torch.uint8, device="cuda")
        d_rows = torch.zeros(4 * F.HEAT_ROW * B, dtype=torch.uint8, device="cuda")
        hs = F.heat_spec(120, 68, 4, mode, 1, spread, 64, 6)
        arr = (F.C.c_int * B)(*streams)
        t = timed(busy, lambda: L.ffgpu_heat_boxes_dev(d_recs.data_ptr(), None, 0, None, arr, B, hs, d_state.data_ptr(), nstreams, d_rows.data_ptr(), S))
        t["state_bytes"] = F.heat_state_bytes(nstreams, 120, 68)
        out["%s_%s" % (name, "box" if mode else "anchor_spread2")] = t
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
