"""u8 BGR input paths of batch-64 executors, measured on the same box with alternating repeats (frames / s, time per step):
  (i)   64 frames at 320 x 320 through forward_bgr_dev (the first kernel converts the bytes itself: the headline input)
  (ii)  64 frames of test.bmp at 640 x 424 through forward_bgr_dev (k_input_bgr4 + the fp32 graph)
  (iii) a mixed batch through forward_bgr_frames_dev, fused (the resizing first kernel): 1920x1080, 1280x720, 640x480, 640x424, 320x320
        in turn, some with padded pitches, some in one shared allocation at odd offsets
  (iv)  batch (iii) with FFGPU_NO_U8_FRONT=1 (k_input_frames + the fp32 graph)
(iii) and (iv) take their frames from three descriptor sets in turn (same pictures, different buffers), so every call rewrites the executor's
frame table -- what a decoder handing over fresh buffers costs.  Two regimes: "chains", bench.py's setup (4 FFGPU_CONCURRENT executors on 4
streams taking the batches in turn), and "single" (one executor, one stream).
usage: python tools/bgr_frames_bench.py [--steps 400] [--warmup 40] [--repeats 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ffcnn_amd import capi as F
    B = a.batch
    bmp, bw, bh = F.load_bmp(os.path.join(ROOT, "data", "test.bmp"))
    rng = np.random.default_rng(5)
    src = np.frombuffer(bmp, np.uint8).reshape(bh, -1)[:, :3 * bw].reshape(bh, bw, 3)
    u320 = torch.from_numpy(rng.integers(0, 256, (B, 320, 960), dtype=np.uint8)).cuda()
    ubmp = torch.from_numpy(np.ascontiguousarray(np.repeat(np.frombuffer(bmp, np.uint8).reshape(1, bh, -1), B, 0))).cuda()
    sizes = [(1920, 1080), (1280, 720), (640, 480), (640, 424), (320, 320)]
    keep, sets = [], []
    for _ in range(3):                                                  # three buffer sets of the same pictures
        desc, shared_rows, lay = [], [], []
        for f in range(B):
            w, h = sizes[f % len(sizes)]
            pitch = 3 * w + (64 if f % 3 == 1 else 0)                   # some padded pitches
            rows = np.zeros((h, pitch), np.uint8)
            rows[:, :3 * w] = np.resize(src, (h, w, 3)).reshape(h, 3 * w)
            if f % 4 == 0:                                              # some frames inside one shared allocation, at odd offsets
                lay.append((f, sum(r.size + 1 for r in shared_rows) + 1, w, h, pitch))
                shared_rows.append(rows)
                desc.append(None)
            else:
                t = torch.from_numpy(rows).cuda()
                keep.append(t)
                desc.append((t.data_ptr(), w, h, pitch))
        big = torch.from_numpy(np.concatenate([np.concatenate([[0], r.reshape(-1)]).astype(np.uint8) for r in shared_rows] + [np.zeros(8, np.uint8)])).cuda()
        keep.append(big)
        for f, o, w, h, pitch in lay:
            desc[f] = (big.data_ptr() + o, w, h, pitch)
        sets.append(desc)
    mean, norm = (0.0, 0.0, 0.0), (1 / 255.0,) * 3
    arrs = [(F.BgrFrame * B)(*[F.BgrFrame(*F.bgr_frame_desc(d)) for d in desc]) for desc in sets]      # (built once: the loop times the library)
    cm, cn = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*norm)
    L = F.lib()
    net = F.Net()
    regimes = {"chains": (4, F.FFGPU.CONCURRENT), "single": (1, 0)}
    out = {"batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    modes = ["i", "ii", "iii", "iv"]
    for rname, (E, flags) in regimes.items():
        execs = [net.executor(B, flags) for _ in range(E)]
        streams = [torch.cuda.Stream() for _ in range(E)]

        def run(mode):
            if mode == "iv":
                os.environ["FFGPU_NO_U8_FRONT"] = "1"
            else:
                os.environ.pop("FFGPU_NO_U8_FRONT", None)

            def one(k):
                ex, st = execs[k % E], streams[k % E].cuda_stream
                if mode == "i":
                    ex.forward_bgr_dev(u320.data_ptr(), 320, 320, mean, norm, stream=st)
                elif mode == "ii":
                    ex.forward_bgr_dev(ubmp.data_ptr(), bw, bh, mean, norm, stream=st)
                else:
                    if L.ffgpu_exec_forward_bgr_frames_dev(ex.h, arrs[k % 3], B, cm, cn, st) < 0:
                        raise RuntimeError(F.last_error())
            for k in range(a.warmup):
                one(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.steps):
                one(k)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.steps

        res = {m: [] for m in modes}
        for r in range(a.repeats):
            for m in (modes if r % 2 == 0 else modes[::-1]):
                res[m].append(run(m))
        os.environ.pop("FFGPU_NO_U8_FRONT", None)
        o = {"executors": E, "flags": flags, "graph_captures": [ex.graph_captures for ex in execs]}
        for m in modes:
            med = float(np.median(res[m]))
            o[m] = {"us_per_step": [round(v, 2) for v in res[m]], "median_us": round(med, 2), "frames_per_s": round(B / med * 1e6, 1)}
        o["iii_vs_i"] = round(o["i"]["median_us"] / o["iii"]["median_us"], 4)
        o["iii_vs_ii"] = round(o["ii"]["median_us"] / o["iii"]["median_us"], 4)
        o["iii_vs_iv"] = round(o["iv"]["median_us"] / o["iii"]["median_us"], 4)
        out[rname] = o
        for ex in execs:
            ex.close()
    net.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
