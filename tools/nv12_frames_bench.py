"""NV12 input of batch-64 executors against the u8 BGR routes, measured on the same box with alternating repeats (frames / s, time per step):
  (a) FFGPU_NV12_FRONT=1: the mixed batch of tools/bgr_frames_bench.py (iii) -- 1920x1080, 1280x720, 640x480, 640x424, 320x320 in turn, some padded pitches,
      some frames in one shared allocation at odd offsets -- handed over as NV12 through forward_nv12_frames_dev, fused (the NV12 form
      of the first kernel)
  (b) the same, FFGPU_NO_U8_FRONT=1 (k_input_nv12_frames + the fp32 graph)
  (c) the same pictures converted to BGR on the host, through forward_bgr_frames_dev, fused: the route a convert-first pipeline ends in, its
      conversion pass not counted
  (d) 64 frames at 320 x 320 as BGR through forward_bgr_dev: the headline input, the anchor
(a) - (c) take their frames from three descriptor sets in turn (same pictures, different buffers), so every call rewrites the executor's
frame table -- what a decoder handing over fresh surfaces costs.  Two regimes: "chains", bench.py's setup (4 FFGPU_CONCURRENT executors on
4 streams taking the batches in turn), and "single" (one executor, one stream).
usage: python tools/nv12_frames_bench.py [--steps 400] [--warmup 40] [--repeats 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAT601 = (16, 298, 409, 100, 208, 516)
# (bgr_to_nv12 / nv12_to_bgr below only make this tool's pictures; the normative model of the conversion is the one in
#  tests/nv12_frames/test_gpu_fuzz_input.py, which the kernels are tested against)


def bgr_to_nv12(img):
    """BT.601 limited range, chroma = mean of each 2 x 2 block (even sizes)"""
    h, w = img.shape[:2]
    b, g, r = (img[..., k].astype(np.float64) for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    uv = np.stack([u.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)), v.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))], -1).reshape(h // 2, w)
    return np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(uv), 0, 255).astype(np.uint8)


def nv12_to_bgr(Y, UV):
    """include/ffcnn_hip.h's integer formula, FFGPU_YUV_BT601_LIMITED"""
    yoff, cy, crv, cgu, cgv, cbu = MAT601
    h, w = Y.shape
    yy, xx = np.mgrid[0:h, 0:w]
    c = Y.astype(np.int32) - yoff
    d = UV[yy >> 1, 2 * (xx >> 1)].astype(np.int32) - 128
    e = UV[yy >> 1, 2 * (xx >> 1) + 1].astype(np.int32) - 128
    return np.clip(np.stack([(cy * c + cbu * d + 128) >> 8, (cy * c - cgu * d - cgv * e + 128) >> 8, (cy * c + crv * e + 128) >> 8], -1), 0, 255).astype(np.uint8)


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
    sizes = [(1920, 1080), (1280, 720), (640, 480), (640, 424), (320, 320)]
    pics = {}
    for w, h in sizes:
        Y, UV = bgr_to_nv12(np.resize(src, (h, w, 3)))
        pics[(w, h)] = (Y, UV, nv12_to_bgr(Y, UV))
    keep, nsets, bsets = [], [], []
    for _ in range(3):                                                  # three buffer sets of the same pictures
        ndesc, bdesc, nshared, bshared, nlay, blay = [], [], [], [], [], []
        for f in range(B):
            w, h = sizes[f % len(sizes)]
            Y, UV, img = pics[(w, h)]
            pad = 64 if f % 3 == 1 else 0                                # some padded pitches
            py, pu, pb = w + pad, w + pad, 3 * w + pad
            surf = np.zeros((h + h // 2, py), np.uint8)                  # one contiguous surface: uv = y + pitch_y h
            surf[:h, :w] = Y
            surf[h:, :w] = UV
            rows = np.zeros((h, pb), np.uint8)
            rows[:, :3 * w] = img.reshape(h, 3 * w)
            if f % 4 == 0:                                              # some frames inside one shared allocation, at odd offsets (NV12: the chroma plane stays even)
                no = sum(r.size + 2 for r in nshared) + 1
                no += (no + py * h) & 1
                nlay.append((f, no, w, h, py, pu))
                nshared.append(surf)
                blay.append((f, sum(r.size + 1 for r in bshared) + 1, w, h, pb))
                bshared.append(rows)
                ndesc.append(None)
                bdesc.append(None)
            else:
                t, u = torch.from_numpy(surf).cuda(), torch.from_numpy(rows).cuda()
                keep += [t, u]
                ndesc.append((t.data_ptr(), 0, w, h, py, pu, 0))
                bdesc.append((u.data_ptr(), w, h, pb))
        nbig = torch.from_numpy(np.concatenate([np.concatenate([[0, 0], r.reshape(-1)]).astype(np.uint8) for r in nshared] + [np.zeros(8, np.uint8)])).cuda()
        bbig = torch.from_numpy(np.concatenate([np.concatenate([[0], r.reshape(-1)]).astype(np.uint8) for r in bshared] + [np.zeros(8, np.uint8)])).cuda()
        keep += [nbig, bbig]
        for f, o, w, h, py, pu in nlay:
            ndesc[f] = (nbig.data_ptr() + o, 0, w, h, py, pu, 0)
        for f, o, w, h, pb in blay:
            bdesc[f] = (bbig.data_ptr() + o, w, h, pb)
        nsets.append(ndesc)
        bsets.append(bdesc)
    mean, norm = (0.0, 0.0, 0.0), (1 / 255.0,) * 3
    narrs = [(F.Nv12Frame * B)(*[F.Nv12Frame(*F.nv12_frame_desc(d)) for d in desc]) for desc in nsets]      # (built once: the loop times the library)
    barrs = [(F.BgrFrame * B)(*[F.BgrFrame(*F.bgr_frame_desc(d)) for d in desc]) for desc in bsets]
    cm, cn = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*norm)
    L = F.lib()
    net = F.Net()
    regimes = {"chains": (4, F.FFGPU.CONCURRENT), "single": (1, 0)}
    out = {"batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    modes = ["a", "b", "c", "d"]
    for rname, (E, flags) in regimes.items():
        execs = [net.executor(B, flags) for _ in range(E)]
        streams = [torch.cuda.Stream() for _ in range(E)]

        def run(mode):
            os.environ.pop("FFGPU_NO_U8_FRONT", None)
            os.environ.pop("FFGPU_NV12_FRONT", None)
            if mode == "a":
                os.environ["FFGPU_NV12_FRONT"] = "1"
            if mode == "b":
                os.environ["FFGPU_NO_U8_FRONT"] = "1"

            def one(k):
                ex, st = execs[k % E], streams[k % E].cuda_stream
                if mode == "d":
                    ex.forward_bgr_dev(u320.data_ptr(), 320, 320, mean, norm, stream=st)
                elif mode == "c":
                    if L.ffgpu_exec_forward_bgr_frames_dev(ex.h, barrs[k % 3], B, cm, cn, st) < 0:
                        raise RuntimeError(F.last_error())
                else:
                    if L.ffgpu_exec_forward_nv12_frames_dev(ex.h, narrs[k % 3], B, cm, cn, st) < 0:
                        raise RuntimeError(F.last_error())
            for k in range(a.warmup):
                one(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.steps):
                one(k)
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) * 1e6 / a.steps
            last[mode] = execs[(a.steps - 1) % E].read_dets().tobytes()      # (untimed) the records of the last step
            return us

        res, last = {m: [] for m in modes}, {}
        for r in range(a.repeats):
            for m in (modes if r % 2 == 0 else modes[::-1]):
                res[m].append(run(m))
        os.environ.pop("FFGPU_NO_U8_FRONT", None)
        os.environ.pop("FFGPU_NV12_FRONT", None)
        if not (last["a"] == last["b"] == last["c"]):                   # the three routes saw the same pictures (set (steps - 1) % 3 each)
            raise RuntimeError("%s: the records of legs a, b, c differ" % rname)
        o = {"executors": E, "flags": flags, "graph_captures": [ex.graph_captures for ex in execs]}
        for m in modes:
            med = float(np.median(res[m]))
            o[m] = {"us_per_step": [round(v, 2) for v in res[m]], "median_us": round(med, 2), "spread_us": round(max(res[m]) - min(res[m]), 2),
                    "frames_per_s": round(B / med * 1e6, 1)}
        o["a_vs_b"] = round(o["b"]["median_us"] / o["a"]["median_us"], 4)
        o["a_vs_c"] = round(o["c"]["median_us"] / o["a"]["median_us"], 4)
        o["b_vs_c"] = round(o["c"]["median_us"] / o["b"]["median_us"], 4)
        o["a_vs_d"] = round(o["d"]["median_us"] / o["a"]["median_us"], 4)
        o["fused_beats_staged_by_more_than_spread"] = bool(o["b"]["median_us"] - o["a"]["median_us"] > max(o["a"]["spread_us"], o["b"]["spread_us"]))
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
