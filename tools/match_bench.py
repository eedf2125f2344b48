#!/usr/bin/env python3
"""Device time of re-identification: ffgpu_match_dev at nq in {64, 256}, D in {128, 512}, capacity in {1 024, 65 536}, k in {1, 5}, with
d_sim as well at the small gallery; ffgpu_gallery_enroll_dev at nq = 256 (nobody known: every query is enrolled, the head reset in front of each
sample); and as yardsticks in the same run ffgpu_topk_dev on 64 rows of 1 024 and the batch-64 forward of data/test.bmp.  HIP events on one stream, one
process, the measurements alternating over `repeats` rounds of 20 warm-up + 100 timed launches, a forward enqueued in front of every sample so that the
events bracket device work and not the host's pace.  Each match shape also carries its two fractions: gallery bytes per second against 8 TB/s and
2 nq capacity D flop per second against the 157.3 TFLOP/s fp32 matrix peak.  Prints one JSON object; with a path argument it is written there too:
    python tools/match_bench.py [profiles/match_bench.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, REPEATS = 64, 3
HBM_BPS, MATRIX_FLOPS = 8e12, 157.3e12
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"forward_batch": B, "warmup": 20, "timed": 100, "repeats": REPEATS, "hbm_bytes_per_s": HBM_BPS, "fp32_matrix_flop_per_s": MATRIX_FLOPS}


def timed(busy, fn, pre=None):
    for _ in range(20):
        busy()
        if pre:
            pre()
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for a, b in ev:
        busy()
        if pre:
            pre()
        a.record(st)
        assert fn() == 0
        b.record(st)
    st.synchronize()
    return sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)


rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
pic = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
ftab = F.bgr_frame_table([(pic.data_ptr(), w, h, rows.shape[1])] * B)
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
net = F.Net()
with net.executor(B) as ex:
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)
    assert fwd() == 0, F.last_error()
    gen = torch.Generator(device="cuda").manual_seed(5800)
    NQ, CAP, DMAX, KMAX = 256, 65536, 512, 5
    queries = torch.randn(NQ * DMAX, generator=gen, device="cuda", dtype=torch.float32)
    gallery = torch.randn(CAP * DMAX, generator=gen, device="cuda", dtype=torch.float32)
    ids = torch.arange(CAP, dtype=torch.int32, device="cuda")
    labels = torch.zeros(2 * NQ * KMAX, dtype=torch.int32, device="cuda")
    sim = torch.zeros(NQ * 1024, dtype=torch.float32, device="cuda")
    wb = F.match_workspace_bytes(NQ, CAP, KMAX)
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    fns, pres, shapes = {"forward": fwd}, {}, {}
    for cap in (1024, CAP):
        for d in (128, 512):
            g = F.gallery(gallery.data_ptr(), cap, d, ids.data_ptr(), None)
            for nq in (64, 256):
                for k in (1, 5):
                    for with_sim in ((False, True) if cap == 1024 and k == 5 else (False,)):
                        name = "match_nq%d_d%d_cap%d_k%d%s" % (nq, d, cap, k, "_sim" if with_sim else "")
                        shapes[name] = (nq, d, cap)
                        fns[name] = (lambda g=g, nq=nq, d=d, k=k, ds=sim.data_ptr() if with_sim else None, cap=cap:
                                     L.ffgpu_match_dev(queries.data_ptr(), nq, d, g, k, labels.data_ptr(), ds, cap, work.data_ptr(), wb, S))
    # enrolment: an empty gallery of 256 x 512, 256 queries nobody knows (each fills it)
    head = torch.zeros(4, dtype=torch.int32, device="cuda")
    unknown = torch.full((2 * NQ,), -1, dtype=torch.int32, device="cuda")
    e_out = torch.zeros(2 * NQ, dtype=torch.int32, device="cuda")
    e_rows = torch.zeros(NQ * DMAX, dtype=torch.float32, device="cuda")
    e_ids = torch.zeros(NQ, dtype=torch.int32, device="cuda")
    ge = F.gallery(e_rows.data_ptr(), NQ, DMAX, e_ids.data_ptr(), head.data_ptr())
    fns["enroll_nq256_d512"] = lambda: L.ffgpu_gallery_enroll_dev(ge, queries.data_ptr(), NQ, DMAX, unknown.data_ptr(), 1, 0.5, e_out.data_ptr(), S)

    def empty_again():
        with torch.cuda.stream(st):
            head.zero_()
    pres["enroll_nq256_d512"] = empty_again
    rows1024 = torch.randn(64 * 1024, generator=gen, device="cuda", dtype=torch.float32)
    fns["topk_5_of_1024_x64"] = lambda: L.ffgpu_topk_dev(rows1024.data_ptr(), 64, 1024, 1024, 5, labels.data_ptr(), S)
    samples = {}
    for name, fn in fns.items():
        if name in pres:
            pres[name]()
        assert fn() == 0, (name, F.last_error())
        samples[name] = []
    st.synchronize()
    assert head.cpu().tolist() == [NQ, NQ, 0, 0] and e_ids.cpu().tolist() == list(range(1, NQ + 1)) and torch.equal(e_rows, queries)
    for _ in range(REPEATS):
        for name, fn in fns.items():
            samples[name] += timed(fwd, fn, pres.get(name))
    for name, v in samples.items():
        v.sort()
        out[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
    for name, (nq, d, cap) in shapes.items():
        t = out[name]["median_us"] * 1e-6
        out[name]["gallery_bytes"] = 4 * cap * d
        out[name]["flop"] = 2 * nq * cap * d
        out[name]["hbm_fraction"] = round(4 * cap * d / t / HBM_BPS, 4)
        out[name]["matrix_fraction"] = round(2 * nq * cap * d / t / MATRIX_FLOPS, 4)
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
