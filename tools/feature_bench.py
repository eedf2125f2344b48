#!/usr/bin/env python3
"""Device time of the feature / top-k / relabel post-passes with 64 crop slots and head-sized last layers (255 x 10 x 10 and
1024 x 10 x 10 per frame): ffgpu_features_dev as MEAN + SOFTMAX and as FLAT, ffgpu_topk_dev (k = 5) on the rows, ffgpu_crops_relabel_dev on the table
ffgpu_exec_crop_bgr cut from a batch-64 forward of data/test.bmp, with and without the full lists -- beside ffgpu_crops_to_source_dev on the same
table, records and lists in the same run (the existing post-pass of the same kind; its code is untouched).  HIP events on one stream, one process,
the measurements alternating over `repeats` rounds of 20 warm-up + 100 timed launches, a forward enqueued in front of every sample so that the events
bracket device work and not the host's pace.  Prints one JSON object; with a path argument it is written there too:
    python tools/feature_bench.py [profiles/feature_bench.json]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, REPEATS, K = 64, 3, 5
G = F.FFGPU
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
out = {"slots": B, "warmup": 20, "timed": 100, "repeats": REPEATS, "k": K}


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


def dev_zeros(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
pic = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
frames = [(pic.data_ptr(), w, h, rows.shape[1])] * B
ftab = F.bgr_frame_table(frames)
mean, norm = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1 / 255.0, 1 / 255.0, 1 / 255.0)
net = F.Net()
with net.executor(B) as ex:
    cap = ex.cand_capacity
    fwd = lambda: L.ffgpu_exec_forward_bgr_frames_dev(ex.h, ftab, B, mean, norm, S)
    assert fwd() == 0, F.last_error()
    # the crop table of the first stage: one crop per frame, 64 slots
    slots, table = dev_zeros(B * F.crop_slot_bytes(12, 10)), dev_zeros(F.crop_table_bytes(B))
    ex.crop_bgr(frames, F.crop_spec(12, 10, F.CROP_F32, per_target=1), slots.data_ptr(), table.data_ptr(), B, stream=S)
    st.synchronize()
    hdr, _ = F.crop_table(table.cpu().numpy())
    assert hdr["taken"] == B, hdr
    recs = ex.read_dets()
    lists = np.zeros((B, cap), F.BOX_DTYPE)
    for t in range(B):
        b = ex.read_boxes(t)
        lists[t, :len(b)] = b
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    d_lists = torch.from_numpy(lists.view(np.uint8).reshape(-1).copy()).cuda()
    o_recs, o_lists = dev_zeros(recs.nbytes), dev_zeros(lists.nbytes)
    out["boxes_per_entry"], out["list_stride"] = int(recs[0]["nfull"]), cap
    samples, fns, sizes = {"forward": []}, {"forward": fwd}, {}
    rsp = F.relabel_spec(0.0, 100, G.RELABEL_LABEL_SCORE)
    gen = torch.Generator(device="cuda").manual_seed(5620)
    keep = []
    for c in (255, 1024):
        x = torch.randn(c * B * 100, generator=gen, device="cuda", dtype=torch.float32)
        prob, flat, labels = dev_zeros(4 * B * c), dev_zeros(4 * B * c * 100), dev_zeros(8 * B * K)
        keep += [x, prob, flat, labels]
        sizes[c] = {"tensor_bytes": 4 * c * B * 100}
        fns["features_mean_softmax_%dx10x10" % c] = (lambda x=x, c=c, prob=prob:
                                                      L.ffgpu_features_dev(x.data_ptr(), B, c, 10, 10, G.FEAT_MEAN, G.POST_SOFTMAX, prob.data_ptr(), c, S))
        fns["features_mean_%dx10x10" % c] = (lambda x=x, c=c, prob=prob:
                                             L.ffgpu_features_dev(x.data_ptr(), B, c, 10, 10, G.FEAT_MEAN, G.POST_NONE, prob.data_ptr(), c, S))
        fns["features_flat_%dx10x10" % c] = (lambda x=x, c=c, flat=flat:
                                             L.ffgpu_features_dev(x.data_ptr(), B, c, 10, 10, G.FEAT_FLAT, G.POST_NONE, flat.data_ptr(), 100 * c, S))
        fns["topk_%d_of_%d" % (K, c)] = lambda c=c, prob=prob, labels=labels: L.ffgpu_topk_dev(prob.data_ptr(), B, c, c, K, labels.data_ptr(), S)
    fns["relabel_with_lists"] = lambda: L.ffgpu_crops_relabel_dev(table.data_ptr(), B, labels.data_ptr(), K, d_recs.data_ptr(), d_lists.data_ptr(), cap, None, B, rsp,
                                                                  o_recs.data_ptr(), o_lists.data_ptr(), S)
    fns["relabel_records_only"] = lambda: L.ffgpu_crops_relabel_dev(table.data_ptr(), B, labels.data_ptr(), K, d_recs.data_ptr(), None, 0, None, B, rsp,
                                                                    o_recs.data_ptr(), None, S)
    fns["crops_to_source_with_lists"] = lambda: L.ffgpu_crops_to_source_dev(table.data_ptr(), B, d_recs.data_ptr(), d_lists.data_ptr(), cap, o_recs.data_ptr(),
                                                                            o_lists.data_ptr(), S)
    fns["crops_to_source_records_only"] = lambda: L.ffgpu_crops_to_source_dev(table.data_ptr(), B, d_recs.data_ptr(), None, 0, o_recs.data_ptr(), None, S)
    fns["exec_relabel"] = lambda: L.ffgpu_exec_relabel(ex.h, G.RELABEL_ENTRIES, table.data_ptr(), B, labels.data_ptr(), K, B, rsp, o_recs.data_ptr(), o_lists.data_ptr(), S)
    for name, fn in fns.items():
        assert fn() == 0, (name, F.last_error())
        samples.setdefault(name, [])
    st.synchronize()
    got = o_recs.cpu().numpy().view(F.DETS_DTYPE)
    assert (got["count"] == recs["count"]).all() and (got["box"]["type"][:, 0] >= 100).all()
    for _ in range(REPEATS):
        for name, fn in fns.items():
            samples[name] += timed(fwd, fn)
    for k, v in samples.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "p90_us": round(v[len(v) * 9 // 10], 2)}
    for c, s in sizes.items():
        for name in ("features_mean_%dx10x10" % c, "features_mean_softmax_%dx10x10" % c, "features_flat_%dx10x10" % c):
            moved = s["tensor_bytes"] * (2 if "flat" in name else 1)
            out[name]["tensor_bytes"] = s["tensor_bytes"]
            out[name]["achieved_GBps"] = round(moved / out[name]["median_us"] / 1e3, 1)
net.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
