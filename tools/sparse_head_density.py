#!/usr/bin/env python3
"""How the sparse form of the yolo heads' input layers (FFGPU_SPARSE_HEAD) depends on the density of detections:
    python tools/sparse_head_density.py [batch]
For three inputs -- the bench's batch (frame 0 the test image, the rest uniform noise), `batch` copies of the test image, and the bench's batch under a
copy of the cfg with ignore_thresh = 0 (every cell passes: the worst case, the dense launch's work plus the box pass) -- it prints, per head, the share
of pixel quads the box pass lists (k_yolo's predicate evaluated on the host from the head layer of an FFGPU_KEEP_ALL executor) and the time of the head's
launch(es) with the form on and off (ffgpu_exec_profile_steps of an FFGPU_CONCURRENT executor: one chain alone, event-timed per step, five repetitions)."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ffcnn_amd import capi

YOLO_KIND = 7
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64


def listed_share(ex, net, layer, thresh):
    """share of the quads of four consecutive cells with a (cell, anchor) whose objectness passes !(1 / (1 + e^-bs) < thresh * 0.999f)"""
    t = np.float32(thresh) * np.float32(0.999)
    hit = tot = 0
    for n in range(B):
        a = ex.read_layer(layer, n)
        A = a.shape[0] // 3
        with np.errstate(over="ignore"):
            s = np.float32(1) / (np.float32(1) + np.exp(-a[4::A].reshape(3, -1, 4)))
        q = (~(s < t)).any(axis=(0, 2))
        hit += int(q.sum())
        tot += q.size
    return hit / tot


def head_times(net, x, heads):
    out = {}
    for knob in ("1", "0"):
        os.environ["FFGPU_SPARSE_HEAD"] = knob
        with net.executor(B, capi.FFGPU.CONCURRENT) as ex:
            ex.profile_steps(x.data_ptr())                       # warm
            steps = ex.profile_steps(x.data_ptr())
            out[knob] = [sum(us for lay, us in steps if lay == h) for h in heads] + [sum(us for _, us in steps)]
    os.environ.pop("FFGPU_SPARSE_HEAD", None)
    return out


def main():
    text = open(capi.CFG).read()
    tmp = tempfile.NamedTemporaryFile("w", suffix=".cfg", delete=False)
    tmp.write(text.replace("ignore_thresh = .45", "ignore_thresh = 0"))
    tmp.close()
    with capi.Net() as net:
        bgr, w, h = capi.load_bmp(os.path.join(capi.DATA, "test.bmp"))
        net.set_input_image(bgr, w, h)
        img = torch.from_numpy(net.input.copy()).cuda()
    g = torch.Generator(device="cuda").manual_seed(1236)
    bench = torch.rand((B, 3, 320, 320), device="cuda", generator=g)
    bench[0] = img
    copies = img.unsqueeze(0).repeat(B, 1, 1, 1).contiguous()
    print("batch %d; time in us of the head's launch(es), one FFGPU_CONCURRENT chain alone; share = listed quads / all quads" % B)
    for name, cfg, x in (("bench batch", capi.CFG, bench), ("%d x test image" % B, capi.CFG, copies), ("every cell passes", tmp.name, bench)):
        with capi.Net(cfg=cfg) as net:
            heads = [i - 1 for i in range(net.layer_num) if net.layer(i).type == YOLO_KIND]
            thresh = [float(net.layer(i).ignore_thres) for i in range(net.layer_num) if net.layer(i).type == YOLO_KIND]
            with net.executor(B, capi.FFGPU.KEEP_ALL) as ex:
                ex.forward_dev(x.data_ptr())
                torch.cuda.synchronize()
                share = [listed_share(ex, net, hl, th) for hl, th in zip(heads, thresh)]
                boxes = sum(int(d["count"]) for d in ex.read_dets())
            t = head_times(net, x, heads)
            for k, hl in enumerate(heads):
                o = net.out_shape(hl)
                print("%-18s layer %3d (%dx%d)  share %6.2f %%  sparse %6.1f us  dense %6.1f us" % (name, hl, o[2], o[1], 100 * share[k], t["1"][k], t["0"][k]))
            print("%-18s boxes in the batch %d; sum of the forward's steps: sparse %.1f us, dense %.1f us" % (name, boxes, t["1"][-1], t["0"][-1]))
    os.unlink(tmp.name)


if __name__ == "__main__":
    main()
