"""ffgpu_exec_forward_bgr_frames_dev: a batch of u8 BGR frames that each have their own device pointer, size and pitch, letterboxed
per frame exactly as net_input (ffcnn.c:259-289) and rescaled per frame.  Staged path (k_input_frames + the fp32 graph) and fused path
(the resizing k_front) against the oracle, against each other, against forward_bgr_dev, in stream order with a record ring, and the
error cases.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests it
extends, after the BASELINE and parity files and before the stress tests.)"""
import os

import numpy as np
import pytest

from test_gpu_parity import _write_random_weights, boxes_match
from test_gpu_round2 import F, close, net  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
SETTING = ((104.0, 117.0, 123.0), (0.017, 0.0175, 0.0171))


def align4(v):
    return (v + 3) & ~3


class Frames:
    """device frames at chosen pitches and byte offsets: a list of (w, h, pitch or 0, offset, shared) specs.  Frames with shared=True
    live one behind the other in one allocation, the others in allocations of their own."""

    def __init__(self, imgs, specs):
        import torch
        self.keep, self.desc, self.packed = [], [], []
        shared, lay = [], []
        for (w, h, pitch, off, sh), img in zip(specs, imgs):
            p = pitch or align4(3 * w)
            buf = np.zeros((off + p * h + 8,), np.uint8)
            buf[off:off + p * h].reshape(h, p)[:, :3 * w] = img.reshape(h, 3 * w)
            pk = np.zeros((h, align4(3 * w)), np.uint8)
            pk[:, :3 * w] = img.reshape(h, 3 * w)
            self.packed.append(pk)
            if sh:
                lay.append((len(self.desc), sum(len(b) for b in shared) + off, w, h, pitch))
                shared.append(buf)
                self.desc.append(None)
            else:
                d = torch.from_numpy(buf).cuda()
                self.keep.append(d)
                self.desc.append((d.data_ptr() + off, w, h, pitch))
        if shared:
            big = torch.from_numpy(np.concatenate(shared)).cuda()
            self.keep.append(big)
            for k, o, w, h, pitch in lay:
                self.desc[k] = (big.data_ptr() + o, w, h, pitch)


def rand_img(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def oracle_run(o, pk, w, h, mean, norm):
    """the oracle's net_input + net_forward of one frame: every layer's output, the candidate count, the boxes"""
    o.set_input_image(np.ascontiguousarray(pk), w, h, mean, norm)
    o.forward(0)
    acts = {}
    for i in range(o.nlayers):
        a = o.layer_out(i)
        if a is not None:
            acts[i] = a.copy()
    return dict(acts=acts, cand=len(o.candidates), boxes=o.boxes, input=np.array(o.input))


@pytest.fixture(scope="module")
def pool(orc, test_image):
    """distinct source images (test.bmp at 640 x 424 among them) with their specs, and the oracle's run of each"""
    bgr, w, h = test_image
    src = np.frombuffer(bgr, np.uint8).reshape(h, align4(3 * w))[:, :3 * w].reshape(h, w, 3)
    rng = np.random.default_rng(77)
    big = np.ascontiguousarray(np.resize(src, (1080, 1920, 3)))
    imgs = [src, big, np.ascontiguousarray(big[:720, :1280]), np.ascontiguousarray(src[:480, :640] if h >= 480 else np.resize(src, (480, 640, 3))),
            np.ascontiguousarray(src[64:384, 150:470]), rand_img(rng, 321, 319), rand_img(rng, 1, 1000), np.ascontiguousarray(src[:300, ::3])]
    specs = [(640, 424, 0, 0, False), (1920, 1080, 5763, 1, True), (1280, 720, 0, 2, True), (640, 480, 1925, 3, False),
             (320, 320, 0, 0, False), (321, 319, 965, 1, True), (1, 1000, 0, 3, False), (imgs[7].shape[1], 300, 0, 2, True)]
    mean, norm = SETTING
    o = orc.Oracle()
    runs = []
    for (w_, h_, _, _, _), img in zip(specs, imgs):
        pk = np.zeros((h_, align4(3 * w_)), np.uint8)
        pk[:, :3 * w_] = img.reshape(h_, 3 * w_)
        runs.append(oracle_run(o, pk, w_, h_, mean, norm))
    o.close()
    return imgs, specs, runs


def batch_of(pool, n):
    imgs, specs, runs = pool
    order = [(3 * f + f // 5) % len(imgs) for f in range(n)]
    return order, Frames([imgs[k] for k in order], [specs[k] for k in order])


@pytest.mark.parametrize("seed", range(3))
def test_staged_input_tensor_bit_identical(F, net, orc, seed):
    """batches 1-5 (below k_front's threshold: the staged path): read_layer(-1) of every frame is bit for bit the oracle's net_input"""
    import torch
    rng = np.random.default_rng(9100 + seed)
    o = orc.Oracle()
    for case in range(6):
        B = int(rng.integers(1, 6))
        specs, imgs = [], []
        for _ in range(B):
            w = int(rng.choice([1, 2, 3, 7, 160, 319, 320, 321, 641, 1000, int(rng.integers(1, 900))]))
            h = int(rng.choice([1, 3, 200, 319, 320, 321, 450, 1000, int(rng.integers(1, 700))]))
            pitch = int(rng.choice([0, align4(3 * w), 3 * w, 3 * w + 5, align4(3 * w) + 64]))
            specs.append((w, h, pitch, int(rng.integers(0, 4)), bool(rng.random() < 0.5)))
            imgs.append(rand_img(rng, w, h))
        if case == 0:
            specs[0], imgs[0] = (320, 320, 0, 0, False), rand_img(rng, 320, 320)
        if case == 1:                                               # degenerate letterboxes: sw == 0 (1 x 1000) and sh == 0 (1000 x 1)
            specs[0], imgs[0] = (1, 1000, 0, 1, False), rand_img(rng, 1, 1000)
            specs.append((1000, 1, 3001, 2, True))
            imgs.append(rand_img(rng, 1000, 1))
            B += 1
        mean = tuple(float(v) for v in rng.uniform(0, 128, 3))
        norm = tuple(float(v) for v in rng.uniform(0.002, 0.02, 3))
        fr = Frames(imgs, specs)
        with net.executor(B, F.FFGPU.KEEP_ALL) as ex:
            ex.forward_bgr_frames_dev(fr.desc, mean, norm)
            torch.cuda.synchronize()
            for f in range(B):
                w, h = specs[f][:2]
                o.set_input_image(np.ascontiguousarray(fr.packed[f]), w, h, mean, norm)
                assert np.array_equal(ex.read_layer(-1, f), np.array(o.input)), "case %d frame %d: %s" % (case, f, specs[f])
    o.close()


@pytest.mark.parametrize("batch,flags", [(16, 64), (37, 64), (64, 64), (32, 32)])
def test_fused_against_oracle_and_staged(F, net, pool, batch, flags, monkeypatch):
    """mixed batches on plans that start with k_front: every materialised layer, the candidate count and the boxes of every frame
    against the oracle's run of that frame alone; test.bmp frames against the golden boxes; the staged path (FFGPU_NO_U8_FRONT) gives
    the same bytes"""
    import json
    import torch
    from conftest import GOLD
    gold = json.load(open(os.path.join(GOLD, "boxes.json")))["net_320x320_v0"]["boxes"]
    order, fr = batch_of(pool, batch)
    runs = pool[2]
    mean, norm = SETTING
    keep = F.FFGPU.KEEP_ALL if not flags & F.FFGPU.SPLIT2 else 0
    with net.executor(batch, keep | flags) as ex:
        ex.forward_bgr_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        dets = ex.read_dets()
        mat = [i for i, hv in enumerate(ex.hash_layers()) if hv] if keep else []
        assert not keep or len(mat) > 20
        for f in range(batch):
            want = runs[order[f]]
            for i in mat:
                close(ex.read_layer(i, f), want["acts"][i], "batch %d frame %d layer %d" % (batch, f, i))
            assert dets[f]["ncand"] == want["cand"], "frame %d" % f
            boxes_match(ex.boxes(f, dets), want["boxes"], "batch %d frame %d" % (batch, f))
        if keep:
            with pytest.raises(RuntimeError, match="no fp32 input tensor exists"):
                ex.read_layer(-1, 0)
        fused = dets.tobytes()
        monkeypatch.setenv("FFGPU_NO_U8_FRONT", "1")
        ex.forward_bgr_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        assert ex.read_dets().tobytes() == fused, "staged path differs"
        if keep:
            assert ex.read_layer(-1, 0).shape == (3, 320, 320)
        monkeypatch.delenv("FFGPU_NO_U8_FRONT")
    # test.bmp with the reference's default mean / norm: the golden boxes
    bmp = [f for f in range(batch) if order[f] == 0]
    with net.executor(batch, flags) as ex:
        ex.forward_bgr_frames_dev(fr.desc)
        torch.cuda.synchronize()
        dets = ex.read_dets()
        for f in bmp:
            boxes_match(ex.boxes(f, dets), gold, "golden boxes frame %d" % f)


@pytest.mark.parametrize("w,h", [(320, 320), (640, 424)])
def test_uniform_batch_matches_forward_bgr_dev(F, net, pool, w, h):
    """a uniform batch through the new entry gives the records of forward_bgr_dev on the same frames, byte for byte; the 320 x 320
    frames of a mixed batch give the records they have in the uniform batch"""
    import torch
    imgs, specs, _ = pool
    k = 0 if (w, h) == (640, 424) else 4
    B = 16
    mean, norm = SETTING
    one = torch.from_numpy(np.ascontiguousarray(np.repeat(Frames([imgs[k]], [(w, h, 0, 0, False)]).packed[0][None], B, 0))).cuda()
    pitch = align4(3 * w)
    with net.executor(B, 0) as ex:
        ex.forward_bgr_dev(one.data_ptr(), w, h, mean, norm)
        torch.cuda.synchronize()
        want = ex.read_dets()
        ex.forward_bgr_frames_dev([(one.data_ptr() + f * pitch * h, w, h, 0) for f in range(B)], mean, norm)
        torch.cuda.synchronize()
        got = ex.read_dets()
        assert got.tobytes() == want.tobytes()
        if k == 4:
            order, fr = batch_of(pool, B)
            ex.forward_bgr_frames_dev(fr.desc, mean, norm)
            torch.cuda.synchronize()
            mixed = ex.read_dets()
            hits = [f for f in range(B) if order[f] == 4]
            assert hits
            for f in hits:
                assert mixed[f].tobytes() == want[0].tobytes(), "frame %d" % f


@pytest.mark.parametrize("fused", [True, False])
def test_stream_order_ring_and_captures(F, net, pool, fused, monkeypatch):
    """three calls back to back on one stream, different descriptor sets, no host sync, a 3-slot ring: each slot holds its own set's
    records; the first call of the entry captures exactly one graph on the fused path (the resizing first kernel's) and none on the staged
    one (the fp32 graph exists from the executor's creation), later calls none"""
    import torch
    if not fused:
        monkeypatch.setenv("FFGPU_NO_U8_FRONT", "1")
    B = 16
    mean, norm = SETTING
    sets = []
    for s in range(3):
        order, fr = batch_of(pool, B)
        perm = [(f + 5 * s) % B for f in range(B)]
        fr.desc = [fr.desc[p] for p in perm]
        sets.append(fr)
    with net.executor(B, F.FFGPU.CONCURRENT) as ex:
        want = []
        for fr in sets:
            ex.forward_bgr_frames_dev(fr.desc, mean, norm)
            torch.cuda.synchronize()
            want.append(ex.read_dets())
        caps = ex.graph_captures
        ring = torch.zeros(3 * B * F.DETS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        ex.set_ring(ring.data_ptr(), 3)
        st = torch.cuda.Stream()
        for fr in sets:
            ex.forward_bgr_frames_dev(fr.desc, mean, norm, stream=st.cuda_stream)
        st.synchronize()
        got = np.frombuffer(ring.cpu().numpy().tobytes(), F.DETS_DTYPE).reshape(3, B)
        for s in range(3):
            assert got[s].tobytes() == want[s].tobytes(), "slot %d" % s
        assert ex.graph_captures == caps
        ex.set_ring(None, 0)
    with net.executor(B, F.FFGPU.CONCURRENT) as ex:
        c0 = ex.graph_captures
        ex.forward_bgr_frames_dev(sets[0].desc, mean, norm)
        c1 = ex.graph_captures
        assert c1 == c0 + (1 if fused else 0)
        for fr in sets[1:]:
            ex.forward_bgr_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        assert ex.graph_captures == c1


def test_executor_scale_unchanged(F, net, pool, orc):
    """after a call of the new entry, forward_dev still rescales by the executor's own set_scale"""
    import torch
    imgs, specs, runs = pool
    B = 16
    order, fr = batch_of(pool, B)
    o = orc.Oracle()
    o.set_input_image(np.ascontiguousarray(fr.packed[0]), specs[order[0]][0], specs[order[0]][1])
    x = torch.from_numpy(np.repeat(np.array(o.input)[None], B, 0)).cuda()
    o.n.s1, o.n.s2 = 3, 2
    o.forward(0)
    want = o.boxes
    o.close()
    with net.executor(B, 0) as ex:
        ex.set_scale(3, 2)
        ex.forward_bgr_frames_dev(fr.desc)
        ex.forward_dev(x.data_ptr())
        torch.cuda.synchronize()
        boxes_match(ex.boxes(0), want, "forward_dev after the frames entry")


def test_tiny3_staged_only(F, orc, tmp_path):
    """tests/data/tiny3.cfg (96 x 64, no k_front): mixed sizes through the staged path, every layer and every box against the oracle"""
    import torch
    from conftest import ROOT
    cfg = os.path.join(ROOT, "tests", "data", "tiny3.cfg")
    o = orc.Oracle(cfg=cfg, weights=None)
    wpath = str(tmp_path / "tiny3.weights")
    _write_random_weights(wpath, o, 7)
    o.close()
    o = orc.Oracle(cfg=cfg, weights=wpath)
    rng = np.random.default_rng(12)
    specs = [(96, 64, 0, 0, False), (200, 90, 601, 1, True), (50, 120, 0, 3, True), (97, 63, 0, 2, False), (3, 400, 10, 1, False)]
    imgs = [rand_img(rng, w, h) for (w, h, _, _, _) in specs]
    fr = Frames(imgs, specs)
    mean, norm = (10.0, 20.0, 30.0), (0.01, 0.012, 0.011)
    with F.Net(cfg, wpath) as n:
        with n.executor(len(specs), F.FFGPU.KEEP_ALL | F.FFGPU.NO_FUSE) as ex:
            ex.forward_bgr_frames_dev(fr.desc, mean, norm)
            torch.cuda.synchronize()
            dets = ex.read_dets()
            for f, (w, h, _, _, _) in enumerate(specs):
                o.set_input_image(np.ascontiguousarray(fr.packed[f]), w, h, mean, norm)
                assert np.array_equal(ex.read_layer(-1, f), np.array(o.input)), "input frame %d" % f
                o.forward(0)
                for i in range(o.nlayers):
                    ref = o.layer_out(i)
                    if ref is not None:
                        close(ex.read_layer(i, f), ref, "tiny3 frame %d layer %d" % (f, i))
                assert dets[f]["ncand"] == len(o.candidates)
                boxes_match(ex.boxes(f, dets), o.boxes, "tiny3 boxes frame %d" % f)
    o.close()


def test_error_cases(F, net, pool):
    """every bad argument: an error with a message, and the executor still gives correct records afterwards"""
    import ctypes as C
    import torch
    B = 16
    order, fr = batch_of(pool, B)
    runs = pool[2]
    mean, norm = SETTING
    L = F.lib()
    good = list(fr.desc)
    with net.executor(B, 0) as ex:
        bad = [
            (good[:-1], "frames for an executor of batch"),
            ([(0, 320, 320, 0)] + good[1:], "NULL bgr"),
            ([(good[0][0], 0, 320, 0)] + good[1:], "bad size"),
            ([(good[0][0], 320, -1, 0)] + good[1:], "bad size"),
            ([(good[0][0], 320, 320, 959)] + good[1:], "pitch"),
        ]
        for desc, msg in bad:
            with pytest.raises(RuntimeError, match=msg):
                ex.forward_bgr_frames_dev(desc, mean, norm)
        arr = (F.BgrFrame * B)(*[F.BgrFrame(*F.bgr_frame_desc(d)) for d in good])
        arr[3].reserved = 1
        m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*norm)
        assert L.ffgpu_exec_forward_bgr_frames_dev(ex.h, arr, B, m, s, None) < 0 and "reserved" in F.last_error()
        arr[3].reserved = 0
        assert L.ffgpu_exec_forward_bgr_frames_dev(ex.h, arr, B, None, s, None) < 0 and "NULL" in F.last_error()
        assert L.ffgpu_exec_forward_bgr_frames_dev(ex.h, arr, B, m, None, None) < 0 and "NULL" in F.last_error()
        assert L.ffgpu_exec_forward_bgr_frames_dev(ex.h, None, B, m, s, None) < 0 and "NULL" in F.last_error()
        ex.forward_bgr_frames_dev(good, mean, norm)
        torch.cuda.synchronize()
        dets = ex.read_dets()
        for f in range(B):
            boxes_match(ex.boxes(f, dets), runs[order[f]]["boxes"], "after errors frame %d" % f)


def test_four_columns_per_lane_plans_stage(F, net, pool, monkeypatch):
    """a plan whose first kernel runs four columns per lane (FFGPU_FRONT_NC=4; the default for planes wider than 190, i.e. nets of 384 -
    512 pixels): the resizing form exists for three columns only, so these frames take the staged path -- against the oracle, equal to
    FFGPU_NO_U8_FRONT, and no graph of the resizing kernel is captured"""
    import torch
    monkeypatch.setenv("FFGPU_FRONT_NC", "4")
    B = 16
    order, fr = batch_of(pool, B)
    runs = pool[2]
    mean, norm = SETTING
    with net.executor(B, F.FFGPU.KEEP_ALL) as ex:
        c0 = ex.graph_captures
        ex.forward_bgr_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        dets = ex.read_dets()
        assert ex.graph_captures == c0
        assert ex.read_layer(-1, 0).shape == (3, 320, 320)          # the fp32 batch exists: staged
        mat = [i for i, hv in enumerate(ex.hash_layers()) if hv]
        for f in range(B):
            want = runs[order[f]]
            assert np.array_equal(ex.read_layer(-1, f), want["input"]), "input frame %d" % f
            for i in mat:
                close(ex.read_layer(i, f), want["acts"][i], "NC 4 frame %d layer %d" % (f, i))
            assert dets[f]["ncand"] == want["cand"], "frame %d" % f
            boxes_match(ex.boxes(f, dets), want["boxes"], "NC 4 frame %d" % f)
        monkeypatch.setenv("FFGPU_NO_U8_FRONT", "1")
        ex.forward_bgr_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        assert ex.read_dets().tobytes() == dets.tobytes()
