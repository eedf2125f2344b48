"""ffgpu_exec_forward_nv12_frames_dev: a batch of NV12 frames (Y plane + interleaved U V plane, own pointers, sizes, pitches and
matrix per frame).  Frame n must behave as net_input (ffcnn.c:259-289) of the BGR image that `nv12_to_bgr` below makes of it -- the
integer formula of include/ffcnn_hip.h, nearest chroma -- then the forward.  net_input samples nearest-neighbour, so converting only the
sampled pixel is exactly converting the whole image first: the yardstick is the oracle's net_input / net_forward on the numpy-converted
image, bit for bit for the input tensor.  Staged route (k_input_nv12_frames + the fp32 graph) and fused route (the NV12 form of
k_front) against the oracle, against each other, against forward_bgr_frames_dev on the converted pictures, alternating with that
entry point in stream order with a record ring, and the error cases.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import os

import numpy as np
import pytest

from test_gpu_parity import _write_random_weights, boxes_match
from test_gpu_round2 import F, close, net  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
DEFAULT = ((0.0, 0.0, 0.0), (1 / 255.0,) * 3)                      # the reference's own setting: test.bmp keeps its three boxes through NV12
SETTING = ((104.0, 117.0, 123.0), (0.017, 0.0175, 0.0171))
SETTINGS = (DEFAULT, SETTING)

MATS = {0: (16, 298, 409, 100, 208, 516), 1: (0, 256, 359, 88, 183, 454),
        2: (16, 298, 459, 55, 136, 541), 3: (0, 256, 403, 48, 120, 475)}


def nv12_to_bgr(Y, UV, w, h, matrix):          # Y: (h, >= w) u8, UV: ((h + 1) // 2, >= 2 ((w + 1) // 2)) u8
    yoff, cy, crv, cgu, cgv, cbu = MATS[matrix]
    yy, xx = np.mgrid[0:h, 0:w]
    c = Y[yy, xx].astype(np.int32) - yoff
    d = UV[yy >> 1, 2 * (xx >> 1)].astype(np.int32) - 128
    e = UV[yy >> 1, 2 * (xx >> 1) + 1].astype(np.int32) - 128
    r = (cy * c + crv * e + 128) >> 8
    g = (cy * c - cgu * d - cgv * e + 128) >> 8
    b = (cy * c + cbu * d + 128) >> 8
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)      # (h, w, 3), B G R


def bgr_to_nv12(img):
    """a picture as a decoder would hand it over: BT.601 limited range, chroma = mean of each 2 x 2 block (edge blocks of odd sizes:
    of the pixels they have)"""
    h, w = img.shape[:2]
    b, g, r = (img[..., k].astype(np.float64) for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def sub(p):
        q = np.full((2 * ch, 2 * cw), np.nan)
        q[:h, :w] = p
        return np.nanmean(q.reshape(ch, 2, cw, 2), axis=(1, 3))
    UV = np.stack([sub(u), sub(v)], -1).reshape(ch, 2 * cw)
    return np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(UV), 0, 255).astype(np.uint8)


def align4(v):
    return (v + 3) & ~3


def pack_bgr(img):
    h, w = img.shape[:2]
    pk = np.zeros((h, align4(3 * w)), np.uint8)
    pk[:, :3 * w] = img.reshape(h, 3 * w)
    return pk


class Nv12Frames:
    """device NV12 frames at chosen pitches and byte offsets: planes is a list of (Y (h, w), UV (ceil(h / 2), 2 ceil(w / 2))), specs a list
    of (w, h, pitch_y or 0, pitch_uv or 0, offset 0-3, uv_mode, shared, matrix).  uv_mode "null": one contiguous surface, the descriptor's
    uv is NULL (uv = y + pitch_y h; the offset is moved by one where that address would be odd); "explicit": the chroma plane starts behind
    the Y plane's height aligned up to 16 rows, as decoders with aligned surface heights lay it out, and is named.  Frames with shared=True
    live one behind the other in one allocation, the others in allocations of their own."""

    def __init__(self, planes, specs):
        import torch
        self.keep, self.desc, self.bgr = [], [], []
        shared, lay = [], []
        for (w, h, pitch_y, pitch_uv, off, uv_mode, sh, matrix), (Y, UV) in zip(specs, planes):
            py, cw, ch = pitch_y or w, 2 * ((w + 1) // 2), (h + 1) // 2
            pu = pitch_uv or cw
            assert Y.shape == (h, w) and UV.shape == (ch, cw) and py >= w and pu >= cw and pu % 2 == 0
            if uv_mode == "null":
                if (off + py * h) & 1:
                    off ^= 1
                uvo = off + py * h
            else:
                uvo = off + py * ((h + 15) & ~15)
                uvo += uvo & 1
            buf = np.full((uvo + pu * ch + 8 + 1) & ~1, 0x5a, np.uint8)      # (even length: every frame of a shared allocation starts even)
            buf[off:off + py * h].reshape(h, py)[:, :w] = Y
            buf[uvo:uvo + pu * ch].reshape(ch, pu)[:, :cw] = UV
            self.bgr.append(nv12_to_bgr(Y, UV, w, h, matrix))
            d = (off, 0 if uv_mode == "null" else uvo, w, h, pitch_y, pitch_uv, matrix)
            if sh:
                lay.append((len(self.desc), sum(len(b) for b in shared), d))
                shared.append(buf)
                self.desc.append(None)
            else:
                t = torch.from_numpy(buf).cuda()
                self.keep.append(t)
                self.desc.append(self._at(t.data_ptr(), d))
        if shared:
            big = torch.from_numpy(np.concatenate(shared)).cuda()
            self.keep.append(big)
            for k, o, d in lay:
                self.desc[k] = self._at(big.data_ptr() + o, d)

    @staticmethod
    def _at(base, d):
        off, uvo, w, h, pitch_y, pitch_uv, matrix = d
        return (base + off, base + uvo if uvo else 0, w, h, pitch_y, pitch_uv, matrix)


class BgrFrames:
    """the same pictures as packed u8 BGR frames (pitch ALIGN(3 w, 4)), each in its own allocation"""

    def __init__(self, imgs):
        import torch
        self.keep = [torch.from_numpy(pack_bgr(img)).cuda() for img in imgs]
        self.desc = [(t.data_ptr(), img.shape[1], img.shape[0], 0) for t, img in zip(self.keep, imgs)]


def rand_planes(rng, w, h):
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=np.uint8))


def oracle_run(o, img, mean, norm):
    """the oracle's net_input + net_forward of one BGR picture: every layer's output, the candidate count, the boxes"""
    h, w = img.shape[:2]
    o.set_input_image(np.ascontiguousarray(pack_bgr(img)), w, h, mean, norm)
    o.forward(0)
    acts = {}
    for i in range(o.nlayers):
        a = o.layer_out(i)
        if a is not None:
            acts[i] = a.copy()
    return dict(acts=acts, cand=len(o.candidates), boxes=o.boxes, input=np.array(o.input))


@pytest.fixture(scope="module")
def pool(orc, test_image):
    """distinct pictures as NV12 (test.bmp at 640 x 424 with matrix 0 among them), their specs, and the oracle's run of each converted picture
    under each of SETTINGS"""
    bgr, w, h = test_image
    src = np.frombuffer(bgr, np.uint8).reshape(h, align4(3 * w))[:, :3 * w].reshape(h, w, 3)
    rng = np.random.default_rng(78)
    big = np.ascontiguousarray(np.resize(src, (1080, 1920, 3)))
    imgs = [src, big, np.ascontiguousarray(big[:720, :1280]), np.ascontiguousarray(src[:480, :640] if h >= 480 else np.resize(src, (480, 640, 3))),
            np.ascontiguousarray(src[64:384, 150:470]), None, None, np.ascontiguousarray(src[:301, ::3])]
    planes = [bgr_to_nv12(i) if i is not None else None for i in imgs]
    planes[5], planes[6] = rand_planes(rng, 321, 319), rand_planes(rng, 1, 1000)
    w7 = imgs[7].shape[1]
    specs = [(640, 424, 0, 0, 0, "null", False, 0), (1920, 1080, 1923, 1984, 1, "explicit", True, 2), (1280, 720, 0, 0, 2, "null", True, 3),
             (640, 480, 704, 642, 3, "explicit", False, 1), (320, 320, 0, 0, 0, "null", False, 0), (321, 319, 325, 0, 1, "null", True, 1),
             (1, 1000, 0, 0, 3, "explicit", False, 2), (w7, 301, 0, 2 * ((w7 + 1) // 2) + 6, 2, "explicit", True, 3)]
    o = orc.Oracle()
    conv = [nv12_to_bgr(Y, UV, s[0], s[1], s[7]) for s, (Y, UV) in zip(specs, planes)]
    runs = [[oracle_run(o, img, mean, norm) for img in conv] for mean, norm in SETTINGS]
    o.close()
    return planes, specs, runs


def batch_of(pool, n):
    planes, specs, runs = pool
    order = [(3 * f + f // 5) % len(planes) for f in range(n)]
    return order, Nv12Frames([planes[k] for k in order], [specs[k] for k in order])


def test_test_bmp_through_nv12_still_has_its_boxes(pool):
    """the pool is not vacuous: test.bmp taken to NV12 and back through matrix 0 gives 20 candidates and three boxes of classes 18, 0, 16
    under the reference's own mean / norm, as the original picture does"""
    run = pool[2][0][0]
    assert run["cand"] == 20 and [int(b["type"]) for b in run["boxes"]] == [18, 0, 16]


@pytest.mark.parametrize("seed", range(3))
def test_staged_input_tensor_bit_identical(F, net, orc, seed):
    """batches 1-5 (below k_front's threshold: the staged path): read_layer(-1) of every frame is bit for bit the oracle's net_input of
    the numpy-converted picture.  Random bytes: a quarter to two fifths of the pixels clamp in some channel."""
    import torch
    rng = np.random.default_rng(9300 + seed)
    o = orc.Oracle()
    seen, count = set(), 0
    for case in range(6):
        B = int(rng.integers(1, 6))
        specs = []

        def spec(w, h, shared=None):
            nonlocal count
            cw = 2 * ((w + 1) // 2)
            matrix = count % 4 if count < 4 else int(rng.integers(0, 4))      # all four occur, whatever the draws
            count += 1
            seen.add(matrix)
            return (w, h, int(rng.choice([0, w, w + 5, align4(w) + 64])), int(rng.choice([0, cw, cw + 2, align4(cw) + 64])), int(rng.integers(0, 4)),
                    str(rng.choice(["null", "explicit"])), bool(rng.random() < 0.5) if shared is None else shared, matrix)
        for _ in range(B):
            w = int(rng.choice([1, 2, 3, 7, 160, 319, 320, 321, 641, 1000, int(rng.integers(1, 900))]))
            h = int(rng.choice([1, 2, 3, 7, 160, 319, 320, 321, 641, 1000, int(rng.integers(1, 700))]))
            specs.append(spec(w, h))
        if case == 0:
            specs[0] = (320, 320, 0, 0, 0, "null", False, specs[0][7])      # unresized, dword aligned planes: the wide loads
            if B > 1:
                specs[1] = (320, 320, 322, 326, 1, "explicit", True, specs[1][7])      # unresized, misaligned planes: a byte and a pair per pixel
            specs.append((320, 320, 320, 322, 0, "null", False, count % 4))            # unresized, aligned Y rows, chroma rows at 2 mod 4: dword Y, two 16-bit pairs
            B += 1
        if case == 1:                                               # degenerate letterboxes: sw == 0 (1 x 1000) and sh == 0 (1000 x 1)
            specs[0] = spec(1, 1000, False)
            specs.append(spec(1000, 1, True))
            B += 1
        planes = [rand_planes(rng, s[0], s[1]) for s in specs]
        mean = tuple(float(v) for v in rng.uniform(0, 128, 3))
        norm = tuple(float(v) for v in rng.uniform(0.002, 0.02, 3))
        fr = Nv12Frames(planes, specs)
        with net.executor(B, F.FFGPU.KEEP_ALL) as ex:
            ex.forward_nv12_frames_dev(fr.desc, mean, norm)
            torch.cuda.synchronize()
            for f in range(B):
                w, h = specs[f][:2]
                o.set_input_image(np.ascontiguousarray(pack_bgr(fr.bgr[f])), w, h, mean, norm)
                assert np.array_equal(ex.read_layer(-1, f), np.array(o.input)), "case %d frame %d: %s" % (case, f, specs[f])
    o.close()
    assert seen == {0, 1, 2, 3}


def test_tensor_pairs_and_default_matrix(F, net, orc):
    """(Y, UV) pairs of uint8 device tensors, strided rows included, and the call's `matrix` for frames that name none"""
    import torch
    rng = np.random.default_rng(41)
    sizes = [(320, 320), (333, 201), (64, 97)]
    planes = [rand_planes(rng, w, h) for w, h in sizes]
    mean, norm = SETTING
    pairs = []
    for k, (Y, UV) in enumerate(planes):
        ty, tuv = torch.from_numpy(Y).cuda(), torch.from_numpy(UV).cuda()
        if k == 1:                                                  # rows of a wider surface
            wide_y = torch.zeros((Y.shape[0], Y.shape[1] + 31), dtype=torch.uint8, device="cuda")
            wide_uv = torch.zeros((UV.shape[0], UV.shape[1] + 10), dtype=torch.uint8, device="cuda")
            wide_y[:, :Y.shape[1]] = ty
            wide_uv[:, :UV.shape[1]] = tuv
            ty, tuv = wide_y[:, :Y.shape[1]], wide_uv[:, :UV.shape[1]]
        pairs.append((ty, tuv))
    o = orc.Oracle()
    with net.executor(3, F.FFGPU.KEEP_ALL) as ex:
        ex.forward_nv12_frames_dev(pairs, mean, norm, matrix=F.YUV_BT709_FULL)
        torch.cuda.synchronize()
        for f, ((w, h), (Y, UV)) in enumerate(zip(sizes, planes)):
            o.set_input_image(np.ascontiguousarray(pack_bgr(nv12_to_bgr(Y, UV, w, h, 3))), w, h, mean, norm)
            assert np.array_equal(ex.read_layer(-1, f), np.array(o.input)), "frame %d" % f
    o.close()


@pytest.mark.parametrize("batch,flags,setting", [(16, 64, 0), (37, 64, 1), (64, 64, 0), (32, 32, 1)])
def test_fused_against_oracle_staged_and_bgr(F, net, pool, batch, flags, setting, monkeypatch):
    """mixed batches on plans that start with k_front, the NV12 form of it asked for (FFGPU_NV12_FRONT=1) and seen to run (one graph
    captured by the first call; no fp32 input tensor to read afterwards): every materialised layer, the candidate count and the boxes of
    every frame against the oracle's run of that frame's converted picture alone; the staged path (FFGPU_NO_U8_FRONT) gives the same layer
    hashes and record bytes; so does forward_bgr_frames_dev on the pictures converted on the host, on an executor of the same plan.
    (FFGPU_SPLIT2 excludes FFGPU_KEEP_ALL: that leg compares candidate counts, boxes and record bytes, no layers.)"""
    import torch
    monkeypatch.setenv("FFGPU_NV12_FRONT", "1")
    order, fr = batch_of(pool, batch)
    runs = pool[2][setting]
    mean, norm = SETTINGS[setting]
    keep = F.FFGPU.KEEP_ALL if not flags & F.FFGPU.SPLIT2 else 0
    with net.executor(batch, keep | flags) as ex:
        c0 = ex.graph_captures
        ex.forward_nv12_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        assert ex.graph_captures == c0 + 1, "the NV12 form of the first kernel did not run"
        if keep:
            with pytest.raises(RuntimeError, match="no fp32 input tensor exists"):
                ex.read_layer(-1, 0)
        dets = ex.read_dets()
        hashes = list(ex.hash_layers()) if keep else []
        mat = [i for i, hv in enumerate(hashes) if hv]
        assert not keep or len(mat) > 20
        for f in range(batch):
            want = runs[order[f]]
            for i in mat:
                close(ex.read_layer(i, f), want["acts"][i], "batch %d frame %d layer %d" % (batch, f, i))
            assert dets[f]["ncand"] == want["cand"], "frame %d" % f
            boxes_match(ex.boxes(f, dets), want["boxes"], "batch %d frame %d" % (batch, f))
        fused = dets.tobytes()
        monkeypatch.setenv("FFGPU_NO_U8_FRONT", "1")
        ex.forward_nv12_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        assert ex.read_dets().tobytes() == fused, "staged path: records differ"
        if keep:
            assert list(ex.hash_layers()) == hashes, "staged path: layers differ"
            for f in range(batch):
                assert np.array_equal(ex.read_layer(-1, f), runs[order[f]]["input"]), "staged input frame %d" % f
        monkeypatch.delenv("FFGPU_NO_U8_FRONT")
    bg = BgrFrames(fr.bgr)
    with net.executor(batch, keep | flags) as ex:
        ex.forward_bgr_frames_dev(bg.desc, mean, norm)
        torch.cuda.synchronize()
        assert ex.read_dets().tobytes() == fused, "forward_bgr_frames_dev on the converted pictures: records differ"
        if keep:
            assert list(ex.hash_layers()) == hashes, "forward_bgr_frames_dev on the converted pictures: layers differ"


def shared_pictures(test_image, B):
    """B buffers that are one picture as a BGR frame and ANOTHER as an NV12 frame with the same pointer, w, h and pitch: rows of pitch
    ALIGN(3 w, 4); the first w bytes of a row are the NV12 frame's Y row, the chroma plane follows the rows (uv NULL).  Even frames hold a
    real picture as BGR (their NV12 reading is whatever those bytes give), odd frames a real picture as NV12 (their BGR reading likewise)."""
    import torch
    bgr, w, h = test_image
    src = np.frombuffer(bgr, np.uint8).reshape(h, align4(3 * w))[:, :3 * w].reshape(h, w, 3)
    rng = np.random.default_rng(3)
    keep, bdesc, ndesc, bimg, nimg = [], [], [], [], []
    for f in range(B):
        fw, fh = [(640, 424), (320, 320), (400, 300), (321, 211)][f % 4]
        x0, y0 = (7 * f) % (w - fw + 1), (5 * f) % (h - fh + 1)
        pic = np.ascontiguousarray(src[y0:y0 + fh, x0:x0 + fw])
        pitch, cw, ch = align4(3 * fw), 2 * ((fw + 1) // 2), (fh + 1) // 2
        rows = rng.integers(0, 256, (fh, pitch), dtype=np.uint8)
        if f % 2 == 0:
            rows[:, :3 * fw] = pic.reshape(fh, 3 * fw)
            UV = rng.integers(96, 160, (ch, cw), dtype=np.uint8)
        else:
            Y, UV = bgr_to_nv12(pic)
            rows[:, :fw] = Y
        buf = torch.from_numpy(np.concatenate([rows.reshape(-1), UV.reshape(-1), np.zeros(8, np.uint8)])).cuda()      # (pitch h is even: uv = y + pitch h is legal)
        keep.append(buf)
        bdesc.append((buf.data_ptr(), fw, fh, pitch))
        ndesc.append((buf.data_ptr(), 0, fw, fh, pitch, 0, f % 4))
        bimg.append(np.ascontiguousarray(rows[:, :3 * fw].reshape(fh, fw, 3)))
        nimg.append(nv12_to_bgr(rows, UV, fw, fh, f % 4))
    return keep, bdesc, ndesc, bimg, nimg


@pytest.mark.parametrize("fused", [True, False])
def test_alternating_with_bgr_frames_ring_and_captures(F, net, orc, test_image, fused, monkeypatch):
    """forward_bgr_frames_dev and forward_nv12_frames_dev in turn on one executor and one stream, no host sync, a 4-slot ring, the two
    calls reading different pictures through descriptors with the same pointers, sizes and pitches: every slot holds its own call's
    records (the "table already sent" shortcut never takes one kind of table for the other).  Captures: the first NV12 call of a fresh
    executor captures exactly one graph on the fused route and none on the staged one; so does the first BGR call, as its own test
    says; 50 further alternating calls capture nothing."""
    import torch
    if fused:
        monkeypatch.setenv("FFGPU_NV12_FRONT", "1")
    else:
        monkeypatch.setenv("FFGPU_NO_U8_FRONT", "1")
    B = 16
    mean, norm = DEFAULT
    keep, bdesc, ndesc, bimg, nimg = shared_pictures(test_image, B)
    o = orc.Oracle()
    with net.executor(B, F.FFGPU.CONCURRENT) as ex:
        ex.forward_bgr_frames_dev(bdesc, mean, norm)
        torch.cuda.synchronize()
        want_b = ex.read_dets()
        ex.forward_nv12_frames_dev(ndesc, mean, norm)
        torch.cuda.synchronize()
        want_n = ex.read_dets()
        assert want_b.tobytes() != want_n.tobytes()                 # different pictures, different records
        for f in range(B):                                          # ... and both are the right ones
            boxes_match(ex.boxes(f, want_b), oracle_run(o, bimg[f], mean, norm)["boxes"], "bgr frame %d" % f)
            boxes_match(ex.boxes(f, want_n), oracle_run(o, nimg[f], mean, norm)["boxes"], "nv12 frame %d" % f)
        assert sum(int(want_b[f]["count"]) for f in range(0, B, 2)) > 0 and sum(int(want_n[f]["count"]) for f in range(1, B, 2)) > 0
        ring = torch.zeros(4 * B * F.DETS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        ex.set_ring(ring.data_ptr(), 4)
        st = torch.cuda.Stream()
        caps = ex.graph_captures
        for k in range(4):
            if k % 2 == 0:
                ex.forward_bgr_frames_dev(bdesc, mean, norm, stream=st.cuda_stream)
            else:
                ex.forward_nv12_frames_dev(ndesc, mean, norm, stream=st.cuda_stream)
        st.synchronize()
        got = np.frombuffer(ring.cpu().numpy().tobytes(), F.DETS_DTYPE).reshape(4, B)
        for k in range(4):
            assert got[k].tobytes() == (want_b if k % 2 == 0 else want_n).tobytes(), "slot %d" % k
        assert ex.graph_captures == caps
        ex.set_ring(None, 0)
    o.close()
    with net.executor(B, F.FFGPU.CONCURRENT) as ex:
        c0 = ex.graph_captures
        ex.forward_nv12_frames_dev(ndesc, mean, norm)
        c1 = ex.graph_captures
        assert c1 == c0 + (1 if fused else 0)
        ex.forward_bgr_frames_dev(bdesc, mean, norm)
        c2 = ex.graph_captures
        assert c2 == c1 + (1 if fused else 0)
        for k in range(50):
            if k % 2 == 0:
                ex.forward_nv12_frames_dev(ndesc, mean, norm)
            else:
                ex.forward_bgr_frames_dev(bdesc, mean, norm)
        torch.cuda.synchronize()
        assert ex.graph_captures == c2
        assert ex.read_dets().tobytes() == want_b.tobytes()


def test_four_columns_per_lane_plans_stage(F, net, pool, monkeypatch):
    """a plan whose first kernel runs four columns per lane (FFGPU_FRONT_NC=4): no resizing form exists there, so NV12 frames take the
    staged path -- no capture, the fp32 batch readable and bit-exact, every layer and box against the oracle"""
    import torch
    monkeypatch.setenv("FFGPU_FRONT_NC", "4")
    B = 16
    order, fr = batch_of(pool, B)
    runs = pool[2][0]
    mean, norm = DEFAULT
    with net.executor(B, F.FFGPU.KEEP_ALL) as ex:
        c0 = ex.graph_captures
        ex.forward_nv12_frames_dev(fr.desc, mean, norm)
        torch.cuda.synchronize()
        dets = ex.read_dets()
        assert ex.graph_captures == c0
        mat = [i for i, hv in enumerate(ex.hash_layers()) if hv]
        assert len(mat) > 20
        for f in range(B):
            want = runs[order[f]]
            assert np.array_equal(ex.read_layer(-1, f), want["input"]), "input frame %d" % f
            for i in mat:
                close(ex.read_layer(i, f), want["acts"][i], "NC 4 frame %d layer %d" % (f, i))
            assert dets[f]["ncand"] == want["cand"], "frame %d" % f
            boxes_match(ex.boxes(f, dets), want["boxes"], "NC 4 frame %d" % f)


def test_tiny3_staged_only(F, orc, tmp_path):
    """tests/data/tiny3.cfg (96 x 64, no k_front) with seeded random weights: mixed NV12 sizes through the staged path, the input bit for
    bit, every layer and every box against the oracle"""
    import torch
    from conftest import ROOT
    cfg = os.path.join(ROOT, "tests", "data", "tiny3.cfg")
    o = orc.Oracle(cfg=cfg, weights=None)
    wpath = str(tmp_path / "tiny3.weights")
    _write_random_weights(wpath, o, 7)
    o.close()
    o = orc.Oracle(cfg=cfg, weights=wpath)
    rng = np.random.default_rng(13)
    specs = [(96, 64, 0, 0, 0, "null", False, 0), (200, 90, 203, 0, 1, "explicit", True, 1), (50, 120, 0, 54, 3, "null", True, 2),
             (97, 63, 0, 0, 2, "explicit", False, 3), (3, 400, 10, 8, 1, "null", False, 0)]
    planes = [rand_planes(rng, s[0], s[1]) for s in specs]
    fr = Nv12Frames(planes, specs)
    mean, norm = (10.0, 20.0, 30.0), (0.01, 0.012, 0.011)
    with F.Net(cfg, wpath) as n:
        with n.executor(len(specs), F.FFGPU.KEEP_ALL | F.FFGPU.NO_FUSE) as ex:
            c0 = ex.graph_captures
            ex.forward_nv12_frames_dev(fr.desc, mean, norm)
            torch.cuda.synchronize()
            assert ex.graph_captures == c0
            dets = ex.read_dets()
            for f, s in enumerate(specs):
                o.set_input_image(np.ascontiguousarray(pack_bgr(fr.bgr[f])), s[0], s[1], mean, norm)
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
    """every rejection: < 0 with the frame's index in the message; the next valid call on the same executor gives the records of a
    fresh executor"""
    import ctypes as C
    import torch
    B = 16
    order, fr = batch_of(pool, B)
    mean, norm = SETTING
    L = F.lib()
    good = list(fr.desc)
    with net.executor(B, 0) as ex:
        ex.forward_nv12_frames_dev(good, mean, norm)
        torch.cuda.synchronize()
        fresh = ex.read_dets().tobytes()
    k = 5
    y, uv, w, h, py, pu, mx = good[k]
    assert order[k] == 0 and w == 640 and uv == 0 and py == 0 and pu == 0      # (test.bmp: one contiguous surface, minimal pitches)
    explicit_uv = y + w * h
    bad = [((0, uv, w, h, py, pu, mx), "NULL y"), ((y, uv, 0, h, py, pu, mx), "bad size"), ((y, uv, w, -2, py, pu, mx), "bad size"),
           ((y, uv, w, h, w - 1, pu, mx), "pitch_y"), ((y, uv, w, h, py, w - 2, mx), "pitch_uv"), ((y, uv, w, h, py, w + 1, mx), "pitch_uv"),
           ((y, explicit_uv + 1, w, h, py, pu, mx), "odd"), ((y, uv, w, h, py, pu, -1), "matrix"), ((y, uv, w, h, py, pu, 4), "matrix")]
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*norm)
    with net.executor(B, 0) as ex:
        for d, msg in bad:
            arr = (F.Nv12Frame * B)(*[F.Nv12Frame(*F.nv12_frame_desc(g)) for g in good[:k] + [d] + good[k + 1:]])
            assert L.ffgpu_exec_forward_nv12_frames_dev(ex.h, arr, B, m, s, None) < 0, d
            err = F.last_error()
            assert "frame %d:" % k in err and msg in err, (d, err)
        arr = (F.Nv12Frame * B)(*[F.Nv12Frame(*F.nv12_frame_desc(g)) for g in good])
        arr[7].reserved = 1
        assert L.ffgpu_exec_forward_nv12_frames_dev(ex.h, arr, B, m, s, None) < 0 and "frame 7:" in F.last_error() and "reserved" in F.last_error()
        arr[7].reserved = 0
        assert L.ffgpu_exec_forward_nv12_frames_dev(ex.h, arr, B - 1, m, s, None) < 0 and "frames for an executor of batch" in F.last_error()
        assert L.ffgpu_exec_forward_nv12_frames_dev(ex.h, arr, B, None, s, None) < 0 and "NULL" in F.last_error()
        assert L.ffgpu_exec_forward_nv12_frames_dev(ex.h, arr, B, m, None, None) < 0 and "NULL" in F.last_error()
        assert L.ffgpu_exec_forward_nv12_frames_dev(ex.h, None, B, m, s, None) < 0 and "NULL" in F.last_error()
        with pytest.raises(RuntimeError, match="frame 5: NULL y"):
            ex.forward_nv12_frames_dev(good[:k] + [bad[0][0]] + good[k + 1:], mean, norm)
        ex.forward_nv12_frames_dev(good, mean, norm)
        torch.cuda.synchronize()
        assert ex.read_dets().tobytes() == fresh
