"""k_yolo and k_nms held to EQUALITY with the oracle: candidates (count, order, all six fields), the full list of survivors and the whole
fixed-size records, byte for byte, with no tolerance anywhere and no element skipped.

The vehicle (tests/detect_tail/heads.py): [dropout], [upsample] stride=1, [yolo] on channels = 3 * (5 + classes), so the frames ARE the head
tensor; every test first asserts that the executor's copy of it (read_layer of the upsample) equals the frames byte for byte.  Expected
candidates are orc.yolo on the executor's own copy of each head's input; expected boxes are orc.nms of them where the scores are pairwise
distinct and heads.nms_ordered (pinned to orc.nms by tests/test_detect_tail_ref.py) where they tie.  Every case runs on an FFGPU_KEEP_ALL executor
and on a default one (fused plan, HIP graph), twice each: the second forward must give the same bytes.

read_candidates (read_layer -2) is not cut at NET.bbox_max -- ncand and the candidate buffer hold every decoded candidate, the first bbox_max of
them in emission order go into NMS (include/ffcnn_hip.h) -- so it is compared with the uncut list, and its first bbox_max with the cut one.

The one thing bytes cannot settle is WHICH NaN a NaN coordinate is (NaN in tx ty tw th): IEEE 754 leaves the sign and payload of an arithmetic
result to the implementation, and the reference's own depend on its compiler (x86 hands the operand on; gfx950 returned x1 = 0xffc00000 beside
x2 = 0x7fc00000 for one NaN centre).  heads.one_nan maps every NaN coordinate to one NaN on both sides before the bytes are compared: which
fields are NaN, and every other bit, must still agree (include/ffcnn_hip.h states this).

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import numpy as np
import pytest

from detect_tail import heads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import ffcnn_amd  # noqa: F401
    from ffcnn_amd import capi
    capi.lib()
    return capi


def first_diff(got, want):
    if len(got) != len(want):
        return "%d boxes, expected %d" % (len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        if g.tobytes() != w.tobytes():
            return "box %d of %d: %s (%s), expected %s (%s)" % (n, len(got), g, g.tobytes().hex(), w, w.tobytes().hex())
    return None


def same_boxes(got, want, what):
    got, want = heads.one_nan(got), heads.one_nan(want)
    assert got.tobytes() == want.tobytes(), "%s: %s" % (what, first_diff(got, want))


def same_record(got, want, what):
    got, want = got.copy(), want.copy()
    got["box"], want["box"] = heads.one_nan(got["box"]), heads.one_nan(want["box"])
    if got.tobytes() != want.tobytes():
        head = {k: (int(got[k]), int(want[k])) for k in ("count", "ncand", "overflow", "nfull") if got[k] != want[k]}
        pytest.fail("%s: record differs: %s %s" % (what, head or "", first_diff(got["box"], want["box"])), pytrace=False)


def compare(ex, wants, bbox_max, what):
    dets = ex.read_dets()
    for f, w in enumerate(wants):
        cand = ex.read_candidates(f)
        same_boxes(cand, w.full, "%s, frame %d, candidates" % (what, f))
        same_boxes(cand[:bbox_max], w.cut, "%s, frame %d, candidates that enter NMS" % (what, f))
        same_boxes(ex.read_boxes(f), w.boxes, "%s, frame %d, boxes" % (what, f))
        same_record(dets[f], w.record, "%s, frame %d" % (what, f))


def load(F, tmp_path, case):
    cfg, wts = str(tmp_path / (case.name + ".cfg")), str(tmp_path / (case.name + ".weights"))
    with open(cfg, "w") as fp:
        fp.write(case.cfg_text())
    with open(wts, "wb") as fp:
        fp.write(np.array([0, 2, 5], "<i4").tobytes() + np.array([0], "<u8").tobytes())       # a darknet header and no weights: no conv layer
    net = F.Net(cfg, wts)
    assert net.layer_num == case.nlayers and net.input_shape == case.shape[1:]
    for h in case.heads:                                      # the head's parameters as the executor has them
        L = net.layer(h.layer)
        assert (L.w, L.h, L.class_num) == (h.w, h.h, h.classes) and tuple(tuple(a) for a in L.anchor_list) == h.anchors
        assert np.float32(L.ignore_thres).tobytes() == h.thresh.tobytes() and np.float32(L.scale_x_y).tobytes() == h.scale.tobytes()
    return net


def frames_reach_the_head(ex, case, frames):
    for f in range(case.batch):
        assert ex.read_layer(1, f).tobytes() == np.ascontiguousarray(frames[f], np.float32).tobytes(), "frame %d: the staged copy differs from the frames" % f


def run(F, orc, tmp_path, case, frames, bbox_max=None, scale=(1, 1), plans=None):
    """both executors, two forwards each; returns the expected results (heads.Want per frame)"""
    wants = None
    with load(F, tmp_path, case) as net:
        if bbox_max is not None:
            net.n.bbox_max = bbox_max
        bm = net.n.bbox_max
        for plan, flags in plans or (("keep_all", F.FFGPU.KEEP_ALL), ("default", 0)):
            with net.executor(case.batch, flags) as ex:
                assert ex.cand_capacity == case.slots
                ex.set_scale(*scale)
                for rep in range(2):
                    ex.forward_host(frames)
                    if wants is None:
                        frames_reach_the_head(ex, case, frames)
                        wants = heads.expected(orc, case, ex.read_layer, bm, *scale)
                    compare(ex, wants, bm, "%s, %s plan, forward %d" % (case.name, plan, rep))
    return wants


# ---------------------------------------------------------------------------------------------------------------- 1. decode: class scan
@pytest.mark.parametrize("classes", [1, 2, 63, 64, 65, 80, 129])
@pytest.mark.parametrize("head", ["10x10 batch 3", "1x1 batch 5, even specs", "1x1 batch 5, odd specs"])
def test_decode_class_scan(F, orc, tmp_path, classes, head):
    """300 threads per frame: waves straddle anchors and frames, the last wave is partial; 1 x 1 at batch 5: a launch of 15 lanes.  Planted on
    random logits (heads.plant_specs): the maximum at class 0 / 1 / 62 / 63 / 64 / last, ties across trips of the wave scan (the first wins),
    +0 against -0, +inf, all -inf, NaN above class 0 (skipped), NaN at class 0 (no candidate), NaN objectness, NaN / +-inf in tx ty tw th"""
    if head.startswith("10x10"):
        case, part = heads.single("scan_c%d" % classes, 10, 10, classes, 3, ".25"), None
    else:
        case, part = heads.single("scan1_c%d" % classes, 1, 1, classes, 5, ".25"), 0 if "even" in head else 1
    frames, plants = heads.decode_scan(case, 100 + classes, part)
    wants = run(F, orc, tmp_path, case, frames)
    heads.check_plants(orc, case, frames, plants, [w.full for w in wants])


# ------------------------------------------------------------------------------------------------------------ 2. decode: threshold edge
@pytest.mark.parametrize("thresh", heads.THRESHOLDS)
def test_decode_threshold_edge(F, orc, tmp_path, thresh):
    """objectness on the 129 floats around logit(thresh) with the class logit at +50 (conf equals the bound of the kernel's early-out) and at 0,
    one anchor at +20: the kernel emits exactly the oracle's set.  That the walks straddle is asserted in tests/test_detect_tail_ref.py and,
    for this threshold's walk, here"""
    case = heads.threshold_case(thresh)
    frames, where = heads.threshold_edge(case)
    wants = run(F, orc, tmp_path, case, frames)
    ok = heads.edge_passes(orc, case, frames, where)
    if thresh in (".01", ".25", ".9"):
        assert 0 < sum(o for o, w in zip(ok, where) if w[0] == 0) < 129
    assert len(wants[1].full) >= 1


# ----------------------------------------------------------------------------------------------------------------- 3. decode: geometry
def test_decode_pooled_head(F, orc, tmp_path):
    """a 7 x 5 head on a 56 x 40 net, scale_x_y 1.05, anchors of its own"""
    case = heads.pooled()
    wants = run(F, orc, tmp_path, case, heads.gauss(case, 21, sigma=16.0))          # (sigma 2 behind the 8 x 8 average)
    assert all(10 < len(w.full) < case.slots for w in wants)


@pytest.mark.parametrize("branch", ["0", "1"])
def test_decode_two_heads(F, orc, tmp_path, monkeypatch, branch):
    """two heads of different sizes, parameters and thresholds: key_base, emission order across heads, two kernels counting into one ncand;
    FFGPU_BRANCH=1: the first head runs on the planner's side lane, beside the pool and the second head"""
    monkeypatch.setenv("FFGPU_BRANCH", branch)
    case = heads.two_heads()
    frames = heads.gauss(case, 21)
    wants = run(F, orc, tmp_path, case, frames)
    for f, w in enumerate(wants):                              # both heads contribute (the frames are the first head's input)
        assert 10 < len(heads.decode(orc, case, case.heads[0], frames[f])) < len(w.full) - 3


# ---------------------------------------------------------------------------------------------------------------- 4. NMS: many candidates
@pytest.mark.parametrize("name,w,h,batch,seed", heads.MANY, ids=[m[0] for m in heads.MANY])
def test_nms_many_candidates(F, orc, tmp_path, name, w, h, batch, seed):
    """threshold 0 and Gaussian logits: every anchor is a candidate, hundreds survive.  20 x 20: the ordinary LDS case, on a seed whose lists
    are free of ties (plain orc.nms); 8190 slots: the largest LDS case; 8193: the smallest that takes the global scratch, natural ties in both"""
    case = heads.many_case(w, h, batch)
    assert (case.slots > heads.NMS_LDS_CAP) == (name == "scratch")
    wants = run(F, orc, tmp_path, case, heads.gauss(case, seed))
    assert all(len(x.full) == case.slots and x.record["overflow"] & 4 for x in wants[:1])
    if (w, h, batch, seed) == heads.TIE_FREE:
        assert all(x.plain for x in wants)
    else:
        assert not all(x.plain for x in wants) and max(len(x.boxes) for x in wants) > 500


# ---------------------------------------------------------------------------------------------------------------------- 5. NMS: bbox_max
@pytest.mark.parametrize("bbox_max", [1, 700, -1, 0], ids=["1", "700", "capacity - 1", "capacity"])
@pytest.mark.parametrize("head", ["20x20", "scratch"])
def test_nms_bbox_max(F, orc, tmp_path, head, bbox_max):
    """NET.bbox_max below, one below and at the number of candidates: the first bbox_max in emission order enter NMS (the sort on the emission
    key), overflow bit 0 says so"""
    w, h = (20, 20) if head == "20x20" else heads.SCRATCH_HEAD
    case = heads.many_case(w, h, 2)
    bm = case.slots + bbox_max if bbox_max <= 0 else bbox_max
    wants = run(F, orc, tmp_path, case, heads.gauss(case, 2), bbox_max=bm)
    for x in wants:
        assert len(x.full) == case.slots and len(x.cut) == bm and (x.record["overflow"] & 1) == (bm < case.slots)


# ------------------------------------------------------------------------------------------------------------------- 6. NMS: record size
@pytest.mark.parametrize("K", heads.RECORD_KS)
def test_nms_record_size(F, orc, tmp_path, K):
    case = heads.record_case(2)
    wants = run(F, orc, tmp_path, case, heads.record_frames(case, (K, K)))
    for x in wants:
        assert (x.record["count"], x.record["nfull"], x.record["overflow"]) == (min(K, 128), K, 4 if K > 128 else 0)


def device_bytes(ptr, nbytes):
    import torch

    class Mem:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(Mem(), device="cuda").cpu().numpy().tobytes()


@pytest.mark.parametrize("keep_all", [True, False])
def test_nms_records_shrink_and_grow(F, orc, tmp_path, keep_all):
    """ONE executor with a host mirror and a ring of three slots pre-filled with 0xA5: 129, 2, 0, 128 boxes per frame in sequence, then frames of
    129 / 0 / 5, with set_scale in between.  After every forward the device records, the host mirror and the forward's ring slot equal the
    expected records in full -- the zeroed tail of a record that shrank included (k_nms writes only the slots that change)"""
    import torch
    case = heads.record_case(3)
    seq = [((129, 129, 129), (1, 1)), ((2, 2, 2), (3, 2)), ((0, 0, 0), (3, 2)), ((128, 128, 128), (1, 1)), ((129, 0, 5), (7, 5)), ((1, 129, 0), (7, 5))]
    with load(F, tmp_path, case) as net:
        bm = net.n.bbox_max
        wants = []
        with net.executor(3, F.FFGPU.KEEP_ALL) as ex:            # the expected records, from this executor's copy of the head tensors
            for ks, scale in seq:
                frames = heads.record_frames(case, ks)
                ex.set_scale(*scale)
                ex.forward_host(frames)
                frames_reach_the_head(ex, case, frames)
                wants.append((frames, heads.expected(orc, case, ex.read_layer, bm, *scale)))
                assert [int(x.record["nfull"]) for x in wants[-1][1]] == list(ks)
        with net.executor(3, F.FFGPU.HOST_DETS | (F.FFGPU.KEEP_ALL if keep_all else 0)) as ex:
            nbytes = heads.DETS_DTYPE.itemsize * 3
            ring = torch.full((3, nbytes), 0xA5, dtype=torch.uint8, device="cuda")
            ex.set_ring(ring.data_ptr(), 3)
            d_ptr, d_bytes = ex.dets_dev()
            assert d_bytes == nbytes
            for n, ((ks, scale), (frames, want)) in enumerate(zip(seq, wants)):
                ex.set_scale(*scale)
                ex.forward_host(frames)
                what = "forward %d (%s boxes)" % (n, ks)
                compare(ex, want, bm, what)
                rec = np.array([x.record for x in want], heads.DETS_DTYPE).tobytes()
                assert ex.dets_host().tobytes() == rec, what + ": host mirror"
                assert device_bytes(d_ptr, nbytes) == rec, what + ": device records"
                slots = ring.cpu().numpy()
                assert slots[n % 3].tobytes() == rec, what + ": ring slot"
                for other in range(3):
                    if other != n % 3:
                        prev = max([m for m in range(n) if m % 3 == other], default=None)
                        assert slots[other].tobytes() == (b"\xa5" * nbytes if prev is None else np.array([x.record for x in wants[prev][1]], heads.DETS_DTYPE).tobytes())


# --------------------------------------------------------------------------------------------------------------------- 7. zero scores
def test_zero_scores(F, orc, tmp_path):
    """threshold 0: candidates of score exactly 0 (objectness -100; every class at -inf, which is class 0) count in ncand and in the candidate
    list; the reference's NMS treats score 0 as dead, so no list and no record contains them although nothing suppresses them"""
    case = heads.zero_case()
    frames, where = heads.zero_frames(case)
    wants = run(F, orc, tmp_path, case, frames)
    for x in wants:
        assert (x.full["score"] == 0).sum() == 6 and x.record["ncand"] == case.slots and not (x.boxes["score"] == 0).any()
    for f, k, i, j, cls in where:
        one = heads.cell_candidate(orc, case, case.heads[0], frames[f], k, i, j)
        assert len(one) == 1 and one[0]["score"] == 0 and one[0]["type"] == cls
