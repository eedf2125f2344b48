"""Flow maps on the device: ffgpu_flow_update_bgr_dev / _nv12_dev, ffgpu_flow_reset_dev, ffgpu_flow_boxes_dev and ffgpu_exec_flow_boxes against
tests/flow/flowref.py, the numpy restatement of the contract in include/ffcnn_hip.h: the whole state, the rows and the words, byte for byte.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import os

import numpy as np
import pytest

from flow import flowref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def c_spec(F, sp):
    return F.flow_spec(sp.w, sp.h, sp.block_log2, sp.range, sp.min_spread, float(sp.min_score), sp.classes)


def texture(seed, sp, shifts):
    """one random texture seen through a window that moves: frame n's content is frame 0's moved by shifts[n]"""
    r, tex = sp.range, np.random.default_rng(seed).integers(0, 256, (sp.h + 2 * sp.range, sp.w + 2 * sp.range))
    return [tex[r - vy:r - vy + sp.h, r - vx:r - vx + sp.w] for vx, vy in shifts]


def on_device(F, sp, lumas, streams, state, nstreams, cuts=(), bgr=None, reset=None):
    """the frames (NV12 with a pitch of w + 3, or the BGR images at an odd address with an odd pitch) through the update, as one call or cut into
    several; returns the state's bytes and the rows"""
    import torch
    w, h, n = sp.w, sp.h, len(streams)
    d_state = torch.from_numpy(state.raw.reshape(-1).copy()).cuda()
    d_rows = torch.full((64 * n,), 0xA5, dtype=torch.uint8, device="cuda")
    if reset is not None:
        F.flow_reset_dev(d_state.data_ptr(), nstreams, w, h, sp.block_log2, reset)
    keep, descs = [], []
    for t in range(n):
        if lumas[t] is None:
            descs.append(None)
        elif bgr is None:
            py, uvoff = w + 3, (h * (w + 3) + 1) & ~1
            buf = np.full(uvoff + (h + 1) // 2 * (w + 1), 0x5A, np.uint8)
            buf[:h * py].reshape(h, py)[:, :w] = lumas[t]
            keep.append(torch.from_numpy(buf).cuda())
            descs.append((keep[-1].data_ptr(), keep[-1].data_ptr() + uvoff, w, h, py, 2 * ((w + 1) // 2)))
        else:
            pitch = 3 * w + 1 + (w & 1)
            buf = np.full(1 + h * pitch, 0x5A, np.uint8)
            buf[1:].reshape(h, pitch)[:, :3 * w] = bgr[t].reshape(h, 3 * w)
            keep.append(torch.from_numpy(buf).cuda())
            descs.append((keep[-1].data_ptr() + 1, w, h, pitch))
    edges = [0] + list(cuts) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        (F.flow_update_nv12_dev if bgr is None else F.flow_update_bgr_dev)(descs[a:b], streams[a:b], c_spec(F, sp), d_state.data_ptr(), nstreams, d_rows.data_ptr() + 64 * a)
    torch.cuda.synchronize()
    return d_state.cpu().numpy(), d_rows.cpu().numpy().view(np.int32).reshape(n, 16)


def check(F, sp, lumas, streams, nstreams=1, state=None, **kw):
    """device against reference from the same first state; returns the reference's state afterwards"""
    state = state or flowref.State(nstreams, sp.w, sp.h, sp.block_log2)
    got, rows = on_device(F, sp, lumas, streams, state, nstreams, **kw)
    if kw.get("reset") is not None:
        state.raw[:] = 0
    want = flowref.update(lumas, streams, sp, state)
    assert rows.tobytes() == want.tobytes(), (rows[:, :7], want[:, :7])
    bad = np.nonzero(got != state.raw.reshape(-1))[0]
    assert not len(bad), "state: %d bytes differ, first at %d of %d a stream" % (len(bad), bad[0], state.raw.shape[1])
    return state


def garbage(seed, nstreams, sp):
    st = flowref.State(nstreams, sp.w, sp.h, sp.block_log2)
    st.raw[:] = np.random.default_rng(seed).integers(0, 256, st.raw.shape)
    return st


@pytest.mark.parametrize("v", [(0, 0), (1, 0), (3, -2), (-5, 5), (5, -5)])
def test_ground_truth(F, v):
    """a random texture, then the same texture moved by v: every block whose source lies inside the frame holds v at cost 0, and so does the header"""
    sp = flowref.Spec(72, 40, 3, 5)
    st = check(F, sp, texture(1, sp, [(0, 0), v]), [0, 0])
    inside = [(j, i) for j in range(sp.gh) for i in range(sp.gw) if 0 <= 8 * i - v[0] and 8 * i + 8 - v[0] <= 72 and 0 <= 8 * j - v[1] and 8 * j + 8 - v[1] <= 40]
    assert len(inside) >= 24 and all((int(st.recs[0][b]["dx"]), int(st.recs[0][b]["dy"]), int(st.recs[0][b]["cost"])) == v + (0,) for b in inside)
    assert st.hdr[0].tolist()[:3] == [2, v[0], v[1]] and st.hdr[0, 3] >= len(inside)


@pytest.mark.parametrize("w,h,k,r", [(8, 8, 3, 1), (5, 3, 3, 4), (71, 37, 3, 7), (72, 40, 3, 16), (130, 70, 4, 16), (96, 64, 4, 1)])
def test_shapes(F, w, h, k, r):
    """one block; a frame smaller than a block; partial blocks; one block past a 64 x 32 tile under a halo wider than a block; three tiles across with a
    partial last one; the least range: a texture that moves twice, the second frame with noise on it"""
    sp = flowref.Spec(w, h, k, r, min_spread=40)
    a, b, c = texture(w * h, sp, [(0, 0), (min(r, 3), -min(r, 2)), (min(r, 3) - r, 1 - min(r, 2))])
    check(F, sp, [a, np.clip(b + np.random.default_rng(r).integers(-9, 10, b.shape), 0, 255), c], [0, 0, 0])


@pytest.mark.parametrize("case", ["constant", "period 4", "saturated", "min_spread 0"])
def test_ties_and_extremes(F, case):
    rng = np.random.default_rng(7)
    if case == "constant":
        sp = flowref.Spec(40, 24, 3, 6)
        st = check(F, sp, [np.full((24, 40), 77)] * 2, [0, 0])
        assert not st.raw[0, -8 * sp.gw * sp.gh:].any() and st.hdr[0].tolist() == [2, 0, 0, 0]
    elif case == "period 4":                                                            # every row repeats its four values: a move by 4 is no move
        sp = flowref.Spec(64, 32, 3, 6)
        rowpat = np.tile(rng.integers(0, 256, (32, 4)), (1, 16))
        st = check(F, sp, [rowpat, np.roll(rowpat, 4, axis=1)], [0, 0])
        assert not st.recs[0]["dx"].any() and not st.recs[0]["dy"].any() and not st.recs[0]["cost"].any() and st.recs[0]["spread"].all()
    elif case == "saturated":
        sp = flowref.Spec(48, 32, 4, 3)
        st = check(F, sp, [np.zeros((32, 48), int), np.full((32, 48), 255)], [0, 0])
        assert (st.recs[0]["cost"] == 65280).all() and not st.recs[0]["spread"].any()
    else:                                                                               # a flat half: its blocks are reliable under neither spec
        sp0, sp1 = flowref.Spec(64, 32, 3, 2, min_spread=0), flowref.Spec(64, 32, 3, 2, min_spread=1)
        fr = texture(3, sp0, [(0, 0), (1, 1)])
        fr = [np.where(np.arange(64) < 32, 9, f) for f in fr]
        s0, s1 = check(F, sp0, fr, [0, 0]), check(F, sp1, fr, [0, 0])
        assert s0.tobytes() == s1.tobytes() and 0 < s0.hdr[0, 3] < 32


@pytest.mark.parametrize("case", ["reset", "three in one call", "interleaved", "garbage"])
def test_time_and_state(F, case):
    sp = flowref.Spec(71, 37, 3, 4, min_spread=100)
    fr = texture(11, sp, [(0, 0), (2, 1), (2, 2), (-4, 0), (1, -3)])
    if case == "reset":                                                                 # any bytes, reset, the first frame: empty records, plane 0 written
        check(F, sp, fr[:1], [0], 2, garbage(5, 2, sp), reset=-1)
    elif case == "three in one call":
        one = check(F, sp, fr[:3], [0, 0, 0])
        assert check(F, sp, fr[:3], [0, 0, 0], cuts=[1, 2]).tobytes() == one.tobytes() and one.hdr[0, 0] == 3
    elif case == "interleaved":                                                         # two streams, a skipped stream and a NULL frame between them
        check(F, sp, [fr[0], fr[1], fr[0], None, fr[1], fr[2], fr[4]], [0, -1, 2, 0, 0, 2, 2], 3)
    else:                                                                               # frames != 0 and both planes, the records and the padding any bytes
        st = garbage(6, 2, sp)
        assert st.hdr[0, 0] != 0 and st.hdr[1, 0] != 0
        check(F, sp, fr[:3], [1, 0, 1], 2, st)


def test_inputs(F):
    """BGR at an odd address with an odd pitch and NV12 with a pitch that is not w, against the same reference luma"""
    sp = flowref.Spec(71, 37, 4, 3)
    imgs = [np.random.default_rng(s).integers(0, 256, (37, 71, 3), dtype=np.uint8) for s in (1, 2)]
    imgs[1][:, 3:] = imgs[0][:, :-3]
    lumas = [flowref.luma_bgr(i) for i in imgs]
    assert check(F, sp, lumas, [0, 0], bgr=imgs).tobytes() == check(F, sp, lumas, [0, 0]).tobytes()


def record_set(sp, S):
    """boxes inside, straddling each edge, wholly outside, inverted, with a NaN score, of a filtered class, and more than 128 that qualify"""
    rng = np.random.default_rng(35)
    w, h = sp.w, sp.h
    recs, flat = np.zeros(3, flowref.DETS_DTYPE), np.zeros(3 * S, flowref.BOX_DTYPE)
    fixed = [(0, .9, 10.5, 9.5, 40.2, 30.9), (0, .9, -20, 5, 12, 20), (2, .9, w - 9, 3, w + 30, 14), (0, .9, 20, -8, 50, 3), (0, .9, 20, h - 2, 50, h + 40), (0, .9, -50, -50, -1, -1),
             (0, .9, w, 0, w + 5, 5), (0, .9, 30, 10, 20, 20), (0, np.nan, 1, 1, 30, 30), (1, .9, 1, 1, 30, 30), (0, .1, 1, 1, 30, 30), (0, .9, -1e10, -1e10, 1e10, 1e10)]
    flat[:len(fixed)] = fixed
    recs[0]["nfull"] = len(fixed)
    for i in range(140):
        x, y = rng.uniform(-10, w), rng.uniform(-10, h)
        flat[S + i] = (2 * (i % 2), .5, x, y, x + rng.uniform(0, 40), y + rng.uniform(0, 30))
    recs[1]["nfull"], recs[2]["nfull"] = 140, 5
    return recs, flat


@pytest.mark.parametrize("junk", [False, True])
def test_boxes(F, junk):
    """the words against the reference on the state two frames leave, and on a state of any bytes (the sums wrap); the state stays"""
    import torch
    sp, S = flowref.Spec(71, 37, 3, 4, min_spread=100, min_score=0.25, classes=[1, 0, 1]), 144
    st = garbage(9, 2, sp) if junk else flowref.State(2, 71, 37, 3)
    if not junk:
        flowref.update(texture(11, sp, [(0, 0), (2, 1), (0, 0), (-3, 2)]), [0, 0, 1, 1], sp, st)
    recs, flat = record_set(sp, S)
    d_state, d_recs, d_flat = (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (st.raw, recs, flat))
    d_words = torch.full((4 * 3 * (8 + 4 * S),), 0xA5, dtype=torch.uint8, device="cuda")
    F.flow_boxes_dev(d_recs.data_ptr(), d_flat.data_ptr(), S, [1, 0, -1], c_spec(F, sp), d_state.data_ptr(), 2, d_words.data_ptr())
    torch.cuda.synchronize()
    want = flowref.boxes(recs, flat, S, None, [1, 0, -1], sp, st)
    assert d_words.cpu().numpy().tobytes() == want.tobytes() and d_state.cpu().numpy().tobytes() == st.tobytes()
    assert want[0, :3].tolist() == [9, 0, 3] and want[1, :2].tolist() == [128, 12] and not want[2].any() and (junk or want[0, 9] > 0)


def test_exec_flow_boxes(F, net):
    """behind a forward of the golden frame: the picture, then the picture moved by (3, -2)"""
    import torch
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    pic = np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))
    sp = flowref.Spec(w, h, 4, 3, min_spread=200, min_score=0.25)
    frames = [pic, np.roll(pic, (-2, 3), axis=(0, 1))]
    dev = torch.from_numpy(np.stack(frames)).cuda()
    st = flowref.State(1, w, h, 4)
    d_state, d_rows = torch.zeros(st.raw.size, dtype=torch.uint8, device="cuda"), torch.zeros(128, dtype=torch.uint8, device="cuda")
    with net.executor(1) as ex:
        S = ex.cand_capacity
        F.flow_update_bgr_dev([dev[0], dev[1]], [0, 0], c_spec(F, sp), d_state.data_ptr(), 1, d_rows.data_ptr())
        torch.cuda.synchronize()
        ex.forward_bgr_frames_dev([dev[1]])
        d_words = torch.full((4 * (8 + 4 * S),), 0xA5, dtype=torch.uint8, device="cuda")
        ex.flow_boxes([0], c_spec(F, sp), d_state.data_ptr(), 1, d_words.data_ptr())
        torch.cuda.synchronize()
        dets, boxes = ex.read_dets(), ex.read_boxes(0)
    flowref.update([flowref.luma_bgr(f) for f in frames], [0, 0], sp, st)
    flat = np.zeros(S, flowref.BOX_DTYPE)
    flat[:len(boxes)] = boxes
    want = flowref.boxes(dets, flat, S, None, [0], sp, st)
    assert d_state.cpu().numpy().tobytes() == st.tobytes() and d_words.cpu().numpy().tobytes() == want.tobytes()
    assert want[0, 0] >= 1 and want[0, 3:6].tolist() == [2, 3, -2] and want[0, 9::4].sum() > 0
