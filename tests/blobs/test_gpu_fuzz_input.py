"""Motion blobs on the device: ffgpu_blobs_dev against tests/blobs/blobref.py, the numpy restatement of the contract in include/ffcnn_hip.h: words,
records and labels byte for byte, guard bytes round each output, every case twice for identical bytes.  The states are built by writing cells.
(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import ctypes as C
import re

import numpy as np
import pytest

from blobs import blobref
from overlay import drawref
from test_gpu_round2 import F  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
G, A5 = 64, b"\xa5"


def scene(name, gw, gh, rng):
    m, (y, x) = np.zeros((gh, gw), bool), np.mgrid[:gh, :gw]
    if name == "serpentine":                                   # full rows joined at alternating ends: one component, the longest path there is
        m[::2], m[1::4, -1], m[3::4, 0] = True, True, True
    elif name == "bars":                                         # 3, 4 and 5 cells, runs over the mask words' boundaries, one that touches them diagonally, a twin pair
        m[0, :3], m[2, :4], m[4, :5], m[6, 60:70], m[7, 70:130], m[8, 0], m[8, gw - 1], m[gh - 1, 62:66], m[gh - 3, 62:66] = (True,) * 9
    else:
        m = {"full": x >= 0, "comb": (y == 0) | (x % 2 == 0), "checker": (x + y) % 2 == 0, "dots": (x % 2 == 0) & (y % 2 == 0)}.get(name)
    return rng.random((gh, gw)) < float(name) if m is None else m


def state_of(sp, masks, flat):
    """stream s holds masks[s] and has seen 5 + s frames: active cells at and above min_pixels up to 0xFFFFFFFF, the others below (flat: all alike)"""
    rng, st = np.random.default_rng(sp.gw), blobref.State(len(masks), sp.w, sp.h, sp.cell_log2)
    for s, m in enumerate(masks):
        st.hdr[s, 0] = 5 + s
        hot = sp.min_pixels if flat else rng.choice([sp.min_pixels, sp.min_pixels + 1, 16, 0xFFFFFFFF], m.shape)
        st.cells[s] = np.where(m, hot, 0 if flat else rng.choice([0, sp.min_pixels - 1], m.shape))
    return st


def check(F, sp, st, streams, labels=True):
    import torch
    want = blobref.blobs(streams, sp, st)
    lab = np.full(want[2].shape, 0xA5A5, "<u2")
    lab[:, :sp.gw * sp.gh] = want[2][:, :sp.gw * sp.gh]
    exp = [want[0].tobytes(), want[1].tobytes(), lab.tobytes() if labels else b""]
    d_state, got = torch.from_numpy(st.raw.reshape(-1).copy()).cuda(), []
    for _ in range(2):
        bufs = [torch.full((len(e) + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for e in exp]
        F.blobs_dev(streams, F.blobs_spec(sp.w, sp.h, sp.cell_log2, sp.min_pixels, sp.warmup, sp.connect, sp.min_cells, sp.max_cells, sp.max_boxes, sp.pad, sp.type),
                    d_state.data_ptr(), st.nstreams, bufs[0].data_ptr() + G, bufs[1].data_ptr() + G, bufs[2].data_ptr() + G if labels else None)
        torch.cuda.synchronize()
        got.append([b.cpu().numpy().tobytes() for b in bufs])
    assert got[0] == got[1] and d_state.cpu().numpy().tobytes() == st.tobytes()
    for name, g, e in zip(("words", "records", "labels"), got[0], exp):
        assert g == A5 * G + e + A5 * G, (name, want[0][:4])
    return want[0]


# id: scene, gw, gh, spec, streams, flat cells, (kept at least, filtered at least) by the reference's words
CASES = {
    "1x1": ("full", 1, 1, {}, [0, 1], False, (1, 0)),
    "bars 131 4-connected": ("bars", 131, 12, dict(connect=4, min_cells=4, max_cells=4, pad=3), [1, 0], True, (3, 5)),
    "bars 131 8-connected": ("bars", 131, 12, dict(connect=8, min_cells=5, max_boxes=1, type_=-3), [1], False, (2, 3)),
    "serpentine 128x64": ("serpentine", 128, 64, dict(connect=4, pad=256), [0, 1], False, (1, 0)),
    "comb 65": ("comb", 65, 33, dict(connect=4), [0, 1], False, (1, 0)),
    "checker 4": ("checker", 20, 10, dict(connect=4, max_boxes=128), [1, 1], True, (100, 0)),
    "checker 8": ("checker", 63, 9, dict(connect=8), [0, 1], False, (1, 0)),
    "dots 128x66 above the table": ("dots", 128, 66, dict(connect=8, max_boxes=128), [1], True, (2048, 0)),
    "full 256x128": ("full", 256, 128, dict(pad=1), [1], False, (1, 0)),
    "warm-up, -1, twice, 130 targets, no labels": ("0.3", 64, 9, dict(warmup=5, min_cells=2), [0, -1, 1, 1, 0] * 26, False, (1, 1)),
    "65 targets": ("0.3", 65, 5, dict(min_cells=2, connect=4), [1, 0, -1, 1, 1] * 13, False, (1, 1)),
    "random 5%": ("0.05", 129, 40, dict(min_cells=2), [0, 1], False, (1, 1)),
    "random 30% 4-connected": ("0.3", 63, 40, dict(connect=4, min_cells=3, max_cells=6), [0, 1], False, (1, 1)),
    "random 60%": ("0.6", 240, 135, dict(connect=4, min_cells=2, max_boxes=7), [1], False, (7, 1)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_blobs_against_reference(F, case):
    name, gw, gh, kw, streams, flat, (kept, filtered) = CASES[case]
    sp = blobref.Spec(4 * gw - 1, 4 * gh - 2, 2, min_pixels=3, **kw)
    rng = np.random.default_rng(gw * gh)
    words = check(F, sp, state_of(sp, [scene(name, gw, gh, rng), np.roll(scene(name, gw, gh, rng), 1, axis=1)], flat), streams, labels="no labels" not in case)
    warm = words[words[:, 5] == 1]
    assert len(warm) and (warm[:, 2] >= kept).all() and (warm[:, 1] - warm[:, 4] - warm[:, 2] >= filtered).all(), warm


def test_rejections_write_nothing(F):
    import torch
    sp, arr = F.blobs_spec(65, 33, 3, 8), (C.c_int * 2)(0, 1)
    bufs = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for n in (4096, 64, 2 * 3088, 256)]
    good = dict(streams=arr, n=2, spec=sp, state=bufs[0].data_ptr(), nstreams=2, words=bufs[1].data_ptr(), recs=bufs[2].data_ptr(), labels=bufs[3].data_ptr())
    for change, msg in ((dict(streams=None), "NULL streams"), (dict(spec=None), "NULL spec"), (dict(state=None), "NULL state"), (dict(words=None), "NULL words"),
                        (dict(recs=None), "NULL records"), (dict(n=0), "0 targets (ntargets >= 1)"), (dict(nstreams=0), "nstreams 0 is outside 1..65536"),
                        (dict(state=bufs[0].data_ptr() + 8), "the state must be 16-byte aligned"), (dict(nstreams=1), "target 1: stream 1 is outside -1 .. 0"),
                        (dict(streams=(C.c_int * 2)(0, -2)), "target 1: stream -2 is outside -1 .. 1"), (dict(spec=F.blobs_spec(65, 33, 3, 8, connect=5)), "connect 5 is neither 4 nor 8"),
                        (dict(spec=F.blobs_spec(1920, 1080, 2, 1)), "a grid of 480 x 270 cells (32768 cells at most)")):
        assert F.lib().ffgpu_blobs_dev(*dict(good, **change).values(), None) < 0
        assert re.search(re.escape("blobs_dev: " + msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert all(b.cpu().numpy().tobytes() == A5 * b.numel() for b in bufs)


def test_update_blobs_draw(F):
    """a real update on two frames that differ in two rectangles, blobs on its state, the draw operator on the blobs record"""
    import torch
    w, h = 150, 90
    a = np.random.default_rng(1).integers(0, 40, (h, w, 3), dtype=np.uint8)
    b = a.copy()
    b[10:30, 20:70], b[50:85, 100:149] = 250, 200                                       # 7 x 3 and 7 x 5 cells of 8 pixels
    dev = torch.from_numpy(np.stack([a, b])).cuda()
    d_state = torch.zeros(F.motion_state_bytes(1, w, h, 3), dtype=torch.uint8, device="cuda")
    d_rows, d_words, d_recs = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (128, 32, 3088))
    F.motion_update_bgr_dev([dev[0], dev[1]], [0, 0], F.motion_spec(w, h, 3, min_pixels=8), d_state.data_ptr(), 1, d_rows.data_ptr())
    F.blobs_dev([0], F.blobs_spec(w, h, 3, 8, warmup=1, pad=2, type_=1), d_state.data_ptr(), 1, d_words.data_ptr(), d_recs.data_ptr())
    F.draw_boxes_bgr_dev(d_recs.data_ptr(), None, 0, [dev[1]], F.draw_style((0, 0, 255), thickness=2))
    torch.cuda.synchronize()
    st = blobref.State(1, w, h, 3, d_state.cpu().numpy())
    words, recs, _ = blobref.blobs([0], blobref.Spec(w, h, 3, 8, warmup=1, pad=2, type_=1), st)
    assert d_recs.cpu().numpy().tobytes() == recs.tobytes() and recs["count"][0] == 2 and words[0, :7].tolist() == [3 * 7 + 5 * 7, 2, 2, 2, 0, 1, 2]
    want = drawref.draw_bgr(b.reshape(-1).copy(), 0, w, h, 3 * w, recs["box"][0][:2], [(0, 0, 255)] * 2, 2)
    assert dev[1].cpu().numpy().tobytes() == want.tobytes()
