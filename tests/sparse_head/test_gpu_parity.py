"""Yolo-fastest with the two layers in front of its yolo heads (layers 120 and 129 as read_layer counts them) in the sparse form (FFGPU_SPARSE_HEAD=1, the default) against the same executor
with the dense launches (=0): the detection records -- counts, boxes, classes, scores, the full lists behind them -- must be the same BYTES, because every
value k_yolo reads is produced by the same instructions either way.

Batches 1, 3 and 5 are smaller than the ones AUTO gives k_conv_x3's pointwise form to, so every executor here is made under FFGPU_PWX3S_MIN_WGS=1 (both
settings alike); ffgpu_sparse_head_launch_text confirms that the form is on where it is meant to be.  Frames: the test image, noise, a frame of constants
and the image mirrored.  The form is taken by FFGPU_CONCURRENT executors only (a single chain measured slower with it), so of the executors here -- plain, FFGPU_CONCURRENT,
FFGPU_SPLIT2 with and without FFGPU_CONCURRENT (at the odd batches the split does not happen: the unsplit plan again) -- the plain ones compare the dense
launch with itself.  And an FFGPU_CONCURRENT executor of a
copy of the cfg with ignore_thresh = 0, where every (cell, anchor) passes and the class pass takes every quad.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the parity tests.)"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from ffcnn_amd import capi
    capi.lib()
    return capi, torch


HEADS = ((120, 10, 96), (129, 20, 120))           # layer (read_layer's index: the layer in front of each [yolo]), plane, input channels
YOLO_KIND = 7                                     # LAYER_TYPE_YOLO (include/ffcnn.h)


@pytest.fixture()
def clean(monkeypatch):
    from test_irb_choice import knob_names
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FFGPU_PWX3S_MIN_WGS", "1")
    return monkeypatch


@functools.lru_cache(maxsize=None)
def frames_of(N):
    from ffcnn_amd import capi
    with capi.Net() as net:
        bgr, w, h = capi.load_bmp(os.path.join(os.path.dirname(capi.CFG), "test.bmp"))
        net.set_input_image(bgr, w, h)
        base = np.array(net.input, np.float32)
    rng = np.random.default_rng(77)
    kinds = [base, rng.uniform(0, 1, base.shape).astype(np.float32), np.full_like(base, 0.37), base[:, :, ::-1]]
    f = np.stack([kinds[k % 4] for k in range(N)]).astype(np.float32)
    f.setflags(write=False)
    return f


def records(ex, N):
    """everything a caller can read of a forward's detections, as bytes: per frame the record's count and boxes and the full list"""
    d = ex.read_dets()
    out = []
    for k in range(N):
        out.append((int(d[k]["count"]), int(d[k]["ncand"]), d[k]["box"][: d[k]["count"]].tobytes(), ex.read_boxes(k).tobytes()))
    return out


def forward_both(capi, clean, net, N, flags, twice=False):
    got = {}
    for knob in ("1", "0"):
        clean.setenv("FFGPU_SPARSE_HEAD", knob)
        for _, hw, ic in HEADS:
            line = capi.sparse_head_launch_text(N, hw, hw, ic, 80, flags)
            assert line.startswith("sparse box<1,4> " if knob == "1" and flags & capi.FFGPU.CONCURRENT else "dense pw_x3s"), line
        assert [i - 1 for i in range(net.layer_num) if net.layer(i).type == YOLO_KIND] == [h[0] for h in HEADS]
        with net.executor(N, flags) as ex:
            ex.set_scale(1, 1)
            ex.forward_host(frames_of(N))
            got[knob] = records(ex, N)
            if twice:
                ex.forward_host(frames_of(N))
                assert records(ex, N) == got[knob], "knob %s: the second forward's records differ from the first's" % knob
                ex.forward_host(frames_of(N)[::-1].copy())
                ex.forward_host(frames_of(N))
                assert records(ex, N) == got[knob], "knob %s: a forward behind other frames differs" % knob
            if knob == "1" and flags & capi.FFGPU.CONCURRENT:
                for layer, _, _ in HEADS:
                    with pytest.raises(RuntimeError, match="not materialised"):
                        ex.read_layer(layer, 0)
    return got


@pytest.mark.parametrize("N", [1, 3, 5])
def test_records_bit_identical(env, clean, N):
    capi, _ = env
    with capi.Net() as net:
        for flags in (0, capi.FFGPU.CONCURRENT, capi.FFGPU.SPLIT2, capi.FFGPU.SPLIT2 | capi.FFGPU.CONCURRENT):
            got = forward_both(capi, clean, net, N, flags, twice=flags == capi.FFGPU.CONCURRENT)
            assert got["1"] == got["0"], "batch %d flags %d: records differ between FFGPU_SPARSE_HEAD=1 and =0" % (N, flags)
            assert sum(r[0] for r in got["1"]) >= 3, "no detections"


def test_split_executor_even_batch(env, clean):
    """a batch the split really halves: each half has its own list and counter"""
    capi, _ = env
    with capi.Net() as net:
        got = forward_both(capi, clean, net, 4, capi.FFGPU.SPLIT2 | capi.FFGPU.CONCURRENT, twice=True)
        assert got["1"] == got["0"]


@pytest.mark.parametrize("N", [1, 3, 5])
def test_every_cell_passes(env, clean, N, tmp_path):
    capi, _ = env
    text = open(capi.CFG).read()
    assert text.count("ignore_thresh = .45") == 2
    cfg = tmp_path / "all_pass.cfg"
    cfg.write_text(text.replace("ignore_thresh = .45", "ignore_thresh = 0"))
    with capi.Net(cfg=str(cfg)) as net:
        got = forward_both(capi, clean, net, N, capi.FFGPU.CONCURRENT)
        assert got["1"] == got["0"]
        assert max(r[0] for r in got["1"]) > 20, "the threshold did not open the heads"


def test_keep_all_reads_the_head_layers(env, clean):
    """FFGPU_KEEP_ALL keeps the dense launch: the head layers are whole and read_layer returns them, the same bits whatever the knob says"""
    capi, _ = env
    got = {}
    with capi.Net() as net:
        for knob in ("1", "0"):
            clean.setenv("FFGPU_SPARSE_HEAD", knob)
            with net.executor(3, capi.FFGPU.KEEP_ALL) as ex:
                ex.forward_host(frames_of(3))
                got[knob] = [ex.read_layer(layer, 2).tobytes() for layer, _, _ in HEADS] + [records(ex, 3)]
    assert got["1"] == got["0"]
