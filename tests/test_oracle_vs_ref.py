"""Pin the oracle to the reference ITSELF: bit for bit against tests/golden/ref_pins.npz (what the unmodified reference computed:
oracle/gen_golden.py ref_pins) everywhere, and against the live reference (oracle/_ref, built by oracle/Makefile where the
reference tree is present) as well when that build exists."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLD

TABLE_FIELDS = ("type", "w", "h", "c", "fs", "fn", "stride", "pad", "groups", "batchnorm", "activation", "depend_num")
V2_CASES = [(8, 9, 11, 1, 1, 1, 0, 12), (6, 8, 8, 6, 3, 1, 1, 6), (3, 10, 10, 1, 3, 2, 1, 8)]     # (ic, ih, iw, groups, fs, stride, pad, fn)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLD, "ref_pins.npz"))


def live_ref(orc, variant="v0"):
    """the reference build itself where oracle/_ref has it, else None"""
    return orc.Ref(variant) if orc.have_ref(variant) else None


def test_every_layer_bit_exact(orc, pins, test_image):
    bgr, w, h = test_image
    o, r = orc.Oracle(), live_ref(orc)
    try:
        o.set_input_image(bgr, w, h)
        assert sha(o.input) == str(pins["input_sha"])
        assert sha(o.weights()) == str(pins["weights_sha"])
        o.forward(0)
        for i, want in zip(pins["layer_ids"], pins["layer_sha"]):
            assert sha(o.layer_out(int(i))) == str(want), "layer %d" % i
        assert o.boxes.tobytes() == pins["boxes"].tobytes()
        if r is not None:
            r.set_input_image(bgr, w, h)
            assert np.array_equal(o.input, r.input)
            assert np.array_equal(o.weights(), np.ctypeslib.as_array(r.n.weight_buf, (r.n.weight_size,)))
            outs = r.forward(keep_activations=True)
            assert sorted(outs) == [int(i) for i in pins["layer_ids"]]
            for i, a in outs.items():
                assert np.array_equal(o.layer_out(i), a), "layer %d" % i
            assert np.array_equal(o.boxes, r.boxes)
    finally:
        o.close()
        if r is not None:
            r.close()


def test_layer_table_fields(orc, pins):
    o, r = orc.Oracle(), live_ref(orc)
    try:
        tables = [pins["table"]]
        if r is not None:
            assert r.n.layer_num == int(pins["layer_num"])
            tables.append(np.array([[getattr(r.layer(i), k) for k in TABLE_FIELDS] + list(r.layer(i).depend_list)
                                    for i in range(r.n.layer_num + 1)], np.int32))
        assert o.nlayers == int(pins["layer_num"])
        for t in tables:
            for i in range(o.nlayers):
                a, b, nxt = o.layer(i), dict(zip(TABLE_FIELDS, t[i])), dict(zip(TABLE_FIELDS, t[i + 1]))
                assert (a.kind, a.iw, a.ih, a.ic) == (b["type"], b["w"], b["h"], b["c"]), i
                if a.kind != 7:
                    assert (a.ow, a.oh, a.oc) == (nxt["w"], nxt["h"], nxt["c"]), i
                if a.kind == 0:
                    assert (a.fs, a.fn, a.stride, a.pad, a.groups, a.batchnorm, a.act) == \
                           (b["fs"], b["fn"], b["stride"], b["pad"], b["groups"], b["batchnorm"], b["activation"]), i
                assert list(a.dep)[:a.ndep] == list(t[i][len(TABLE_FIELDS):])[:b["depend_num"]]
    finally:
        o.close()
        if r is not None:
            r.close()


def test_random_groupconv_vs_v2_im2col(orc, pins):
    """conv-v2.c (im2col+GEMM, the variant the north star names) is bit-identical too."""
    r = live_ref(orc, "v2")
    try:
        for k, (ic, ih, iw, g, fs, s, p, fn) in enumerate(V2_CASES):
            x, f = pins["v2_%d_x" % k], pins["v2_%d_f" % k]
            got = orc.groupconv(x, f, g, p, s, fs, 2)
            assert np.array_equal(got, pins["v2_%d_out" % k]), k
            if r is not None:
                assert np.array_equal(got, r.groupconv(x, f, g, p, s, fs, 2)), k
    finally:
        if r is not None:
            r.close()


@pytest.mark.parametrize("bbox_max", [0, 700, 40])
def test_candidate_capacity_regimes_bit_exact(orc, pins, test_image, bbox_max):
    """ignore_thresh = 0 (1 500 candidates per frame, hundreds of boxes after NMS) and net->bbox_max lowered until the
    reference's emission-order truncation bites (ffcnn.c:463): the oracle's candidate cap reproduces both bit for bit"""
    bgr, w, h = test_image
    o, r = orc.Oracle(), live_ref(orc)
    try:
        for i in range(o.nlayers):
            if o.layer(i).kind == 7:
                o.layer(i).thresh = 0.0
                if r is not None:
                    r.layer(i).ignore_thres = 0.0
        if bbox_max:
            o.n.cap = bbox_max
            if r is not None:
                r.n.bbox_max = bbox_max
        o.set_input_image(bgr, w, h)
        o.forward(0)
        assert o.n.ncand == (bbox_max or 1500)
        assert o.boxes.tobytes() == pins["cap_%d_boxes" % bbox_max].tobytes() and len(o.boxes) > (100 if not bbox_max else 5)
        if r is not None:
            r.set_input_image(bgr, w, h)
            r.forward()
            assert o.boxes.tobytes() == r.boxes.tobytes()
    finally:
        o.close()
        if r is not None:
            r.close()
