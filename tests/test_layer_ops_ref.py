"""CPU side of tests/layer_ops: the cfgs load, and the oracle's OPERATORS (orc.pool, orc.upsample, orc.shortcut, np.concatenate) -- what the GPU
tests compare the kernels with -- are pinned to the oracle's NET path and, where oracle/_ref is built, to the reference itself, non-finite inputs
included.  The inputs of the non-finite cases are held to their purpose here as well (cfgs.assert_inputs_reach), without a GPU."""
import numpy as np
import pytest

from layer_ops import cfgs
from test_gpu_parity import _write_random_weights

ALL = cfgs.every_cfg()
BIG = 1 << 21           # elements of the net input above which one frame is enough here (the large-grid cfgs)


def _load(orc, tmp_path, g):
    cfg, wts = str(tmp_path / (g.name + ".cfg")), str(tmp_path / (g.name + ".weights"))
    with open(cfg, "w") as fp:
        fp.write(g.cfg_text())
    o = orc.Oracle(cfg=cfg, weights=None)
    _write_random_weights(wts, o, 1 + len(g.name))
    o.close()
    return cfg, wts


def _oracle_reader(orc, cfg, wts, g, frames):
    o = orc.Oracle(cfg=cfg, weights=wts)
    assert o.nlayers == g.n
    for i in range(g.n):
        L = o.layer(i)
        if g.kind[i] != "yolo":
            assert (L.oc, L.oh, L.ow) == tuple(g.shape[i]), (g.name, i)
    outs = {}

    def read(layer, f):
        if f not in outs:
            o.input[...] = frames[f]
            o.n.s1, o.n.s2 = 1, 1
            o.forward(0)
            outs.clear()                                   # (one frame's activations at a time)
            outs[f] = {i: o.layer_out(i).copy() for i in range(g.n) if g.kind[i] not in ("yolo", "dropout")}
            outs[f][-1] = frames[f].copy()
        return outs[f][layer]
    return o, read


@pytest.mark.parametrize("g", ALL, ids=[g.name for g in ALL])
def test_cfg_loads_and_operators_match_the_net_path(orc, tmp_path, g):
    cfg, wts = _load(orc, tmp_path, g)
    frames = cfgs.plain_frames(g, 1)
    if g.c * g.h * g.w * g.batch > BIG:
        frames = frames[:1]
    o, read = _oracle_reader(orc, cfg, wts, g, frames)
    for f in range(len(frames)):
        cfgs.verify(orc, _one_frame(g, f), lambda layer, _f, f=f: read(layer, f), {0: frames[f]}, "oracle", merged=False)
    o.close()


class _one_frame:
    """a view of a Cfg with batch 1 whose frame 0 is frame f (the oracle keeps one frame's activations at a time)"""

    def __init__(self, g, f):
        self.ops, self.batch, self.name = g.ops, 1, "%s frame %d" % (g.name, f)


@pytest.mark.parametrize("case", cfgs.NONFINITE_CASES, ids=[c[0] for c in cfgs.NONFINITE_CASES])
def test_nonfinite_inputs_do_their_job(orc, tmp_path, case):
    """the crafted inputs through the oracle's net path: the operators equal it, and the inputs put NaN where the input has none / +-Inf into the
    outputs, as the GPU test requires of them.  Where oracle/_ref is built, the operators also equal the reference (v0) itself -- for the cfgs it
    can run: pool2x2, SPP, upsample, shortcut, route, and the generic pools at stride 1 (see below for strides that do not divide the plane)"""
    name, make, frames_of, purpose = case
    g = make()
    cfg, wts = _load(orc, tmp_path, g)
    frames = frames_of(g)
    o, read = _oracle_reader(orc, cfg, wts, g, frames)
    seen = []
    for f in range(g.batch):
        seen += [("fused",) + s[1:] for s in cfgs.verify(orc, _one_frame(g, f), lambda layer, _f, f=f: read(layer, f), {0: frames[f]}, "oracle", merged=False)]
    o.close()
    cfgs.assert_inputs_reach(purpose, g, seen)
    # the reference itself: only where its pool loop stays inside its output buffer.  It walks ix = 0, stride, ... < w (ffcnn.c:387-388), which
    # is ceil(w / stride) outputs per row, into a tensor sized w / stride (ffcnn.c:151-157): with w or h no multiple of the stride it writes
    # past the allocation.  The oracle and the kernels take the floor, the size the tensor has.
    if not orc.have_ref("v0") or any(g.out_shape(op.src[0])[k] % op.stride for op in g.ops if op.kind.endswith("pool") for k in (1, 2)):
        return
    for f in range(g.batch):
        r = orc.Ref("v0", cfg=cfg, weights=wts)           # (a fresh net per frame: a leading dropout moves the input buffer away, ffcnn.c:412-416)
        r.input[...] = frames[f]
        acts = r.forward(keep_activations=True)
        acts[-1] = frames[f]
        cfgs.verify(orc, _one_frame(g, f), lambda layer, _f: acts[layer], {0: frames[f]}, "reference", merged=False)
        r.n.layer_list[0].data = None                       # (forward(keep_activations) has released every tensor, the moved input among them)
        r.close()


def test_spp_cascade_restatement_against_the_reference_loop():
    """regression note for the k_spp defect this suite was written around (no product code runs here): a numpy restatement of the reference's
    window scan beside the row-pass / column-pass cascade k_spp uses for odd ascending sizes.  Finite planes agree at every size, clipped
    windows included; one NaN at (4, 6) of an 11 x 13 plane shows where they part -- the reference has it at (5, 7) / (6, 8) / (8, 10) for
    sizes 3 / 5 / 9 (the outputs whose window BEGINS on it), the plain cascade leaves it at (4, 6).  k_spp therefore gives planes that hold
    a NaN to the window scan."""
    def ref(p, fs):
        h, w = p.shape
        o = np.empty_like(p)
        for oy in range(h):
            for ox in range(w):
                x0, y0 = ox - (fs - 1) // 2, oy - (fs - 1) // 2
                x1, y1 = min(x0 + fs, w), min(y0 + fs, h)
                x0, y0 = max(x0, 0), max(y0, 0)
                v = p[y0, x0]
                for y in range(y0, y1):
                    for x in range(x0, x1):
                        if v < p[y, x]:
                            v = p[y, x]
                o[oy, ox] = v
        return o

    def cascade(p, sizes):
        h, w = p.shape
        cur, outs, prev = p.copy(), [], 1
        for fs in sizes:
            a = (fs - prev) // 2
            tmp, new = np.empty_like(cur), np.empty_like(cur)
            for oy in range(h):
                for ox in range(w):
                    v = cur[oy, ox]
                    for x in range(max(ox - a, 0), min(ox + a, w - 1) + 1):
                        if v < cur[oy, x]:
                            v = cur[oy, x]
                    tmp[oy, ox] = v
            for oy in range(h):
                for ox in range(w):
                    v = tmp[oy, ox]
                    for y in range(max(oy - a, 0), min(oy + a, h - 1) + 1):
                        if v < tmp[y, ox]:
                            v = tmp[y, ox]
                    new[oy, ox] = v
            outs.append(new)
            cur, prev = new, fs
        return outs
    p = np.random.default_rng(0).uniform(-1, 1, (11, 13)).astype(np.float32)
    for sizes in ((3, 5, 9), (5, 9, 13)):
        for o, fs in zip(cascade(p, sizes), sizes):
            assert np.array_equal(o, ref(p, fs))
    p[4, 6] = np.nan
    for o, fs, at in zip(cascade(p, (3, 5, 9)), (3, 5, 9), ((5, 7), (6, 8), (8, 10))):
        assert np.argwhere(np.isnan(ref(p, fs))).tolist() == [list(at)]
        assert np.argwhere(np.isnan(o)).tolist() == [[4, 6]]
