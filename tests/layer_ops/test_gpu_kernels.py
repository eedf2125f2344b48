"""The layers between the convolutions -- k_pool, k_pool2x2, k_spp, k_upsample32 / k_upsample, k_add_act, k_copy and the frame-major -> CNHW
staging in front of them -- held to EQUALITY with the oracle's operators (orc.pool, orc.upsample, orc.shortcut, np.concatenate).

Each case is a tiny darknet cfg (tests/layer_ops/cfgs.py) with random weights, run by an FFGPU_KEEP_ALL executor.  The oracle's operator is
applied to the EXECUTOR'S OWN output of the op's source layers, so the comparison is exact whatever the convolutions in front did.  Every op
layer must be readable (read_layer raises on a tensor that was not materialised), and the executor's step list must be the one the cfg's author
wrote down (cfgs.Cfg.steps): merged SPP pools disappear as steps, in-place routes make no launch, an unfused plan launches everything.
The comparison rules are in cfgs.check.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import numpy as np
import pytest

from layer_ops import cfgs
from test_gpu_parity import _write_random_weights

pytestmark = pytest.mark.gpu

PLANS = (("fused", True, {}), ("unfused", False, {}))
PLANS_POOL2X2 = PLANS + (("fused, FFGPU_NO_POOL2X2", True, {"FFGPU_NO_POOL2X2": "1"}),)


@pytest.fixture(scope="module")
def F():
    import ffcnn_amd  # noqa: F401
    from ffcnn_amd import capi
    capi.lib()
    return capi


def run(F, orc, tmp_path, monkeypatch, g, frames, plans=PLANS):
    """one forward of `frames` per plan; every op layer of `g`, every frame, against the oracle's operator on the executor's own copy of the
    op's sources.  Returns [(plan, op, frame, sources, expected)] for the assertions a test makes about its inputs."""
    cfg, wts = str(tmp_path / (g.name + ".cfg")), str(tmp_path / (g.name + ".weights"))
    with open(cfg, "w") as fp:
        fp.write(g.cfg_text())
    o = orc.Oracle(cfg=cfg, weights=None)
    _write_random_weights(wts, o, 1 + len(g.name))
    o.close()
    seen = []
    with F.Net(cfg, wts) as net:
        assert net.layer_num == g.n
        for plan, fuse, env in plans:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            with net.executor(g.batch, F.FFGPU.KEEP_ALL | (0 if fuse else F.FFGPU.NO_FUSE)) as ex:       # (a fresh one: a captured graph keeps its launches)
                model = [lay for lay, _ in ex.step_model()]
                assert [lay for lay in model if lay >= 0] == g.steps[fuse], "%s, %s plan: launches of layers %s" % (g.name, plan, model)
                assert sum(lay < 0 for lay in model) == g.extra[fuse], "%s, %s plan: launches %s" % (g.name, plan, model)
                ex.forward_host(frames)
                seen += cfgs.verify(orc, g, ex.read_layer, frames, plan, merged=fuse)
            for k in env:
                monkeypatch.delenv(k)
    return seen


# ----------------------------------------------------------------------------------------------------------------------- 1. k_pool
@pytest.mark.parametrize("c,batch", [(3, 2), (5, 1)])
@pytest.mark.parametrize("plane", cfgs.POOL_PLANES)
def test_pool_generic(F, orc, tmp_path, monkeypatch, plane, c, batch):
    """max and avg, sizes 1-13 x strides 1-3: windows larger than the plane, even sizes (the asymmetric window), w or h no multiple of the stride"""
    g = cfgs.pool_grid(plane[0], plane[1], c, batch)
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 1))


def test_pool_grid_stride_loop(F, orc, tmp_path, monkeypatch):
    g = cfgs.pool_big()
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 2))


# -------------------------------------------------------------------------------------------------------------------- 2. k_pool2x2
@pytest.mark.parametrize("w,h", [(w, h) for w in cfgs.POOL2_W for h in cfgs.POOL2_H] + list(cfgs.POOL2_FALLBACK))
def test_pool2x2(F, orc, tmp_path, monkeypatch, w, h):
    """four outputs per thread: one quad per row (w = 8), power-of-two and other magic divisors; w % 8 != 0 and odd h fall back to k_pool"""
    g = cfgs.pool2x2(w, h)
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 3), PLANS_POOL2X2)


# ------------------------------------------------------------------------------------------------------------------------ 3. k_spp
@pytest.mark.parametrize("form", ["cascade", "direct"])
@pytest.mark.parametrize("plane", cfgs.SPP_PLANES)
def test_spp(F, orc, tmp_path, monkeypatch, plane, form):
    """cascade: (3,5,9), (5,9,13), (5,9); direct: (9,5,3), (5,5), (2,4), (3,4,9).  15 planes: the last trip of a workgroup has one plane"""
    g = cfgs.spp(plane[0], plane[1], cfgs.SPP_CASCADE if form == "cascade" else cfgs.SPP_DIRECT)
    seen = run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 4))
    assert any(op.merged for (_, op, _, _, _) in seen)


def test_spp_workgroup_loops(F, orc, tmp_path, monkeypatch):
    g = cfgs.spp_many_planes()
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 5))


@pytest.mark.parametrize("plane", cfgs.SPP_EDGE_PLANES)
def test_spp_plane_size_edges(F, orc, tmp_path, monkeypatch, plane):
    """16 w h bytes of dynamic LDS: 64 x 64 is 64 KB exactly, 80 x 52 the first plane above it, 128 x 64 the largest merged one (128 KB);
    128 x 65 is not merged (three k_pool launches in both plans)"""
    g = cfgs.spp(plane[0], plane[1], [(3, 5, 9)], c=3, batch=1)
    seen = run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 6))
    assert any(op.merged for (_, op, _, _, _) in seen) == (plane[0] * plane[1] <= 8192)


# ------------------------------------------------------------------------------------------------------------ 4. non-finite values
@pytest.mark.parametrize("case", cfgs.NONFINITE_CASES, ids=[c[0] for c in cfgs.NONFINITE_CASES])
def test_nonfinite(F, orc, tmp_path, monkeypatch, case):
    """NaN (with payloads, both signs), +-Inf and -0 through every op: as crafted input of a first-layer op (batch 1 reads the frames, batch > 1
    the staged CNHW copy) and behind a 1x1 conv (a NaN pixel is NaN in every channel there).  cfgs.assert_inputs_reach holds the inputs to their
    purpose: +Inf and -Inf in the expected outputs, and an oracle NaN at a position where the input has none for every stride-1 max pool."""
    name, make, frames_of, purpose = case
    g = make()
    seen = run(F, orc, tmp_path, monkeypatch, g, frames_of(g), PLANS_POOL2X2 if purpose == "pool2x2" else PLANS)
    cfgs.assert_inputs_reach(purpose, g, seen)


# ----------------------------------------------------------------------------------------------------------------- 5. k_upsample32
@pytest.mark.parametrize("plane", cfgs.UPSAMPLE_PLANES)
def test_upsample(F, orc, tmp_path, monkeypatch, plane):
    """strides 1-4; magic 0 for a dimension of 1, divisors with the largest rounding excess of ceil(2^32 / d) (3, 5, 17, 257)"""
    g = cfgs.upsample_grid(plane[0], plane[1])
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 13))


def test_upsample_grid_stride_loop(F, orc, tmp_path, monkeypatch):
    g = cfgs.upsample_big()
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 15))


def test_upsample_64bit_fallback(F, orc, tmp_path, monkeypatch):
    g = cfgs.upsample_wide()
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 16))


# --------------------------------------------------------------------------------------------------------- 6. k_add_act and k_copy
@pytest.mark.parametrize("shape", cfgs.ADD_SHAPES)
def test_shortcuts(F, orc, tmp_path, monkeypatch, shape):
    """shortcuts no conv absorbs: behind a pool, behind a route, the net input as either side; linear, leaky, relu; n % 4 = 1, 2, 3, 0"""
    g = cfgs.shortcuts(*shape)
    seen = run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 17))
    assert sorted({op.act for (_, op, _, _, _) in seen if op.kind == "shortcut"}) == [0, 1, 2]


def test_shortcut_grid_stride_loop(F, orc, tmp_path, monkeypatch):
    g = cfgs.shortcut_big()
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 18))


@pytest.mark.parametrize("shape", cfgs.ROUTE_SHAPES)
def test_route_copies(F, orc, tmp_path, monkeypatch, shape):
    """two and three sources with odd element counts (the later destinations are not 16-byte aligned); a fused plan builds the first route
    in place and copies for the others"""
    g = cfgs.routes(*shape)
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 19))


def test_route_copy_grid_stride_loop(F, orc, tmp_path, monkeypatch):
    g = cfgs.route_big()
    run(F, orc, tmp_path, monkeypatch, g, cfgs.plain_frames(g, 21))
