"""The merged stage (k_irb_stage: a run of 48 -> 224 -> 48 blocks on a small plane as one launch, one frame per workgroup) against the per-block launches
it replaces, bit for bit, and against the reference chain.

Every case builds a small net (tests/irb_stage/nets.py) and runs the same frames through two FFGPU_CONCURRENT executors: FFGPU_IRB_STAGE=0 (one k_irbw XL
launch per block) and 1 (the run merged).  The two outputs must be EQUAL AS BIT PATTERNS -- NaN by position, the sign of zero included: both paths do the
same operations in the same order.  The merged output is also held to tests/irb_blocks/blockref.py chained B times (the oracle's fp32 chain, a float64
restatement as the yardstick) under the bound of tests/irb_blocks/test_gpu_kernels.py, so that a defect both GPU paths share does not pass:
    E_k <= 2 E_ref + 1e-6   and   E_k <= 8e-7 max |y| + 1e-6      (E = max |. - float64| over the outputs finite in both)
with the same NaN positions and equal +-Inf values as the fp32 chain.

Shapes: 32 frames (the fewest the merge takes) and 33; 2 and 5 blocks; planes 10x10, 9x7 (odd width: scalar rows, a partial second strip), 12x10 (120
pixels, the most 32 row quads hold at that width) and 4x4 (one strip, most lanes idle); leaky, relu on expand and depthwise with a NaN in the input,
linear everywhere; +Inf and -Inf in border and interior pixels (the zero ring: an Inf at the edge reaches exactly the outputs it reaches per block).

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import functools

import numpy as np
import pytest

from irb_blocks import blockref
from irb_stage import nets

pytestmark = pytest.mark.gpu

# (id, W, H, N, B, act1, actd, plant)
CASES = [
    ("10x10-n32-b5-leaky", 10, 10, 32, 5, 2, 2, None),
    ("10x10-n33-b2-leaky-inf", 10, 10, 33, 2, 2, 2, "inf"),
    ("9x7-n33-b2-relu-nan", 9, 7, 33, 2, 1, 1, "nan"),
    ("9x7-n32-b5-leaky-inf", 9, 7, 32, 5, 2, 2, "inf"),
    ("12x10-n32-b2-linear", 12, 10, 32, 2, 0, 0, None),
    ("12x10-n33-b5-relu-nan", 12, 10, 33, 5, 1, 1, "nan"),
    ("4x4-n33-b5-leaky-inf", 4, 4, 33, 5, 2, 2, "inf"),
    ("4x4-n32-b2-linear", 4, 4, 32, 2, 0, 0, None),
]


def plant(x, what, N, W, H):
    xf = x.reshape(nets.IC, N, H, W)
    if what == "inf":
        xf[0, 0, 0, 0] = np.inf                                  # a corner, an edge, an interior pixel; the last frame's last pixel
        xf[5, 1, H - 1, W // 2] = -np.inf
        xf[17, 2, H // 2, W // 2] = np.inf
        xf[nets.IC - 1, N - 1, H - 1, W - 1] = -np.inf
    elif what == "nan":
        xf[3, 0, 0, W - 1] = np.nan
        xf[20, N - 1, H // 2, W // 2] = np.nan


@functools.lru_cache(maxsize=None)
def reference(i, seed=0):
    """frames (N, 48, H, W), the filters, and both chains of CASES[i], computed once (read only)"""
    from oracle import orc
    orc.build()
    _, W, H, N, B, act1, actd, what = CASES[i]
    x, filters = nets.draw(7000 + 10 * i + 1000 * seed, N, W, H, B)
    plant(x, what, N, W, H)
    shape = (N, W, H, nets.IC, nets.EC, nets.IC, 1)
    y32, y64 = x, x.astype(np.float64)
    for f1, fd, f2 in filters:
        y32 = blockref.chain32(orc, y32, f1, fd, f2, y32, *shape, (act1, actd, 0, 0)).reshape(nets.IC * N, H, W)
        y64 = blockref.block64(y64, f1, fd, f2, y64, *shape, (act1, actd, 0, 0)).reshape(nets.IC * N, H, W)
    frames = np.ascontiguousarray(x.reshape(nets.IC, N, H, W).transpose(1, 0, 2, 3))
    for a in (frames, y32, y64):
        a.setflags(write=False)
    return frames, filters, y32.reshape(nets.IC, N, H, W), y64.reshape(nets.IC, N, H, W)


@pytest.fixture(scope="module")
def F():
    from ffcnn_amd import capi
    capi.lib()
    return capi


def clean_env(monkeypatch):
    from test_irb_choice import knob_names
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)


def run(F, net, monkeypatch, stage, N, B, batches):
    """the last shortcut's tensor, (48, N, H, W) as uint32 bits, after each batch of frames in turn through ONE executor; and its launches per forward"""
    monkeypatch.setenv("FFGPU_IRB_STAGE", str(stage))
    import torch
    c, h, w = net.out_shape(net.layer_num - 1)
    spec = F.feature_spec(-1, F.FFGPU.FEAT_FLAT, F.FFGPU.POST_NONE)
    outs = []
    with net.executor(N, F.FFGPU.CONCURRENT) as ex:
        for frames in batches:
            ex.forward_host(frames)
            rows = torch.full((N, c * h * w), float("nan"), device="cuda")
            torch.cuda.synchronize()                             # (the fill runs on torch's stream, the rows are written on the executor's)
            assert ex.features(spec, rows.data_ptr()) == c * h * w
            torch.cuda.synchronize()
            outs.append(np.ascontiguousarray(rows.cpu().numpy().reshape(N, c, h, w).transpose(1, 0, 2, 3)).view(np.uint32))
        return outs, ex.kernel_count


def load(F, tmp_path, W, H, B, act1, actd, filters):
    cfg = str(tmp_path / "stage.cfg")
    open(cfg, "w").write(nets.cfg_text(W, H, B, act1, actd))
    net = F.Net(cfg, None)
    nets.fill(net, filters)
    return net


def same_bits(a, b, what):
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%s: %d of %d outputs differ in their bits, first at (channel, frame, y, x) %r: %r / %r" % (
        what, len(bad), a.size, bad[:4].tolist(), a.view(np.float32)[tuple(bad[0])], b.view(np.float32)[tuple(bad[0])])


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_stage_equals_blocks(F, i, tmp_path, monkeypatch):
    name, W, H, N, B, act1, actd, what = CASES[i]
    clean_env(monkeypatch)
    assert F.irb_plan_text((N, W, H, nets.IC, nets.EC, nets.IC, 1, act1, actd, 0, 0), F.FFGPU.CONCURRENT).startswith("irbw<12,3,1,2,big,x3,xl> ")
    frames, filters, y32, y64 = reference(i)
    with load(F, tmp_path, W, H, B, act1, actd, filters) as net:
        (blocks,), kb = run(F, net, monkeypatch, 0, N, B, [frames])
        (stage,), ks = run(F, net, monkeypatch, 1, N, B, [frames])
    assert kb - ks == B - 1, "the run of %d blocks was not merged into one launch (%d / %d launches)" % (B, kb, ks)
    same_bits(stage, blocks, name)
    got = stage.view(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(y32)), "%s: NaN at %r, the chain's at %r" % (name, np.argwhere(np.isnan(got))[:4].tolist(), np.argwhere(np.isnan(y32))[:4].tolist())
    inf = np.isinf(y32)
    assert np.array_equal(got[inf], y32[inf]), "%s: +-Inf outputs differ" % name
    ok = np.isfinite(y32) & np.isfinite(y64)
    assert np.isfinite(got[ok]).all() and ok.any(), name
    E_k, E_ref, ymax = float(np.abs(got[ok] - y64[ok]).max()), float(np.abs(y32[ok] - y64[ok]).max()), float(np.abs(y64[ok]).max())
    print("RATIO %s E_k %.3g E_ref %.3g ymax %.3g E_k/E_ref %.3f E_k/ymax %.3g" % (name, E_k, E_ref, ymax, E_k / max(E_ref, 1e-30), E_k / ymax))
    assert blockref.criterion(E_k, E_ref, ymax), (name, E_k, E_ref, ymax)


def test_two_forwards_back_to_back(F, tmp_path, monkeypatch):
    """the merged launch twice on different frames, the first of them with +-Inf: ring, frame buffer and split image are clean between workgroup trips"""
    i = 1
    name, W, H, N, B, act1, actd, what = CASES[i]
    clean_env(monkeypatch)
    frames_a, filters, _, _ = reference(i)
    frames_b = np.random.default_rng(99).uniform(-1, 1, frames_a.shape).astype(np.float32)
    with load(F, tmp_path, W, H, B, act1, actd, filters) as net:
        blocks, kb = run(F, net, monkeypatch, 0, N, B, [frames_a, frames_b, frames_a])
        stage, ks = run(F, net, monkeypatch, 1, N, B, [frames_a, frames_b, frames_a])
    assert kb - ks == B - 1
    for k in range(3):
        same_bits(stage[k], blocks[k], "%s, forward %d" % (name, k))
    same_bits(stage[2], stage[0], "%s, the first frames again" % name)
    assert not np.isnan(stage[1].view(np.float32)).any()
