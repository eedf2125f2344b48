"""Which form an executor's launch of the pointwise layer in front of a yolo head takes (ffgpu_sparse_head_launch_text: pure host code, no GPU): the
sparse pair with its grids against a restatement of the launcher's arithmetic, and every switch that keeps the dense launch."""
import pytest

KEEP_ALL, NO_FUSE, SPLIT2, CONCURRENT = 1, 8, 32, 64           # include/ffcnn_hip.h


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture()
def clean(monkeypatch):
    from test_irb_choice import knob_names
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def want_line(N, hw, ic, classes, mt, nw=4):
    """two launches on the dense launch's pixel ranges: one channel tile of one 16-row block, then ceil(ceil(3 classes / 16) / MT) tiles of MT blocks"""
    P = N * hw * hw
    ntn = -(-P // 64)
    npg = -(-ntn // nw)
    slots = -(-npg // 8) * 8
    ngr = -(-(ic // 8) // 4)
    nrb = {0: -(-3 * (5 + classes) // 16), 1: 1, 2: -(-3 * classes // 16)}
    mts = {0: mt, 1: 1, 2: mt}
    ntm = {k: -(-nrb[k] // mts[k]) for k in nrb}
    image = sum(ntm[k] * ngr * 3 * mts[k] * 256 for k in nrb)
    return "sparse box<1,%d> rows=15 grid=%d class<%d,%d> rows=%d grid=%d quads=%d image=%d" % (nw, slots, mt, nw, 3 * classes, slots * ntm[2], P // 4, image)


def test_the_two_heads_of_the_bench(capi, clean):
    for flags in (CONCURRENT, CONCURRENT | SPLIT2):
        assert capi.sparse_head_launch_text(64, 20, 20, 120, 80, flags) == want_line(64, 20, 120, 80, 4)
        assert capi.sparse_head_launch_text(64, 10, 10, 96, 80, flags) == want_line(64, 10, 96, 80, 2)
    assert "grid=104 " in want_line(64, 20, 120, 80, 4) and "grid=416 " in want_line(64, 20, 120, 80, 4)      # (the dense launch: 416 workgroups)


@pytest.mark.parametrize("flags,env", [(0, {}), (SPLIT2, {}), (KEEP_ALL, {}), (CONCURRENT | NO_FUSE, {}), (CONCURRENT | KEEP_ALL, {}), (CONCURRENT, {"FFGPU_SPARSE_HEAD": "0"}), (CONCURRENT, {"FFGPU_NO_FUSE": "1"})])
def test_switches_that_keep_the_dense_launch(capi, clean, flags, env):
    for k, v in env.items():
        clean.setenv(k, v)
    assert capi.sparse_head_launch_text(64, 20, 20, 120, 80, flags) == "dense pw_x3s"


def test_the_knob_and_other_kernels(capi, clean):
    for v in ("1", "2", ""):
        clean.setenv("FFGPU_SPARSE_HEAD", v)
        assert capi.sparse_head_launch_text(64, 20, 20, 120, 80, CONCURRENT).startswith("sparse ")
    # a layer AUTO does not give to k_conv_x3 keeps its kernel: small batches by default, k_conv_x3 switched off
    assert capi.sparse_head_launch_text(1, 20, 20, 120, 80, CONCURRENT).startswith("dense ") and "x3s" not in capi.sparse_head_launch_text(1, 20, 20, 120, 80, CONCURRENT)
    clean.setenv("FFGPU_PWX3S_MIN_WGS", "1")
    assert capi.sparse_head_launch_text(1, 20, 20, 120, 80, CONCURRENT).startswith("sparse box<1,4> ")
    clean.setenv("FFGPU_PW_X3S", "0")
    assert capi.sparse_head_launch_text(64, 20, 20, 120, 80, CONCURRENT).startswith("dense ")
    # eight waves per workgroup, one block per wave
    clean.delenv("FFGPU_PW_X3S")
    clean.setenv("FFGPU_IGX3_NW", "8")
    clean.setenv("FFGPU_IGX3_MT", "1")
    assert capi.sparse_head_launch_text(64, 20, 20, 120, 80, CONCURRENT) == want_line(64, 20, 120, 80, 1, 8)


def test_bad_arguments(capi, clean):
    with pytest.raises(RuntimeError, match="bad arguments"):
        capi.sparse_head_launch_text(0, 20, 20, 120, 80, 0)
    with pytest.raises(RuntimeError, match="bad arguments"):
        capi.sparse_head_launch_text(64, 20, 20, 120, 0, 0)
