"""Where the planner merges a run of small-plane fused blocks into one stage launch (ffgpu_plan.hpp: ffgpu_layout_stage; ffgpu_irb_stage.inc), on the CPU.

Two probes, neither needs a device.  The layout pass through the sanitizer driver (`make -C ffcnn_amd/csrc plan`, san/plan_driver.cc with its optional
seventh argument `stage`): which runs merge on the layer table alone, that the tensors inside a run get no arena range and cannot be read back
(canon -3, not readable: what ffgpu_exec_read_layer refuses as "not materialised", exactly as the inside of a fused block), and the layout's invariants
I1 - I6 on the cfg corpus with the merge on.  And ffgpu_irb_stage_plan_text: what an executor of a given batch and flags does with a run -- the
conditions that are the executor's own (FFGPU_CONCURRENT, 32 frames, FFGPU_IRB_STAGE, FFGPU_KEEP_ALL, FFGPU_NO_FUSE) and the kernel's (the plane)."""
import os
import subprocess

import pytest

from conftest import ROOT
from irb_stage import nets
from test_host_sanitizer import _cfgs, YCFG
from test_irb_choice import knob_names

CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
BIN = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_plan_san")
KEEP_ALL, NO_FUSE, CONCURRENT = 1, 8, 64


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")

    def run(cfg, batch=64, flags=0, stage=1, take="all", branch=0):
        r = subprocess.run([BIN, cfg] + [str(x) for x in (batch, flags, take, 0, branch, stage)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
        out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "VIOLATION" not in out, "%s -> rc %d\n%s\n%s" % (cfg, r.returncode, out[-2000:], err[-3000:])
        lines = out.strip().split("\n")
        rows = [l.split() for l in lines if l and l[0].isdigit() and len(l.split()) == 8]
        return {int(r[0]): r for r in rows}, [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("stage ")]
    return run


@pytest.fixture
def probe(monkeypatch):
    from ffcnn_amd import capi
    capi.lib()
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)
    return capi.irb_stage_plan_text


def write(tmp_path, text):
    p = str(tmp_path / "run.cfg")
    open(p, "w").write(text)
    return p


def net(W, H, blocks):
    return "[net]\nwidth=%d\nheight=%d\nchannels=%d\n\n" % (W, H, nets.IC) + nets.conv(nets.IC, 1, "linear", groups=nets.IC) + "".join(blocks)


def test_yolo_fastest_merges_layers_84_to_108(plan, probe):
    rows, stages = plan(YCFG, 64, 0, 1)
    assert stages == [(84, 106, 5)]                              # first layer of the first block, last conv of the last one (its shortcut is layer 108), five blocks
    for i in range(84, 106):                                     # nothing inside the run has a tensor: no arena range, not readable
        assert rows[i][1] == "-3" and rows[i][2] == "0" and rows[i][3:] == ["-"] * 5, rows[i]
    assert rows[108][1] == "108" and rows[108][2] == "1" and rows[83][1] == "83" and int(rows[83][4]) >= 106      # the run's input lives until its one launch
    rows0, stages0 = plan(YCFG, 64, 0, 0)
    assert stages0 == [] and rows0[88][1] == "88" and rows0[88][2] == "1"
    # the executor's side: four chains of 64 frames merge, a single chain does not
    assert probe(64, 10, 10, 5, 2, 2, CONCURRENT).startswith("stage B=5 launches=1 N=64 H=10 W=10 ")
    assert probe(64, 10, 10, 5, 2, 2, 0) == "blocks B=5 launches=5"


def test_the_executors_own_conditions(probe, monkeypatch):
    assert probe(32, 10, 10, 5, 2, 2, CONCURRENT).startswith("stage ")
    assert probe(31, 10, 10, 5, 2, 2, CONCURRENT).startswith("blocks ")
    assert probe(64, 10, 10, 5, 2, 2, CONCURRENT | KEEP_ALL).startswith("blocks ")
    assert probe(64, 10, 10, 5, 2, 2, CONCURRENT | NO_FUSE).startswith("blocks ")
    assert probe(64, 10, 10, 1, 2, 2, CONCURRENT).startswith("blocks ")                  # a run is at least two blocks
    monkeypatch.setenv("FFGPU_IRB_STAGE", "0")
    assert probe(64, 10, 10, 5, 2, 2, CONCURRENT).startswith("blocks ")
    monkeypatch.setenv("FFGPU_IRB_STAGE", "1")
    assert probe(64, 10, 10, 5, 2, 2, CONCURRENT).startswith("stage ")


def test_planes_the_kernel_holds(probe):
    """at most 128 pixels in at most 32 quads of a row, and the whole of it in 160 KB of LDS"""
    for w, h, ok in ((10, 10, True), (9, 7, True), (12, 10, True), (4, 4, True), (16, 8, True), (12, 11, False), (9, 14, False), (20, 20, False)):
        line = probe(64, w, h, 5, 2, 2, CONCURRENT)
        assert line.startswith("stage " if ok else "blocks "), (w, h, line)
        if ok:
            f = dict(t.split("=") for t in line.split()[1:])
            assert int(f["lds"]) <= 160 * 1024 and int(f["grid"]) == 64 and int(f["block"]) == 448
            assert int(f["lds"]) == 4 * (int(f["f_off"]) + 48 * w * h) and int(f["e_slice"]) >= 16 * int(f["EP"]) and int(f["e_slice"]) >= 2048


def test_layout_flags_switch_the_merge_off(plan):
    for flags in (KEEP_ALL, NO_FUSE):
        assert plan(YCFG, 64, flags, 1)[1] == []
    assert plan(YCFG, 64, 0, 1, take="none")[1] == []            # (the kernels refuse: no fused block, no run)


def test_a_second_reader_ends_the_run(plan, tmp_path):
    """three blocks, and a route behind them that reads the FIRST block's output (layer 5): that tensor must exist, so the run starts behind it"""
    text = net(10, 10, [nets.block(2, 2)] * 3) + "[route]\nlayers=5\n\n" + nets.conv(8, 1, "linear")
    rows, stages = plan(write(tmp_path, text))
    assert stages == [(6, 13, 2)]
    assert rows[5][1] == "5" and rows[5][2] == "1" and rows[10][1] == "-3"
    rows, stages = plan(write(tmp_path, net(10, 10, [nets.block(2, 2)] * 3) + nets.conv(8, 1, "linear")))
    assert stages == [(1, 13, 3)]


def test_a_block_of_another_shape_ends_the_run(plan, tmp_path):
    """two blocks, one with 96 expanded channels, two more: two runs of two; and a run is cut where the activations change"""
    blocks = [nets.block(2, 2)] * 2 + [nets.block(2, 2, ec=96)] + [nets.block(2, 2)] * 2
    rows, stages = plan(write(tmp_path, net(10, 10, blocks)))
    assert stages == [(1, 8, 2), (16, 23, 2)]
    assert rows[15][1] == "15" and rows[15][2] == "1"            # the odd block's output exists
    rows, stages = plan(write(tmp_path, net(10, 10, [nets.block(2, 2)] * 2 + [nets.block(1, 1)] * 2)))
    assert stages == [(1, 8, 2), (11, 18, 2)]
    # a shortcut that is not linear, or comes from somewhere else than the block's own input, is not the stage's
    relu_sc = nets.block(2, 2).replace("[shortcut]\nfrom=-5\nactivation=linear", "[shortcut]\nfrom=-5\nactivation=leaky")
    assert plan(write(tmp_path, net(10, 10, [relu_sc] * 3)))[1] == []
    far = nets.block(2, 2) + nets.block(2, 2, frm=-10) + nets.block(2, 2)
    assert plan(write(tmp_path, net(10, 10, [far])))[1] == []


def test_a_plane_above_128_pixels_is_not_merged(plan, tmp_path):
    assert plan(write(tmp_path, net(12, 11, [nets.block(2, 2)] * 3)))[1] == []
    assert plan(write(tmp_path, net(9, 14, [nets.block(2, 2)] * 3)))[1] == []          # 126 pixels in 42 row quads
    assert plan(write(tmp_path, net(16, 8, [nets.block(2, 2)] * 3)))[1] == [(1, 13, 3)]


def test_corpus_keeps_the_invariants_with_the_merge_on(plan):
    for cfg in _cfgs():
        for batch, flags, branch in ((1, 0, 0), (64, 0, 0), (64, 0, 1), (33, KEEP_ALL, 0), (64, NO_FUSE, 1)):
            plan(cfg, batch, flags, 1, branch=branch)             # (the fixture asserts: no violation, no sanitizer report)
