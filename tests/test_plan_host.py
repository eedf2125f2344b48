"""ffcnn_amd/csrc/ffgpu_plan.hpp -- the executor planner's layout pass: aliases, fused blocks, concat in place, lifetimes, the side lane, arena offsets --
on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C ffcnn_amd/csrc plan`).  The driver (san/plan_driver.cc) loads a cfg through
the host parser and the stub device side, lays the net out, prints the layout and checks its invariants itself (I1 no two tensors that are
live together share arena space, I2 concat children tile their parent, I3 reads and writes fall inside lifetimes, I4 offsets and bounds, I5 the side
lane's tensors are never handed on): exit code 1 names the invariant and the layers.  Every cfg of the corpus runs at batches 1, 2, 3 x flags 0, KEEP_ALL,
NO_FUSE x the callables taking every candidate block or none x dwpw x branch.  A sanitizer report aborts the child: the test fails with it."""
import itertools
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT
from test_host_sanitizer import _CONV, _HOSTILE, _NET, _cfgs, mutated_cfgs, YCFG

CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
BIN = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_plan_san")
KEEP_ALL, NO_FUSE = 1, 8                                         # FFGPU_KEEP_ALL, FFGPU_NO_FUSE
COMBOS = list(itertools.product((1, 2, 3), (0, KEEP_ALL, NO_FUSE), ("none", "all"), (0, 1), (0, 1)))      # batch, flags, callables, dwpw, branch


@pytest.fixture(scope="module")
def plan():
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")

    def run(cfg, batch=1, flags=0, take="all", dwpw=0, branch=0):
        r = subprocess.run([BIN, cfg] + [str(x) for x in (batch, flags, take, dwpw, branch)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
        out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "VIOLATION" not in out, \
            "%s %s -> rc %d\n%s\n%s" % (cfg, (batch, flags, take, dwpw, branch), r.returncode, "\n".join(l for l in out.split("\n") if "VIOLATION" in l)[:2000], err[-3000:])
        return out
    return run


def sweep(plan, cfg):
    """every combination on one cfg; the outputs in COMBOS order"""
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda c: plan(cfg, *c), COMBOS))


def layout(out):
    """the driver's output: ([(layer, canon, readable, first, last, root, offset, size) or (layer, canon, readable)], (side_lo, side_hi, arena), counts)"""
    lines = out.strip().split("\n")
    rows = [tuple(int(x) for x in l.split() if x != "-") for l in lines[:-2]]
    words = lines[-1].split()
    return rows, tuple(int(x) for x in lines[-2].split()), {words[k]: int(words[k + 1]) for k in range(0, len(words), 2)}


def test_repo_cfgs(plan):
    for cfg in _cfgs():
        outs = sweep(plan, cfg)
        assert all(o.strip().split("\n")[-1].startswith("fused_into ") for o in outs), cfg      # every one of them is laid out
        for combo, out in zip(COMBOS, outs):
            rows, (side_lo, side_hi, arena), counts = layout(out)
            batch, flags, take, dwpw, branch = combo
            if flags & NO_FUSE:                                  # nothing aliased into a route's tensor, nothing absorbed, no block, no lane
                assert all(r[5] == r[1] for r in rows if len(r) > 3) and counts == {"fused_into": 0, "irb": 0, "dwpw": 0, "inplace": 0}, (cfg, combo)
                assert (side_lo, side_hi) == (-1, -1)
            if flags & KEEP_ALL:                                 # every root has a range of its own, rounded up to 64 floats
                roots = {r[5] for r in rows if len(r) > 3}
                size = {r[0]: r[7] for r in rows if len(r) > 3 and r[1] == r[0]}
                assert arena == max(64, sum((size[t] + 63) // 64 * 64 for t in roots)), (cfg, combo)
            if take == "none" or not dwpw:
                assert counts["dwpw"] == 0
            if take == "none":
                assert counts["irb"] == 0
            if not branch:
                assert (side_lo, side_hi) == (-1, -1)


def test_yolo_fastest_side_lane_and_blocks(plan):
    """read off data/yolo-fastest-1.1.cfg: the first [yolo] is layer 121 and the [route] behind it (layers = -7) goes back to layer 115, so layers
    116 .. 121 are the side lane; the net has 24 expand / depthwise / project triples, 18 of them in front of a shortcut, and two two-source routes"""
    for batch in (1, 2, 3):
        for flags in (0, KEEP_ALL):
            rows, side, counts = layout(plan(YCFG, batch, flags, "all", 0, 1))
            assert side[:2] == (116, 121)
            assert counts == {"fused_into": 18, "irb": 24, "dwpw": 0, "inplace": 2}
            assert [r[1] for r in rows[119:123]] == [119, 120, -2, 115]
            last = {r[1]: r[4] for r in rows if len(r) > 3}
            assert all(last[t] == 132 for t in last if t >= 115)                    # born behind the fork, or read by the lane: live to the end (L + 1)
        assert layout(plan(YCFG, batch, NO_FUSE, "all", 0, 1))[1][:2] == (-1, -1)
        rows, _, counts = layout(plan(YCFG, batch, 0, "all", 1, 0))
        assert counts["dwpw"] > 0 and sum(1 for r in rows if r[1] == -3) == 2 * counts["irb"] + counts["dwpw"]


def test_layer_op_cfgs(plan, tmp_path):
    from layer_ops import cfgs
    for g in cfgs.every_cfg():
        p = str(tmp_path / "op.cfg")
        open(p, "w").write(g.cfg_text())
        outs = sweep(plan, p)
        assert all("fused_into " in o for o in outs), g.name


@pytest.mark.parametrize("name", sorted(_HOSTILE))
def test_hostile_cfgs(plan, tmp_path, name):
    p = str(tmp_path / "h.cfg")
    open(p, "wb").write(_HOSTILE[name].encode("latin-1"))
    outs = sweep(plan, p)
    assert all("net_load: NULL" in o or "layout: refused" in o or "fused_into " in o for o in outs)


def test_route_of_two_plane_sizes_is_refused(plan, tmp_path):
    """What the seeded mutations turned up (a damaged stride in front of a route): a route whose sources have planes of different sizes gets the last
    source's plane from the parser, so its sources -- copied or placed behind each other -- ran past its end, into whatever tensor follows it in the
    arena (I2).  The layout refuses such a net, fused or not."""
    p = str(tmp_path / "planes.cfg")
    open(p, "w").write(_NET + _CONV + "[maxpool]\nsize=2\nstride=2\n\n" + "[route]\nlayers=-1,-2\n\n" + _CONV)
    for out in sweep(plan, p):
        assert out == "layout: refused (route 2: source layer 1 is 32 x 32, the route 64 x 64)\n"


def test_seeded_mutations_of_the_real_cfg(plan, tmp_path):
    for it, text in enumerate(mutated_cfgs()):
        p = str(tmp_path / "m.cfg")
        open(p, "w").write(text)
        outs = sweep(plan, p)
        assert all("net_load: NULL" in o or "layout: refused" in o or "fused_into " in o for o in outs), "mutation %d" % it
