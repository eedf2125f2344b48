"""Which form the launch of the stride-2 block 4 -> 24 -> 8 takes (ffgpu_irb_s2_launch_text: thin_s2_form in ffgpu_conv_kernels.inc, pure host arithmetic),
without a GPU: the streaming form's frames per wave, band, tasks and grid against a restatement of the rule, the planned key where the launch follows the
plan, both knobs, and the planned line (ffgpu_irb_plan_text), which the form must never change."""
import pytest

from irb_blocks import cases

CONCURRENT = 64                                                # FFGPU_CONCURRENT (include/ffcnn_hip.h)
NC = 3                                                         # output columns per lane
WAVES = 640                                                    # THIN_S2_WAVES: the band doubles while the launch keeps that many waves
BATCHES = (1, 2, 3, 64)
WIDTHS = (16, 156, 158, 160, 200)
BLOCK = (4, 24, 8, 2, 2, 2, 0, 0)                              # ic, ec, oc, stride, act1, actd, act2, res_act


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


def want_band(groups, OH):
    """the longest of 2, 4, 8, 16 output rows that still leaves WAVES waves (groups * OH / band >= WAVES at every doubling)"""
    band = 2
    for b in (4, 8, 16):
        if groups * OH >= WAVES * b:
            band = b
        else:
            break
    return band


def want_line(N, W, H, flags, knob, band_knob, block=BLOCK):
    """the streaming form's line, or None where the rule keeps the planned kernel"""
    ic, ec, oc, stride = block[:4]
    OW, OH = (W - 1) // 2 + 1, (H - 1) // 2 + 1
    lanes = len(range(0, OW, NC))
    if not ((ic, ec, oc, stride) == (4, 24, 8, 2) and W % 2 == 0 and OW >= NC and lanes <= 32 and N >= 2 and flags == CONCURRENT and knob != 0 and 3 not in block[4:7]):
        return None
    frames = 64 // lanes
    groups = len(range(0, N, frames))
    band = band_knob if band_knob else want_band(groups, OH)
    nbands = len(range(0, OH, band))
    tasks = groups * nbands
    return "thin_s2<4,24,8,3> frames=%d band=%d tasks=%d grid=%d block=256 W=%d H=%d N=%d lanes=%d nbands=%d" % (frames, band, tasks, len(range(0, tasks, 4)), W, H, N, lanes, nbands)


def check(capi, N, W, H, flags, knob, band_knob, block=BLOCK):
    shape = (N, W, H) + block
    plan = capi.irb_plan_text(shape, flags)
    line = capi.irb_s2_launch_text(shape, flags)
    want = want_line(N, W, H, flags, knob, band_knob, block)
    if want is not None:
        assert plan != "unsupported" and not plan.startswith("thin<"), (shape, plan)
        assert line == want, (shape, flags, knob, band_knob, line, want)
        return "s2"
    if plan == "unsupported":
        assert line == "unsupported", (shape, line)
        return "none"
    p = cases.fields(plan)
    f = cases.fields(line)
    assert f["key"] == p["key"] and f["grid"] == p["grid"] and f["block"] == p["block"], (shape, line, plan)      # the launch follows the plan
    return "plan"


def test_the_rule(capi, clean):
    seen = {"s2": 0, "plan": 0, "none": 0}
    for N in BATCHES:
        for W in WIDTHS:
            for H in (4, 5, 6, 7, 160):
                for flags in (0, CONCURRENT):
                    got = check(capi, N, W, H, flags, 1, 0)
                    seen[got] += 1
                    assert (got == "s2") == (N >= 2 and W != 200 and flags == CONCURRENT), (N, W, H, flags, got)
    assert seen["s2"] >= 40 and seen["plan"] >= 40, seen
    # other blocks keep their plan: another channel count, stride 1, an odd width, a block the thin family takes
    for block in [(8, 32, 8, 2, 2, 2, 0, 0), (4, 24, 8, 1, 2, 2, 0, 0), (4, 24, 4, 2, 2, 2, 0, 0), (4, 8, 4, 1, 2, 2, 0, 0), (3, 24, 8, 2, 2, 2, 0, 0)]:
        assert check(capi, 64, 160, 160, CONCURRENT, 1, 0, block) == "plan", block
    assert check(capi, 2, 159, 7, CONCURRENT, 1, 0) == "plan"
    assert check(capi, 2, 4, 4, CONCURRENT, 1, 0) == "plan"                                          # two output columns: fewer than a lane's three
    assert check(capi, 2, 6, 4, CONCURRENT, 1, 0) == "s2"
    for acts in [(1, 1, 0, 0), (1, 2, 1, 0), (0, 0, 2, 0)]:
        assert check(capi, 2, 160, 6, CONCURRENT, 1, 0, (4, 24, 8, 2) + acts) == "s2"


def test_the_flagship_block(capi, clean):
    """layers 9-11 at batch 64: 27 lanes per row, two frames per wave, 32 groups"""
    shape = (64, 160, 160) + BLOCK
    assert capi.irb_s2_launch_text(shape, CONCURRENT) == "thin_s2<4,24,8,3> frames=2 band=4 tasks=640 grid=160 block=256 W=160 H=160 N=64 lanes=27 nbands=20"
    assert capi.irb_s2_launch_text(shape, 0).startswith("irbw<1,1,2,3")
    assert capi.irb_plan_text(shape, CONCURRENT).startswith("irbw<1,1,2,3")
    assert capi.irb_s2_launch_text((2, 16, 4) + BLOCK, CONCURRENT).startswith("thin_s2<4,24,8,3> frames=21 ")
    assert capi.irb_s2_launch_text((2, 200, 4) + BLOCK, CONCURRENT).startswith("irbw<1,1,2,")
    assert capi.irb_s2_launch_text((1, 160, 6) + BLOCK, CONCURRENT).startswith("irbw<1,1,2,")


@pytest.mark.parametrize("s2_knob", ["0", "1", "2", "", None])
def test_the_knobs(capi, clean, s2_knob):
    """FFGPU_THIN_S2 (0: never; unset, empty or anything else: where the rule says) and FFGPU_THIN_S2_BAND; the planned line never moves"""
    plans = {}
    for flags in (0, CONCURRENT):
        for N in BATCHES:
            for W in WIDTHS:
                plans[(flags, N, W)] = capi.irb_plan_text((N, W, 7) + BLOCK, flags)
    if s2_knob is not None:
        clean.setenv("FFGPU_THIN_S2", s2_knob)
    knob = int(s2_knob) if s2_knob else 1
    for band_knob in (0, 1, 3, 5, 16, 200):
        if band_knob:
            clean.setenv("FFGPU_THIN_S2_BAND", str(band_knob))
        for N in BATCHES:
            for W in WIDTHS:
                for H in (4, 7, 160):
                    got = check(capi, N, W, H, CONCURRENT, knob, band_knob)
                    assert got == ("s2" if knob and N >= 2 and W != 200 else "plan"), (N, W, H, got)
                    assert check(capi, N, W, H, 0, knob, band_knob) == "plan"
        for key, plan in plans.items():
            assert capi.irb_plan_text((key[1], key[2], 7) + BLOCK, key[0]) == plan, key
    # the thin family's band knob is not this form's
    clean.delenv("FFGPU_THIN_S2_BAND", raising=False)
    clean.setenv("FFGPU_THIN_BAND", "5")
    assert check(capi, 64, 160, 160, CONCURRENT, knob, 0) == ("s2" if knob else "plan")
