"""Which form the launch of a thin block takes (ffgpu_irb_thin_launch_text: thin_form in ffgpu_conv_kernels.inc, pure host arithmetic), without a GPU: the
columns per lane, the band, the tasks and the grid of the paired form against a brute-force restatement for every width 4..256 and batch 1..65, and the
single form's line against the planned one (ffgpu_irb_plan_text, which the form must not change)."""
import pytest

from irb_blocks import cases

CONCURRENT = 64                                                # FFGPU_CONCURRENT (include/ffcnn_hip.h)
CHANNELS = [(4, 4), (8, 4), (4, 8), (8, 8)]


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


def want_ncp(W, ic):
    """the fewest of 3, 4, 5 columns per lane that divide the row and put it into 32 lanes; five columns of 8 input channels are not built"""
    fits = [nc for nc in (3, 4, 5) if any(nc * lanes == W for lanes in range(1, 33))]
    if not fits or (fits[0] == 5 and ic == 8):
        return 0
    return fits[0]


def want_band(units, H):
    """thin_band's rule: the longest of 2, 4, 8, 16 rows that still leaves about 640 waves (units * H / band >= 640 at every doubling)"""
    band = 2
    for b in (4, 8, 16):
        if units * H >= 640 * b:
            band = b
        else:
            break
    return band


def want_pair_line(N, W, H, ic, oc, ncp, band):
    pairs = len(range(0, N, 2))
    nbands = len(range(0, H, band))
    ntasks = pairs * nbands
    return "thin_pair<%d,8,%d,%d> W=%d H=%d N=%d band=%d nbands=%d ntasks=%d grid=%d block=256" % (ic, oc, ncp, W, H, N, band, nbands, ntasks, len(range(0, ntasks, 4)))


def check(capi, N, W, H, ic, oc, flags, pair_knob, band_knob):
    shape = (N, W, H, ic, 8, oc, 1, 2, 2, 0, 0)
    plan = capi.irb_plan_text(shape, flags)
    line = capi.irb_thin_launch_text(shape, flags)
    if not plan.startswith("thin<"):
        assert line == "unsupported", (shape, plan, line)
        return "other"
    p = cases.fields(plan)
    ncp = want_ncp(W, ic)
    if ncp and N >= 2 and flags == CONCURRENT and pair_knob != 0:
        band = band_knob if band_knob else want_band(len(range(0, N, 2)), H)
        assert line == want_pair_line(N, W, H, ic, oc, ncp, band), (shape, line)
        assert band_knob or band <= p["band"], "half the units never ask for a longer band"
        return "pair"
    # the single form: the planned band, tasks and grid, from the launch's own arithmetic
    assert line == "thin<%d,8,%d> W=%d H=%d N=%d band=%d nbands=%d ntasks=%d grid=%d block=256" % (ic, oc, W, H, N, p["band"], p["nbands"], p["ntasks"], p["grid"]), (shape, line, plan)
    assert p["ntasks"] == N * len(range(0, H, p["band"])) and p["grid"] == len(range(0, p["ntasks"], 4))
    return "single"


def test_every_width_and_batch(capi, clean):
    seen = {"pair": 0, "single": 0, "other": 0}
    ncps = set()
    for W in range(4, 257):
        for N in range(1, 66):
            H = (7 * W + 3 * N) % 160 + 1
            ic, oc = CHANNELS[(W + N) % 4]
            for flags in (0, CONCURRENT):
                seen[check(capi, N, W, H, ic, oc, flags, 1, 0)] += 1
            ncps.add(want_ncp(W, ic))
    assert ncps == {0, 3, 4, 5} and min(seen.values()) > 1000, seen


def test_the_flagship_block(capi, clean):
    """layers 4-8 at batch 64: five columns, 32 pairs, band 8 -- the 640 waves the single form's band 16 gives 64 frames"""
    shape = (64, 160, 160, 4, 8, 4, 1, 2, 2, 0, 0)
    assert capi.irb_thin_launch_text(shape, CONCURRENT) == "thin_pair<4,8,4,5> W=160 H=160 N=64 band=8 nbands=20 ntasks=640 grid=160 block=256"
    assert capi.irb_thin_launch_text(shape, 0) == "thin<4,8,4> W=160 H=160 N=64 band=16 nbands=10 ntasks=640 grid=160 block=256"
    assert capi.irb_plan_text(shape, CONCURRENT) == capi.irb_plan_text(shape, 0)
    # 8 input channels at five columns: not built (it spills), the single form stays
    assert capi.irb_thin_launch_text((64, 160, 160, 8, 8, 4, 1, 2, 2, 0, 0), CONCURRENT).startswith("thin<8,8,4> ")
    assert capi.irb_thin_launch_text((64, 128, 160, 8, 8, 4, 1, 2, 2, 0, 0), CONCURRENT).startswith("thin_pair<8,8,4,4> ")
    assert capi.irb_thin_launch_text((2, 164, 5, 4, 8, 4, 1, 2, 2, 0, 0), CONCURRENT).startswith("thin<4,8,4> ")
    assert capi.irb_thin_launch_text((1, 160, 5, 4, 8, 4, 1, 2, 2, 0, 0), CONCURRENT).startswith("thin<4,8,4> ")
    assert capi.irb_thin_launch_text((64, 20, 20, 24, 136, 24, 1, 2, 2, 0, 0), CONCURRENT) == "unsupported"


@pytest.mark.parametrize("pair_knob", ["0", "1", "2", ""])
def test_the_knobs(capi, clean, pair_knob):
    """FFGPU_THIN_PAIR (0: never; unset, empty or anything else: where the rule says) and FFGPU_THIN_BAND, which both forms obey; the planned line never moves"""
    clean.setenv("FFGPU_THIN_PAIR", pair_knob)
    knob = int(pair_knob) if pair_knob else 1
    for band_knob in (0, 1, 3, 5, 16, 200):
        if band_knob:
            clean.setenv("FFGPU_THIN_BAND", str(band_knob))
        for N, W, H in [(2, 160, 5), (3, 20, 7), (3, 140, 7), (2, 12, 4), (2, 128, 3), (2, 164, 5), (1, 160, 5), (64, 160, 160), (33, 160, 160), (65, 96, 31)]:
            for ic, oc in CHANNELS:
                got = check(capi, N, W, H, ic, oc, CONCURRENT, knob, band_knob)
                assert got == ("pair" if knob and N >= 2 and want_ncp(W, ic) else "single")
                assert check(capi, N, W, H, ic, oc, 0, knob, band_knob) == "single"
    clean.delenv("FFGPU_THIN_BAND", raising=False)
    a = capi.irb_plan_text((64, 160, 160, 4, 8, 4, 1, 2, 2, 0, 0), CONCURRENT)
    clean.delenv("FFGPU_THIN_PAIR")
    assert a == capi.irb_plan_text((64, 160, 160, 4, 8, 4, 1, 2, 2, 0, 0), CONCURRENT)
