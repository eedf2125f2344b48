"""CPU side of tests/irb_blocks: the table of cases is held to its purpose with the host-only planner probe, and the yardstick -- the fp32 reference chain
(the oracle's three groupconv calls and its shortcut) -- is held to the error criterion against the float64 restatement of the block before any kernel is.

  - every case plans onto its declared key under its switches;
  - the declared keys are exactly ffgpu_irb_instantiations(): a row added to a table of instantiations fails this test until it has its cases;
  - the structural conditions of irb_blocks/cases.py hold in the plan lines' own fields;
  - E_ref = max |chain - float64| meets E <= 8e-7 max |y| + 1e-6 for every case, and the non-finite cases hold every kind of value they are there for."""
import numpy as np
import pytest

from irb_blocks import blockref, cases
from irb_blocks.cases import CASES, fields


@pytest.fixture(scope="module")
def probe():
    from ffcnn_amd import capi
    capi.build_library()
    return capi.irb_plan_text


@pytest.fixture(scope="module")
def lines(probe):
    mp = pytest.MonkeyPatch()
    out = []
    try:
        for c in CASES:
            cases.set_switches(mp, c)
            out.append(cases.plan_line(probe, c))
    finally:
        mp.undo()
    return out


def test_every_case_plans_onto_its_key(lines):
    bad = [(c.id, line.split(" ")[0]) for c, line in zip(CASES, lines) if line.split(" ")[0] != c.key]
    assert not bad, bad


def test_the_keys_are_the_librarys_list():
    from ffcnn_amd import capi
    listed = capi.irb_instantiations()
    assert len(listed) == len(set(listed)) == 61
    for kind in ("tiny", "tiled"):
        declared = [c.key for c in CASES if c.kind == kind]
        assert sorted(declared) == sorted(listed), (kind, set(declared) ^ set(listed))
    assert {c.key for c in CASES} == set(listed)
    assert set(cases.FAMILIES) == {cases.family(k) for k in listed} and all(cases.family(k) == f for f, k in cases.FAMILIES.items())
    for key in cases.FAMILIES.values():
        assert sorted(c.acts for c in CASES if c.key == key and c.kind == "act") == sorted(cases.ACT_SETS)
        assert sorted(c.acts for c in CASES if c.key == key and c.kind == "relu") == sorted(cases.RELU_SETS)
        assert all(c.res for c in CASES if c.key == key and c.kind in ("act", "relu"))


def _tiles(f):
    """tile width and height in output pixels, tiles in x and y"""
    if f["key"].startswith("irb<"):
        return f["tile"][1], f["tile"][0], f["tiles"][0], f["tiles"][1]
    return 4 * f["tile"][0], f["tile"][1], f["tiles"][0], f["tiles"][1]


def test_structure_of_the_cases(lines):
    F = [fields(line) for line in lines]
    for c, f in zip(CASES, F):
        N, W, H, ic, ec, oc, stride = c.shape
        if c.kind == "tiny":
            assert N <= 2 and W <= 24 and H <= 24, c.id
        if c.kind != "tiled":
            continue
        assert N in (2, 3) and W <= 48 and H <= 48, c.id
        if c.key.startswith("thin<"):
            assert f["nbands"] >= 2 and H % f["band"] != 0, c.id
            continue
        tw, th, tx, ty = _tiles(f)
        assert tx >= 2 and ty >= 2 and f["OW"] % tw != 0 and f["OH"] % th != 0, (c.id, f["tile"], f["tiles"])
        assert ec > 32 and ec % 16 != 0 and oc % 16 != 0, c.id
        if c.key.startswith("irbw"):
            assert f["ngroups"] >= 3, c.id
        else:
            assert f["nchunks"] * f["ECH"] >= ec > 32, c.id
    tiled = [c for c in CASES if c.kind == "tiled"]
    assert sum(c.res for c in tiled) * 2 in (len(tiled), len(tiled) + 1, len(tiled) - 1)
    per_key = [(c, f) for c, f in zip(CASES, F) if c.kind in ("tiny", "tiled", "tiny-nf")]
    # single-strip wave rows: the half form of the last group (ec % 16 in 1..8) and the full form
    single = [(c, f) for c, f in per_key if c.key.startswith("irbw<")]
    assert {f["half"] for c, f in single} == {0, 1}
    assert all(f["half"] == (1 <= c.shape[4] % 16 <= 8) for c, f in single)
    # the waves of a tile: one wave per tile with a tile count that is no multiple of WPB; the group split with the partial sums side by side and folded
    wave = [(c, f) for c, f in per_key if c.key.startswith("irbw")]
    assert any(f["G"] == 1 and f["tiles"][2] % f["WPB"] != 0 for c, f in wave)
    assert any(f["G"] > 1 and "FFGPU_IRBW_FOLD" not in c.env for c, f in wave)
    assert any(f["G"] > 1 and c.env.get("FFGPU_IRBW_FOLD") == "1" for c, f in wave)
    # workgroup rows: every channel-loop split, one chunk / two streamed buffers / resident chunks (more than two), several frames per tile, both chunk sizes
    wg = [f for c, f in per_key if c.key.startswith("irb<")]
    assert {f["KS"] for f in wg} == {1, 2, 4}
    assert any(f["nchunks"] == 1 for f in wg) and any(f["nchunks"] > 1 and not f["resident"] for f in wg) and any(f["nchunks"] > 2 and f["resident"] for f in wg)
    assert any(f["tile"][3] > 1 for f in wg)
    assert {f["ECH"] for f in wg} == {16, 32}


@pytest.mark.parametrize("i", range(len(CASES)), ids=cases.IDS)
def test_reference_chain_meets_the_criterion(i):
    """the yardstick before it is used: the chain's own error against float64 passes the absolute part of the criterion, and a kernel exactly as good as the
    chain would pass the relative part"""
    c, r = CASES[i], cases.reference(i)
    y32, y64 = r["y32"], r["y64"]
    assert np.array_equal(np.isnan(y32), np.isnan(y64)) and np.array_equal(np.isinf(y32), np.isinf(y64))
    assert np.array_equal(y32[np.isinf(y32)], y64[np.isinf(y32)].astype(np.float32))
    assert r["E_ref"] <= 8e-7 * r["ymax"] + 1e-6, (r["E_ref"], r["ymax"])
    assert blockref.criterion(r["E_ref"], r["E_ref"], r["ymax"])
    if c.kind != "relu":
        assert r["ok"].all()
        return
    # every kind of value the case is there for: NaN and -Inf survive a linear shortcut only; relu turns them into exact zeros
    assert r["ok"].any() and np.isposinf(y32).any()
    if c.acts[3] == 0:
        assert np.isnan(y32).any() and np.isneginf(y32).any()
    else:
        assert not np.isnan(y32).any() and not np.isneginf(y32).any() and (y32 == 0).any()
