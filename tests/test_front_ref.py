"""CPU side of tests/front: the table of cases and the yardsticks of k_front's tests are held to their purpose before the kernel is.

  - the table covers the list of tests/front/cases.py's docstring -- asserted from the table's own geometry, not from its comments;
  - every case's probe line (ffgpu_front_plan_text, host code) is the line the rule gives: NC = 3 iff the knob says 3, W >= 6 and (W + 2) / 3 <= 64; band, nbands,
    ntasks and grid as the launch computes them; the resizing forms "staged" at four columns per lane;
  - the oracle's chain stays within frontref.bound (derived, not measured) against front64 for every case and meets the criterion the kernel is held to: a wrong
    bound or a wrong front64 shows here.  Its worst share of the bound is printed;
  - part 3: the touched set of the geometry IS the set of non-finite outputs of front64 under linear activations, NaN, +Inf and -Inf all occur there, every kind of
    placement is planted, outputs are left untouched, and the oracle agrees with front64 on every NaN and Inf;
  - frontref.u8_input is the oracle's net_input for frames of the net's size."""
import numpy as np
import pytest

from front import cases, frontref
from front.cases import CASES, NF_CASES, FORM_CASES
from irb_blocks import blockref


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi
    capi.build_library()
    return capi


def test_the_table_covers_the_list():
    g = {c.id: cases.geometry(c) for c in CASES}               # NC, lpr, sl, band, nbands, ntasks, grid
    nc3 = {c.W: g[c.id] for c in CASES if g[c.id][0] == 3}
    nc4 = {c.W: g[c.id] for c in CASES if g[c.id][0] == 4}
    assert set(nc3) >= {8, 12, 16, 44, 48, 52, 184, 188, 192} and set(nc4) >= {4, 8, 64, 68, 196, 256}
    assert [nc3[W][1:3] for W in (8, 12, 16, 44, 48, 52, 184, 188, 192)] == [(3, 1), (4, 0), (6, 2), (15, 1), (16, 0), (18, 2), (62, 2), (63, 1), (64, 0)]
    assert [nc4[W][1] for W in (4, 8, 64, 68, 196, 256)] == [1, 2, 16, 17, 49, 64]
    assert any(c.W == 4 and c.nc == 3 for c in CASES) and any(c.W == 196 and c.nc is None for c in CASES)      # the rule, not the knob, says 4
    assert any(c.W == 8 and c.nc == 4 for c in CASES)                                                          # the knob says 4 where the rule would take 3
    bands = {(c.H, g[c.id][3]) for c in CASES}
    assert any(H == 1 for H, _ in bands) and any(H < b for H, b in bands) and any(H == b for H, b in bands) and any(H == b + 1 for H, b in bands)
    assert {c.band for c in CASES} >= {1, 2, 3, 16, None}
    lengths = {min(b, H - k * b) for H, b in bands for k in range(-(-H // b))}
    assert any(n % 2 for n in lengths) and any(n % 2 == 0 for n in lengths)
    assert any(g[c.id][5] % 4 for c in CASES) and any(g[c.id][4] > 1 and c.N > 1 for c in CASES)
    assert all(c.H <= 9 and c.N <= 5 for c in CASES + NF_CASES)
    for slot in range(4):
        assert {c.acts[slot] for c in CASES} == {0, 1, 2}, slot
        assert {c.acts[slot] for c in NF_CASES} == {0, 1, 2}, slot
    assert {cases.geometry(c)[0] for c in NF_CASES} == {3, 4} and {cases.geometry(c)[2] for c in NF_CASES} == {0, 1, 2}
    assert {cases.geometry(c)[2] for c in FORM_CASES if c.nc == 3} == {0, 1, 2} and {c.nc for c in FORM_CASES} == {3, 4}
    assert all(cases.geometry(c)[0] == c.nc for c in FORM_CASES)
    assert cases.MEAN != (0.0, 0.0, 0.0) and min(cases.NORM) < 0 < max(cases.NORM)


def test_scale_and_bias():
    _, f0, f1, fd, f2 = cases.make_inputs(CASES[0])
    sc = np.concatenate([f0[:, 28], f1[:, 8], fd[:, 12], f2[:, 8]])
    assert (f0[:, 28] < 0).sum() == 2 and (f0[:, 28] == 0).sum() == 1 and (fd[:, 12] == 0).sum() == 1 and (sc < 0).sum() == 5 and (sc > 0).sum() == 21
    _, f0, f1, fd, f2 = cases.make_inputs(NF_CASES[0], nf=True)
    assert (f0[:, 28] != 0).all() and (f1[:, 8] != 0).all() and (fd[:, 12] != 0).all() and (f2[:, 8] == 0).sum() == 1 and (f0[:, 28] < 0).sum() == 2


def test_probe_follows_the_rule(capi):
    mp = pytest.MonkeyPatch()
    bad = []
    try:
        for c in CASES + NF_CASES + FORM_CASES:
            cases.set_switches(mp, c)
            for form in capi.FRONT_FORMS:
                got, want = cases.plan_line(capi.front_plan_text, c, form), cases.want_line(c, form)
                if got != want:
                    bad.append((c.id, form, got, want))
        # the rule itself, over every width the kernel takes and each setting of the knob
        for knob in (None, 3, 4, 5):
            c0 = cases.Case("rule", 2, 8, 4, knob, None, (2, 2, 2, 0), 0)
            for W in range(4, 260, 4):
                c = c0._replace(W=W)
                cases.set_switches(mp, c)
                want = 3 if knob in (None, 3) and W >= 6 and (W + 2) // 3 <= 64 else 4
                assert cases.nc_rule(knob, W) == want
                line = cases.plan_line(capi.front_plan_text, c)
                if line != cases.want_line(c) or not line.startswith("front<4,0,%d,0,0> " % want):
                    bad.append((knob, W, line))
    finally:
        mp.undo()
    assert not bad, bad[:4]
    assert capi.front_plan_text(1, 7, 4) == "unsupported" and capi.front_plan_text(1, 260, 4) == "unsupported"
    with pytest.raises(RuntimeError, match="bad arguments"):
        capi.front_plan_text(0, 8, 4)


@pytest.mark.parametrize("i", range(len(CASES)), ids=cases.IDS)
def test_oracle_within_the_bound(i):
    r = cases.reference(i)
    d = np.abs(r["y32"].astype(np.float64) - r["y64"])
    used = float((d / r["bound"]).max())
    print("BOUND %s oracle uses %.3f of the bound, E_ref %.3g ymax %.3g" % (CASES[i].id, used, r["E_ref"], r["ymax"]))
    assert np.isfinite(r["y64"]).all() and (r["bound"] > 0).all() and np.isfinite(r["bound"]).all()
    assert (d <= r["bound"]).all(), used
    assert blockref.criterion(r["E_ref"], r["E_ref"], r["ymax"]), (r["E_ref"], r["ymax"])


@pytest.mark.parametrize("i", range(len(NF_CASES)), ids=cases.NF_IDS)
def test_non_finite_inputs_do_what_they_are_there_for(i):
    c, r = NF_CASES[i], cases.nf_reference(i)
    y32, y64, lin, t, ok, b = r["y32"], r["y64"], r["lin64"], r["touched"], r["ok"], r["bound"]
    assert np.array_equal(~np.isfinite(lin), t), "the touched set of the geometry is not the set of non-finite outputs of front64"
    assert cases.classes(lin) == {"nan", "+inf", "-inf"}, cases.classes(lin)
    assert ok.mean() >= 0.1, "%.2f of the outputs are untouched" % ok.mean()
    NC, lpr, sl, band, nbands, _, _ = cases.geometry(c)
    kinds = {what for *_, what in r["P"]}
    assert kinds == {"corners", "frame-seam", "lane", "seam", "last-column", "band", "rows", "pair"} and nbands > 1, kinds
    assert {v for *_, v, _ in r["P"] if np.isinf(v)} == {np.inf, -np.inf} and any(np.isnan(v) for *_, v, _ in r["P"])
    xs = {x for _, _, _, x, _, what in r["P"] if what == "lane"}
    assert xs == {x for k in (1, 16, 32) if 2 * NC * k < 2 * c.W for x in (2 * NC * k - 1, 2 * NC * k)}
    assert np.array_equal(np.isnan(y32), np.isnan(y64)) and np.array_equal(np.isinf(y32), np.isinf(y64))
    assert np.array_equal(y32[np.isinf(y32)], y64[np.isinf(y32)].astype(np.float32))
    fin = np.isfinite(y64)
    assert fin[ok].all() and np.isfinite(b[fin]).all() and (b[ok] > 0).all()
    d = np.abs(np.where(fin, y32, 0).astype(np.float64) - np.where(fin, y64, 0))
    used = float((d[fin] / np.maximum(b[fin], 1e-300)).max())
    print("BOUND %s oracle uses %.3f of the bound over the finite outputs, %d of them touched" % (c.id, used, int((fin & t).sum())))
    assert (d[fin] <= b[fin]).all(), used
    assert blockref.criterion(r["E_ref"], r["E_ref"], r["ymax"])
    if 1 in c.acts:
        assert (fin & t).any(), "a relu brings touched outputs back to ordinary numbers or exact zeros"


def test_lane_boundaries_of_the_dpp_rows_are_planted():
    seen = set()
    for i, c in enumerate(NF_CASES):
        NC = cases.geometry(c)[0]
        seen |= {(NC, x // (2 * NC)) for _, _, _, x, _, what in cases.nf_reference(i)["P"] if what == "lane" and x % (2 * NC) == 0}
    assert seen >= {(3, 1), (3, 16), (3, 32), (4, 1), (4, 16), (4, 32)}, seen


def test_u8_input_is_net_input(orc, tmp_path):
    c = FORM_CASES[0]
    cfg = str(tmp_path / "front.cfg")
    open(cfg, "w").write(cases.cfg_text(c))
    o = orc.Oracle(cfg=cfg, weights=None)
    try:
        IW, IH = 2 * c.W, 2 * c.H
        u8 = np.random.default_rng(5).integers(0, 256, (2, IH, IW, 3), dtype=np.uint8)
        want = frontref.u8_input(u8, cases.MEAN, cases.NORM)
        for n in range(2):
            pk = np.zeros((IH, (3 * IW + 3) & ~3), np.uint8)
            pk[:, :3 * IW] = u8[n].reshape(IH, 3 * IW)
            o.set_input_image(pk, IW, IH, cases.MEAN, cases.NORM)
            assert np.array_equal(np.array(o.input).view(np.uint32), want[n].view(np.uint32))
    finally:
        o.close()
