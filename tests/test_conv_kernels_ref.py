"""CPU side of tests/conv_kernels: the table of cases and the two yardsticks are held to their purpose before any kernel is.

  - every case's (variant, shape) answers the declared kernel name under the case's switches (ffgpu_groupconv_kernel_name is host code);
  - the oracle stays within the hard bound of convref (derived, not measured) against conv64 for every case, and meets the criterion the kernels are held to:
    a wrong bound or a wrong conv64 shows here;
  - for the non-finite inputs of part B: the oracle's and conv64's NaN and +-Inf patterns agree, the touched set computed from the geometry IS the set of
    non-finite outputs of conv64 under a linear activation, {NaN, +Inf, -Inf} all occur there, and relu / sigmoid turn them into the exact values the GPU test expects;
  - every placement of cases.placements is planted in at least one case of every kernel it is meant for."""
import numpy as np
import pytest

from conv_kernels import cases, convref
from conv_kernels.cases import CASES, NF_CASES, PAIRS, NF_PAIRS
from irb_blocks import blockref


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi
    capi.build_library()
    return capi


def test_every_case_reaches_its_kernel(capi):
    mp = pytest.MonkeyPatch()
    bad = []
    try:
        for c in CASES + NF_CASES:
            cases.set_switches(mp, c)
            if cases.kernel_name(capi, c) != c.name:
                bad.append((c.id, cases.kernel_name(capi, c)))
    finally:
        mp.undo()
    assert not bad, bad


def test_the_table_covers_the_kernels():
    fp32 = {"conv_generic", "dw3_stream", "dw_lds", "dw_pair", "pw_mfma", "pw_gemm", "conv_dense8", "conv_first", "conv_igemm", "conv_thin"}
    assert {c.kernel for c in CASES} == fp32
    assert {c.kernel for c in NF_CASES} == fp32 | {"pw_bf16"}
    for k in fp32 | {"pw_bf16"}:
        want = {0, 1, 2} if k in cases.NO_SIGMOID else {0, 1, 2, 3}
        assert {c.act for c in NF_CASES if c.kernel == k} == want, k
    # the two forms of the first layer come in pairs on the same shape and activation (compared bit for bit on the device)
    first = [(c.shape, c.act) for c in CASES if c.kernel == "conv_first"]
    assert first and all((s, a) in [(c.shape, c.act) for c in CASES if c.kernel == "conv_dense8"] for s, a in first)
    # ragged K where the issue's defect lives
    assert {c.shape[3] % 4 for c in NF_CASES if c.kernel == "pw_mfma"} >= {1, 2, 3}
    assert all(c.shape[3] % 16 and c.shape[3] % 32 for c in NF_CASES if c.kernel in ("pw_gemm", "pw_bf16"))
    assert any(c.shape[3] == 136 for c in NF_CASES if c.kernel == "pw_gemm") and any(c.shape[3] == 136 for c in NF_CASES if c.kernel == "pw_bf16")
    assert any((c.shape[7] ** 2 * c.shape[3] // c.shape[4]) % 4 for c in NF_CASES if c.kernel == "conv_igemm")
    assert any(c.shape[4] > 1 for c in NF_CASES if c.kernel == "conv_igemm") and any(c.shape[4] > 1 for c in NF_CASES if c.kernel == "conv_thin")


@pytest.mark.parametrize("i", range(len(CASES)), ids=cases.IDS)
def test_oracle_within_the_bound(i):
    r = cases.reference(i)
    d = np.abs(r["y32"].astype(np.float64) - r["y64"])
    used = float((d / r["bound"]).max())
    print("BOUND %s oracle uses %.3f of the bound, E_ref %.3g ymax %.3g" % (CASES[i].id, used, r["E_ref"], r["ymax"]))
    assert np.isfinite(r["y64"]).all() and (r["bound"] > 0).all()
    assert (d <= r["bound"]).all(), used
    assert blockref.criterion(r["E_ref"], r["E_ref"], r["ymax"]), (r["E_ref"], r["ymax"])


@pytest.mark.parametrize("i", range(len(NF_CASES)), ids=cases.NF_IDS)
def test_non_finite_inputs_do_what_they_are_there_for(i):
    c, r = NF_CASES[i], cases.nf_reference(i)
    y32, y64, lin, t, ok = r["y32"], r["y64"], r["lin64"], r["touched"], r["ok"]
    assert np.array_equal(~np.isfinite(lin), t), "the touched set of the geometry is not the set of non-finite outputs of conv64"
    assert cases.classes(lin) == {"nan", "+inf", "-inf"}, cases.classes(lin)
    assert ok.any(), "no untouched output left"
    assert np.array_equal(np.isnan(y32), np.isnan(y64)) and np.array_equal(np.isinf(y32), np.isinf(y64))
    assert np.array_equal(y32[np.isinf(y32)], y64[np.isinf(y32)].astype(np.float32))
    # a touched output is NaN, +-Inf or -- after relu / sigmoid -- exactly 0 or 1, in both
    tv = y64[t]
    assert np.isin(tv[~np.isnan(tv)], (np.inf, -np.inf, 0.0, 1.0)).all()
    assert np.array_equal(y32[t][~np.isnan(tv)], tv[~np.isnan(tv)].astype(np.float32))
    if c.act == 1:
        assert not np.isnan(y64).any() and not np.isneginf(y64).any() and np.isposinf(y64).any()
    if c.act == 3:
        assert not np.isinf(y64).any() and np.isnan(y64).any() and (tv == 1.0).any() and (tv == 0.0).any()
    if c.act == 2:
        assert np.isneginf(y64).any()
    d = np.abs(np.where(ok, y32, 0).astype(np.float64) - np.where(ok, y64, 0))
    assert (d[ok] <= r["bound"][ok]).all(), float((d[ok] / r["bound"][ok]).max())
    assert blockref.criterion(r["E_ref"], r["E_ref"], r["ymax"])


def test_every_placement_is_planted():
    by_kernel = {}
    for i, c in enumerate(NF_CASES):
        by_kernel.setdefault(c.kernel, set()).update(what for *_, what in cases.nf_reference(i)["P"])
    common = {"last-channel", "group-edge", "pair", "nan", "corners", "edges", "frame-seam"}
    for k, seen in by_kernel.items():
        assert seen >= common, (k, common - seen)
    for k in ("pw_mfma", "pw_gemm", "pw_bf16"):
        assert "strip-seam" in by_kernel[k], k
    for k in ("conv_generic", "dw_lds", "conv_dense8", "conv_first", "conv_igemm", "conv_thin"):
        assert "stride" in by_kernel[k], k


@pytest.mark.parametrize("nf", [False, True], ids=["finite", "nf"])
def test_pair_reference(nf):
    for i, p in enumerate(NF_PAIRS if nf else PAIRS):
        r = cases.pair_reference(i, nf)
        ok = r["ok"]
        d = np.abs(np.where(ok, r["y32"], 0).astype(np.float64) - np.where(ok, r["y64"], 0))
        assert ok.any() and (~r["touched"] <= ok).all() and (d[ok] <= r["bound"][ok]).all(), (p.id, float((d[ok] / r["bound"][ok]).max()))
        assert blockref.criterion(r["E_ref"], r["E_ref"], r["ymax"]), p.id
        assert np.array_equal(np.isnan(r["y32"]), np.isnan(r["y64"])) and np.array_equal(np.isinf(r["y32"]), np.isinf(r["y64"])), p.id
        if nf:
            assert np.array_equal(~np.isfinite(r["lin64"]), r["touched"]), p.id
            assert cases.classes(r["lin64"]) >= {"nan", "+inf"}, p.id


@pytest.mark.parametrize("row", cases.RES_TABLE + [cases.RES_NF], ids=cases.RES_IDS + [cases.RES_NF[0]])
def test_residual_cfgs(capi, orc, tmp_path, monkeypatch, row):
    """part C without a GPU: AUTO picks the declared kernel for the conv under the case's switches, the cfg is one the reference's parser takes, the conv is linear
    and shape-preserving, and the shortcut adds the declared layer with the declared activation"""
    name, kernel, env, batch, w, h, ic, oc, size, groups, act = row
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert capi.kernel_name(batch, w, h, ic, groups, size // 2, 1, size, oc) == kernel
    g, a, b, c, s = cases.res_nf_cfg(row) if row is cases.RES_NF else cases.res_cfg(row)
    cfg = str(tmp_path / "res.cfg")
    with open(cfg, "w") as fp:
        fp.write(g.cfg_text())
    o = orc.Oracle(cfg=cfg, weights=None)
    try:
        L, S = o.layer(c), o.layer(s)
        assert (L.kind, L.ic, L.oc, L.fs, L.stride, L.pad, L.groups, L.act) == (0, ic, oc, size, 1, size // 2, groups, 0)
        assert (L.ow, L.oh) == (w, h) and S.ndep == 1 and S.dep[0] == a and S.act == {"linear": 0, "relu": 1, "leaky": 2}[act]
        assert (o.layer(a).oc, o.layer(a).ow, o.layer(a).oh) == (oc, w, h)
    finally:
        o.close()
    assert s not in g.steps[True] and s in g.steps[False] and c in g.steps[True]
