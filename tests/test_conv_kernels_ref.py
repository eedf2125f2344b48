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
    x3 = set(cases.X3)
    assert {c.kernel for c in CASES} == fp32 | x3
    assert {c.kernel for c in NF_CASES} == fp32 | x3 | {"pw_bf16"}
    for k in fp32 | x3 | {"pw_bf16"}:
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


def test_the_table_covers_the_split_kernels():
    """every path the split-bf16 kernels' cases are there for, stated on the shapes"""
    A = {k: [c for c in CASES if c.kernel == k] for k in cases.X3}
    B = {k: [c for c in NF_CASES if c.kernel == k] for k in cases.X3}
    for k in cases.X3:
        assert all(c.variant == cases.X3_VARIANT[k] for c in A[k] + B[k]), k
        assert {c.act for c in A[k]} == {0, 1, 2, 3}, k
    ics = lambda L: {c.shape[3] for c in L}
    px = lambda c: c.shape[0] * c.shape[1] * c.shape[2]
    # k_pw_x3: k-steps of 32 -- under one, one channel into the second, several; row blocks of 16 ragged; more than one 64-channel workgroup; MT 1, 2, 4
    assert ics(A["pw_x3"]) >= {8, 33} and any(c.shape[3] > 64 and c.shape[3] % 32 for c in A["pw_x3"]) and any(c.shape[8] % 16 for c in A["pw_x3"]) and any(c.shape[8] > 128 for c in A["pw_x3"])
    assert {c.env.get("FFGPU_PWX3_MT") for c in A["pw_x3"]} == {None, "1", "2", "4"}
    # pw_x3s: one k-unit (three padded), a ragged last group, whole groups; a frame size that is no multiple of 64; a ragged last tile
    assert {c.shape[3] // 8 % 4 for c in A["pw_x3s"]} >= {0, 1, 2, 3} or {c.shape[3] // 8 for c in A["pw_x3s"]} >= {1, 5, 15, 2}
    assert any(c.shape[0] > 1 and (c.shape[1] * c.shape[2]) % 64 for c in A["pw_x3s"]) and any(px(c) % 64 for c in A["pw_x3s"])
    assert {(c.env.get("FFGPU_IGX3_MT"), c.env.get("FFGPU_IGX3_NW")) for c in A["pw_x3s"]} == {(None, None), ("1", "4"), ("2", "4"), ("4", "8")}
    # k_pw_x3t: chunks of 16 in pairs -- half a chunk, an odd number of chunks, whole pairs; under one 128-pixel tile, a ragged last one; a ragged second 256-channel tile
    assert ics(A["pw_x3t"]) >= {8, 33, 16} and any(px(c) < 128 for c in A["pw_x3t"]) and any(px(c) > 128 and px(c) % 128 for c in A["pw_x3t"])
    assert any(256 < c.shape[8] < 512 for c in A["pw_x3t"]) and any(128 < c.shape[8] < 256 for c in A["pw_x3t"])
    assert {tuple(sorted(c.env.items())) for c in A["pw_x3t"]} == {(), (("FFGPU_PWXT_NARROW", "0"),), (("FFGPU_PWXT_NT", "1"),), (("FFGPU_PWXT_TM", "128"),)}
    # k_conv_x3: qskip = 0 .. 3 at stride 1 (width % 4 = 0, 1, 2, 3 -> qskip = 0, 3, 2, 1), one row, ragged last group; stride 2: output widths 4, 5, 6, 13
    s1, s2 = [c for c in A["conv_x3"] if c.shape[6] == 1], [c for c in A["conv_x3"] if c.shape[6] == 2]
    assert {c.shape[1] % 4 for c in s1} == {0, 1, 2, 3} and {(3 * c.shape[3] // 8 + 3) // 4 for c in s1} >= {1, 2, 3, 4} and any(c.shape[2] == 1 for c in s1) and any((3 * c.shape[3] // 8) % 4 for c in s1) and any(c.shape[8] > 64 for c in s1)
    assert {c.shape[1] // 2 for c in s2} >= {4, 5, 6, 13} and all(c.shape[1] % 2 == 0 and c.shape[2] % 2 == 0 for c in s2)
    for L in (s1, s2):
        assert {(c.env.get("FFGPU_IGX3_MT"), c.env.get("FFGPU_IGX3_NW")) for c in L} == {(None, None), ("1", "4"), ("2", "8"), ("4", "4")}
    # part B: ic ragged for every k-step size, the range seams inside the tensor, both strides of the 3x3 form, a width that is no multiple of 4
    for k in ("pw_x3", "pw_x3s", "pw_x3t"):
        assert all(c.shape[3] % 32 and c.shape[3] % 16 and px(c) > 512 for c in B[k]), k
    assert {c.shape[6] for c in B["conv_x3"]} == {1, 2} and any(c.shape[1] % 4 for c in B["conv_x3"]) and any((3 * c.shape[3] // 8) % 4 for c in B["conv_x3"])


X3_CASES = [i for i, c in enumerate(CASES) if c.kernel in cases.X3]


@pytest.mark.parametrize("i", X3_CASES, ids=[cases.IDS[i] for i in X3_CASES])
def test_split_model(i):
    """the three conditions that make part A of a split kernel worth running: (a) the oracle and the numpy model of the kernels' arithmetic meet the derived bound,
    (b) the model meets the criterion the kernels are held to (factor 2 against E_ref), (c) the model that forgets ONE of the three 2^-16-sized partial
    products fails it -- the hard bound alone would not notice from K of about 16 up"""
    c, r = CASES[i], cases.reference(i)
    model, *wrong = cases.x3_models(i)
    d = np.abs(model.astype(np.float64) - r["y64"])
    E_m = float(d.max())
    print("MODEL %s E_model / E_ref %.3f, %.3f of the bound" % (c.id, E_m / r["E_ref"], float((d / r["bound"]).max())))
    assert (d <= r["bound"]).all(), float((d / r["bound"]).max())
    assert blockref.criterion(E_m, r["E_ref"], r["ymax"], 2.0), (E_m, r["E_ref"], r["ymax"])
    for drop, w in zip(convref.X3_SMALL, wrong):
        E_w = float(np.abs(w.astype(np.float64) - r["y64"]).max())
        print("      without w%d x%d: E / E_ref %.1f" % (drop + (E_w / r["E_ref"],)))
        assert not blockref.criterion(E_w, r["E_ref"], r["ymax"], 2.0), "a kernel that forgets w%d x%d would pass: E %.3g, E_ref %.3g" % (drop + (E_w, r["E_ref"]))


def test_split3_is_exact():
    """the model's split is the kernels': three bf16 numbers that add up to the value exactly; the dropped terms reach 2^-21.03 |w x| and stay
    under convref.X3_DROPPED; an empty part of a weight is packed as sign(w) 2^(e-40)"""
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.uniform(-2, 2, 100000), np.exp2(rng.uniform(-60, 60, 1000)), [1 + 2.0 ** -7 - 2.0 ** -23, 0.0, 1.0, -0.75]]).astype(np.float32)
    p = convref.split3(v)
    assert all(((q.view(np.uint32) & 0xffff) == 0).all() for q in p)
    assert np.array_equal(p[0].astype(np.float64) + p[1].astype(np.float64) + p[2].astype(np.float64), v.astype(np.float64))
    p64 = [q.astype(np.float64) for q in p]
    w, x = p64, [np.roll(q, 1) for q in p64]
    dropped = np.abs(w[1] * x[2] + w[2] * x[1] + w[2] * x[2])
    wx = np.abs(v.astype(np.float64) * np.roll(v, 1).astype(np.float64))
    assert (dropped <= convref.X3_DROPPED * wx).all()
    one = p64[1][-4] * p64[2][-4] * 2 + p64[2][-4] ** 2                   # w = x = 1 + 2^-7 - 2^-23
    assert 2.0 ** -21.1 < one / float(v[-4]) ** 2 < 2.0 ** -21
    q = convref.split3(np.array([1.5, -0.75, 0.0, 1.0 + 2.0 ** -10], np.float32), weights=True)
    assert q[1][0] == 2.0 ** -40 and q[2][0] == 2.0 ** -40 and q[1][1] == -2.0 ** -41 and q[1][2] == 0 and q[2][2] == 0 and q[1][3] == 2.0 ** -10 and q[2][3] == 2.0 ** -40


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
    for k in cases.X3:
        assert by_kernel[k] >= {"strip-seam", "range-seam", "unit-edge"}, k
    assert by_kernel["conv_x3"] >= {"last-quad", "row-wrap", "stride", "last-column", "last-row"}
    assert not any(what in ("range-seam", "unit-edge", "last-quad", "row-wrap", "last-column", "last-row") for k, seen in by_kernel.items() if k not in cases.X3 for what in seen)


def test_split_placements_land_on_positions_of_their_own():
    """none of the split kernels' placements falls on a position that is taken, every one of them is there, and each is where it is meant to be"""
    want = {"range-seam": 4, "unit-edge": 1, "strip-seam": 4}
    for c in NF_CASES:
        if c.kernel not in cases.X3:
            continue
        N, W, H, ic, groups, pad, stride, fs, oc, OH, OW, K = cases.dims(c)
        dropped = []
        P = cases.placements(N, W, H, ic, groups, stride, fs, dropped)
        new = ("range-seam", "unit-edge", "last-quad", "row-wrap", "last-column", "last-row")
        assert not [d for d in dropped if d[5] in new], (c.id, dropped)
        assert len({p[:4] for p in P}) == len(P)
        n = {}
        for *_, what in P:
            n[what] = n.get(what, 0) + 1
        w3 = dict(want, **({"last-quad": 4, "row-wrap": 2} if fs == 3 else {}), **({"last-column": 1, "last-row": 1, "stride": 2} if stride == 2 else {}))
        if N * H * W <= 512:
            w3["range-seam"] = sum(p < N * H * W for p in (255, 256, 511, 512))
        assert all(n.get(k, 0) == v for k, v in w3.items()), (c.id, n)
        flat = sorted(nn * H * W + y * W + x for ch, nn, y, x, v, what in P if what == "range-seam")
        assert flat == [p for p in (255, 256, 511, 512) if p < N * H * W], (c.id, flat)
        assert [p[0] for p in P if p[5] == "unit-edge"] == [ic - 8] and [p[0] for p in P if p[5] == "last-channel"] == [ic - 1]
        if fs == 3:
            assert sorted(p[3] for p in P if p[5] == "last-quad") == [W - 4, W - 3, W - 2, W - 1] and len({p[:3] for p in P if p[5] == "last-quad"}) == 1
            a, b = [p for p in P if p[5] == "row-wrap"]
            assert a[:2] == b[:2] and (a[2] + 1, a[3], b[3]) == (b[2], W - 1, 0)
        if stride == 2:
            assert [p[3] for p in P if p[5] == "last-column"] == [W - 1] and [p[2] for p in P if p[5] == "last-row"] == [H - 1]


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


@pytest.mark.parametrize("row", cases.RES_TABLE + [cases.RES_NF, cases.RES_NF_X3], ids=cases.RES_IDS + [cases.RES_NF[0], cases.RES_NF_X3[0]])
def test_residual_cfgs(capi, orc, tmp_path, monkeypatch, row):
    """part C without a GPU: AUTO picks the declared kernel for the conv under the case's switches, the cfg is one the reference's parser takes, the conv is linear
    and shape-preserving, and the shortcut adds the declared layer with the declared activation"""
    name, kernel, env, batch, w, h, ic, oc, size, groups, act = row
    stride = cases.RES_STRIDE.get(name, 1)
    for k in cases.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in cases.SWITCHES, k
        monkeypatch.setenv(k, v)
    assert capi.kernel_name(batch, w, h, ic, groups, size // 2, stride, size, oc) == kernel
    g, a, b, c, s = cases.res_nf_cfg(row) if row in (cases.RES_NF, cases.RES_NF_X3) else cases.res_cfg(row)
    cfg = str(tmp_path / "res.cfg")
    with open(cfg, "w") as fp:
        fp.write(g.cfg_text())
    o = orc.Oracle(cfg=cfg, weights=None)
    try:
        L, S = o.layer(c), o.layer(s)
        assert (L.kind, L.ic, L.oc, L.fs, L.stride, L.pad, L.groups, L.act) == (0, ic, oc, size, stride, size // 2, groups, 0)
        assert (L.ow, L.oh) == (w // stride, h // stride) and S.ndep == 1 and S.dep[0] == a and S.act == {"linear": 0, "relu": 1, "leaky": 2}[act]
        assert (o.layer(a).oc, o.layer(a).ow, o.layer(a).oh) == (oc, w // stride, h // stride)
        if kernel in cases.X3 and name != "pw_x3s":
            # the thresholds steer THIS conv only: without them AUTO takes it elsewhere, and with them the cfg's other convs are not taken along
            assert all(capi.kernel_name(batch, T.iw, T.ih, T.ic, T.groups, T.pad, T.stride, T.fs, T.oc) not in ("pw_x3", "pw_x3t") or k == c
                       for k in range(len(g.kind)) if g.kind[k] == "conv" for T in [o.layer(k)])
            for k in env:
                monkeypatch.delenv(k)
            assert capi.kernel_name(batch, w, h, ic, groups, size // 2, stride, size, oc) != kernel
    finally:
        o.close()
    assert s not in g.steps[True] and s in g.steps[False] and c in g.steps[True]
