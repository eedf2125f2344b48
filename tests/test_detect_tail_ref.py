"""CPU side of tests/detect_tail: the tie-ordered NMS restatement (heads.nms_ordered) is pinned to orc.nms, every crafted head tensor is held to
its purpose in the ORACLE's eyes (planted class-scan cases, the threshold walk straddling, zero scores, record sizes, tie-free and tied lists),
and the operators the GPU tests compare the kernels with (orc.yolo + orc.nms on a head's input) equal the oracle's net path and, where oracle/_ref
is built, the reference itself on the same cfgs.  No comparison has a tolerance."""
import numpy as np
import pytest

from detect_tail import heads

SCAN_CLASSES = (1, 2, 63, 64, 65, 80, 129)


def _random_list(rng, n, classes, zeros=0, specials=False):
    b = np.zeros(n, heads.BOX_DTYPE)
    b["type"] = rng.integers(0, classes, n)
    b["score"] = rng.permutation(n).astype(np.float32) / np.float32(n) + np.float32(0.001)       # pairwise distinct
    cx, cy = rng.uniform(0, 100, n), rng.uniform(0, 100, n)
    w, h = rng.uniform(1, 60, n), rng.uniform(1, 60, n)
    for c, v in (("x1", cx - w / 2), ("y1", cy - h / 2), ("x2", cx + w / 2), ("y2", cy + h / 2)):
        b[c] = v.astype(np.float32)
    if zeros:
        b["score"][rng.permutation(n)[:zeros]] = 0          # (several zeros tie with each other only: none of them is kept)
    if specials:
        at = rng.permutation(n)[:6]
        b["x1"][at[0]], b["y2"][at[1]] = np.nan, np.nan
        b["x1"][at[2]], b["x2"][at[2]] = -np.inf, np.inf
        b["y1"][at[3]], b["y2"][at[3]] = -np.inf, np.inf
        b["x2"][at[4]] = b["x1"][at[4]]                     # an empty box: area 0, metric 0 / 0
        b["x1"][at[5]], b["x2"][at[5]] = np.inf, np.inf     # inf - inf
    return b


@pytest.mark.parametrize("seed", range(6))
def test_nms_ordered_is_orc_nms_on_tie_free_lists(orc, seed):
    rng = np.random.default_rng(seed)
    for n, classes, zeros, specials in ((1, 1, 0, False), (12, 2, 3, False), (300, 3, 0, False), (300, 2, 7, True), (900, 5, 1, True)):
        b = _random_list(rng, n, classes, zeros, specials)
        assert heads.tie_free(b[b["score"] != 0])
        for use_min in (1, 0):
            for s1, s2 in ((1, 1), (3, 2), (7, 5)):
                want = orc.nms(b, 0.5, use_min, s1, s2)
                got = heads.nms_ordered(b, 0.5, use_min, s1, s2)
                assert got.tobytes() == want.tobytes(), (seed, n, use_min, s1, s2)
                assert not (want["score"] == 0).any() and len(want) < max(n, 2)
    assert len(heads.nms_ordered(np.zeros(0, heads.BOX_DTYPE))) == 0 and len(orc.nms(np.zeros(0, heads.BOX_DTYPE))) == 0


def test_nms_ordered_breaks_ties_by_position(orc):
    """two identical boxes of one class and one score: the earlier one stays; of two disjoint ones both stay, in list order"""
    b = _random_list(np.random.default_rng(0), 4, 1)
    b[1] = b[0]
    b["x1"][2:], b["x2"][2:] = (1000, 2000), (1010, 2010)
    b["score"][2:] = 0.5
    b["type"][1] = 0
    b["type"][0] = 0
    got = heads.nms_ordered(b)
    assert [g.tobytes() for g in got if g["score"] == np.float32(0.5)] == [b[2].tobytes(), b[3].tobytes()]
    assert sum(g.tobytes() == b[0].tobytes() for g in got) == 1


def _fulls(orc, case, frames):
    return [np.concatenate([heads.decode(orc, case, h, frames[f]) for h in case.heads]) for f in range(case.batch)]


@pytest.mark.parametrize("classes", SCAN_CLASSES)
def test_decode_scan_plants(orc, classes):
    """every planted case is present and is what it claims, on both heads; the small head takes the specs in two halves"""
    names = set()
    for case, part in ((heads.single("scan", 10, 10, classes, 3, ".25"), None), (heads.single("scan1", 1, 1, classes, 5, ".25"), 0), (heads.single("scan1", 1, 1, classes, 5, ".25"), 1)):
        frames, plants = heads.decode_scan(case, 100 + classes, part)
        fulls = _fulls(orc, case, frames)
        heads.check_plants(orc, case, frames, plants, fulls)
        if part is not None:
            names |= {p[0] for p in plants}
        else:
            assert len(plants) == len(heads.plant_specs(classes)) and len({p[1:5] for p in plants}) == len(plants)
            assert all(20 < len(c) < 300 for c in fulls)
    assert names == {s[0] for s in heads.plant_specs(classes)}
    want = {"maximum at class %d" % c for c in (0, 1, 62, 63, 64, classes - 1) if c < classes} | {"NaN at class 0", "all -inf", "NaN objectness", "+inf twice"}
    assert want <= names and (classes < 2 or any(n.startswith("tie") for n in names)) and (classes <= 64 or "tie 3 = 64" in names)


def test_threshold_walk_straddles(orc):
    """across the thresholds the oracle passes some anchors of the walks and fails others -- and within the walk of .01, .25 and .9, where 64 ulps
    of objectness are many ulps of confidence; the +20 anchor passes everywhere; at threshold 0 everything passes"""
    total = {True: 0, False: 0}
    for t in heads.THRESHOLDS:
        case = heads.threshold_case(t)
        frames, where = heads.threshold_edge(case)
        assert len(where) == 2 * 129 and len(set(where)) == len(where)
        ok = heads.edge_passes(orc, case, frames, where)
        for f in (0, 1):
            mine = [o for o, w in zip(ok, where) if w[0] == f]
            total[True] += sum(mine)
            total[False] += len(mine) - sum(mine)
            if t in (".01", ".25", ".9") and f == 0:
                assert 0 < sum(mine) < len(mine), (t, sum(mine))
                assert mine == sorted(mine), "passing is monotonic in the objectness"
        if t == "0":
            assert all(ok)
        full = _fulls(orc, case, frames)
        assert len(full[1]) >= 1 and len(full[0]) == sum(o for o, w in zip(ok, where) if w[0] == 0) + (300 - 129 if t == "0" else 0)
    assert total[True] > 100 and total[False] > 100


def test_many_candidate_lists(orc):
    """threshold 0: every anchor is a candidate; the named seed is free of ties (plain orc.nms), the large lists have natural ties and hundreds
    of survivors; the scratch-sized head has more than FFGPU_NMS_LDS_CAP slots, the one before it at most that many"""
    w, h, batch, seed = heads.TIE_FREE
    case = heads.many_case(w, h, batch)
    kept = []
    for c in _fulls(orc, case, heads.gauss(case, seed)):
        assert len(c) == case.slots and heads.tie_free(c)
        kept.append(len(heads.nms(orc, c)[0]))
    assert max(kept) > heads.MAX_DET and min(kept) > 100            # (a record that overflows and, on this seed, one that does not)
    tied = 0
    for name, w, h, batch, seed in heads.MANY:
        case = heads.many_case(w, h, batch)
        for c in _fulls(orc, case, heads.gauss(case, seed)):
            assert len(c) == case.slots
            tied += not heads.tie_free(c)
    assert tied >= 2
    assert heads.many_case(*heads.SCRATCH_HEAD, 2).slots == heads.NMS_LDS_CAP + 1 and heads.many_case(65, 42, 2).slots == 8190
    assert heads.many_case(53, 52, 2).slots == 8268


def test_tied_list_against_both_orders(orc):
    """nms_ordered on a list WITH ties: make the order it states strict by hand (new scores, descending in that order) and plain orc.nms keeps
    the same boxes in the same order"""
    case = heads.many_case(65, 42, 2)
    c = _fulls(orc, case, heads.gauss(case, 1))[0]
    assert not heads.tie_free(c)
    c = c[c["score"] > 0]
    order = np.argsort(-c["score"].astype(np.float64), kind="stable")
    d = c[order].copy()
    d["score"] = np.linspace(1, 0.1, len(d)).astype(np.float32)            # the same order, now strict
    assert heads.tie_free(d)
    a, b = heads.nms_ordered(d), orc.nms(d)
    assert a.tobytes() == b.tobytes()
    kept = heads.nms_ordered(c)
    assert [k.tobytes()[8:] for k in kept] == [k.tobytes()[8:] for k in a] and (kept["type"] == a["type"]).all()


def test_record_frames(orc):
    case = heads.record_case(len(heads.RECORD_KS))
    frames = heads.record_frames(case, heads.RECORD_KS)
    for K, c in zip(heads.RECORD_KS, _fulls(orc, case, frames)):
        assert len(c) == K and heads.tie_free(c)
        boxes, plain = heads.nms(orc, c)
        assert plain and len(boxes) == K                                  # disjoint: nothing is suppressed
        r = heads.record(boxes, K, 768)
        assert (r["count"], r["nfull"], r["overflow"]) == (min(K, 128), K, 4 if K > 128 else 0)


def test_zero_score_frames(orc):
    """the planted anchors are candidates of score exactly 0 (class 2, and class 0 for the all -inf one) that orc.nms never returns, although
    nothing of their class touches them"""
    case = heads.zero_case()
    frames, where = heads.zero_frames(case)
    fulls = _fulls(orc, case, frames)
    for f, k, i, j, cls in where:
        one = heads.cell_candidate(orc, case, case.heads[0], frames[f], k, i, j)
        assert len(one) == 1 and one[0]["score"] == 0 and one[0]["type"] == cls and not np.signbit(one[0]["score"])
    for f, c in enumerate(fulls):
        assert len(c) == case.slots and (c["score"] == 0).sum() == 6 and (c["type"] == 2).sum() == 5
        boxes, _ = heads.nms(orc, c)
        assert not (boxes["score"] == 0).any() and not (boxes["type"] == 2).any()
        live = c[c["score"] != 0]
        assert heads.nms(orc, live)[0].tobytes() == boxes.tobytes()        # dead boxes change nothing for the others


# ---------------------------------------------------------------------------------------------- the operators against the net paths
def _net_cases():
    out = []
    for classes in (1, 65):
        case = heads.single("scan_c%d" % classes, 10, 10, classes, 3, ".25")
        out.append((case, heads.decode_scan(case, 100 + classes)[0]))
    case = heads.threshold_case(".25")
    out.append((case, heads.threshold_edge(case)[0]))
    out.append((heads.pooled(), heads.gauss(heads.pooled(), 21, sigma=16.0)))
    out.append((heads.two_heads(), heads.gauss(heads.two_heads(), 21)))
    case = heads.zero_case()
    out.append((case, heads.zero_frames(case)[0]))
    case = heads.many_case(20, 20, 3)
    out.append((case, heads.gauss(case, 1)))
    return out


@pytest.mark.parametrize("n", range(7))
def test_operators_match_the_net_paths(orc, tmp_path, n):
    """orc.yolo on each head's input, concatenated in cfg order, then orc.nms: the oracle's own net path gives the same bytes, and so does the
    reference (v0) where it is built -- same libc, same qsort, so ties are ordered alike in all three"""
    case, frames = _net_cases()[n]
    cfg = str(tmp_path / (case.name + ".cfg"))
    with open(cfg, "w") as fp:
        fp.write(case.cfg_text())
    wts = str(tmp_path / (case.name + ".weights"))
    with open(wts, "wb") as fp:
        fp.write(np.array([0, 2, 5], "<i4").tobytes() + np.array([0], "<u8").tobytes())       # a darknet header and no weights: no conv layer
    o = orc.Oracle(cfg=cfg, weights=wts)
    assert o.nlayers == case.nlayers
    for f in range(case.batch):
        o.input[...] = frames[f]
        o.n.s1, o.n.s2 = 1, 1
        o.forward(0)
        acts = {h.src: o.layer_out(h.src).copy() for h in case.heads}
        assert acts[1].tobytes() == frames[f].tobytes() if 1 in acts else True
        full = np.concatenate([heads.decode(orc, case, h, acts[h.src]) for h in case.heads])[:o.n.cap]
        assert o.candidates.tobytes() == full.tobytes() and len(full) >= 1
        want = orc.nms(full, 0.5, 1, 1, 1)
        assert o.boxes.tobytes() == want.tobytes()
        if heads.tie_free(full):
            assert heads.nms_ordered(full).tobytes() == want.tobytes()
        if orc.have_ref("v0"):
            r = orc.Ref("v0", cfg=cfg, weights=wts)           # (a fresh net per frame: the leading dropout moves the input buffer away)
            r.input[...] = frames[f]
            r.n.s1, r.n.s2 = 1, 1                            # (net_input would set them)
            r.forward(keep_activations=True)
            cut = orc.nms(full[:r.n.bbox_max], 0.5, 1, 1, 1)
            assert r._boxes.tobytes() == cut.tobytes(), (case.name, f)
            r.n.layer_list[0].data = None
            r.close()
    o.close()
