"""The crops classified on the device, without a GPU: the exported symbols, the layout of ffgpu_feature_spec / ffgpu_label / ffgpu_relabel_spec in the
ctypes mirror and the constants in the header, ffgpu_feature_dim, the contract's sentences in the header, tests/features/featref.py (the numpy
restatement the GPU tests compare with) pinned to literal scalar loops -- top-k, the MAX rules, relabel -- and the device entry points failing the way
every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from crops import cropref
from features import featref

SYMBOLS = ["ffgpu_feature_dim", "ffgpu_exec_feature_dim", "ffgpu_features_dev", "ffgpu_exec_features", "ffgpu_topk_dev", "ffgpu_crops_relabel_dev",
           "ffgpu_exec_relabel"]
NAN, INF = float("nan"), float("inf")
F32 = np.float32
BOX, DETS, LABEL = featref.BOX_DTYPE, featref.DETS_DTYPE, featref.LABEL_DTYPE


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_feature_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_feature_struct_layout(capi):
    P, L, R, G = capi.FeatureSpec, capi.Label, capi.RelabelSpec, capi.FFGPU
    assert (C.sizeof(P), C.sizeof(L), C.sizeof(R)) == (16, 8, 16)
    assert [getattr(P, f).offset for f in ("layer", "pool", "post", "reserved")] == [0, 4, 8, 12]
    assert [getattr(L, f).offset for f in ("index", "value")] == [0, 4]
    assert [getattr(R, f).offset for f in ("min_value", "type_base", "score_mode", "reserved")] == [0, 4, 8, 12]
    assert capi.LABEL_DTYPE == LABEL and LABEL.itemsize == 8 and featref.BOX_DTYPE == capi.BOX_DTYPE and featref.DETS_DTYPE == capi.DETS_DTYPE
    assert (G.FEAT_FLAT, G.FEAT_MEAN, G.FEAT_MAX) == (featref.FLAT, featref.MEAN, featref.MAX) == (0, 1, 2)
    assert (G.POST_NONE, G.POST_SOFTMAX, G.POST_L2) == (featref.NONE, featref.SOFTMAX, featref.L2) == (0, 1, 2)
    assert (G.RELABEL_KEEP_SCORE, G.RELABEL_LABEL_SCORE) == (featref.KEEP_SCORE, featref.LABEL_SCORE) == (0, 1)
    assert (G.RELABEL_ENTRIES, G.RELABEL_MERGED, G.TOPK_MAX) == (0, 1, 16)
    sp = capi.feature_spec(-1, G.FEAT_MAX, G.POST_L2)
    assert (sp.layer, sp.pool, sp.post, sp.reserved) == (-1, 2, 2, 0)
    rs = capi.relabel_spec(0.25, 100, G.RELABEL_LABEL_SCORE)
    assert (rs.min_value, rs.type_base, rs.score_mode, rs.reserved) == (0.25, 100, 1, 0)
    for name in ("feature_spec", "feature_dim", "features_dev", "topk_dev", "relabel_spec", "crops_relabel_dev"):
        assert getattr(G, name) is getattr(capi, name)
    for name in ("features", "feature_dim", "relabel"):
        assert callable(getattr(capi.Executor, name))


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    for name, val in (("FFGPU_FEAT_FLAT", 0), ("FFGPU_FEAT_MEAN", 1), ("FFGPU_FEAT_MAX", 2), ("FFGPU_POST_NONE", 0), ("FFGPU_POST_SOFTMAX", 1),
                      ("FFGPU_POST_L2", 2), ("FFGPU_TOPK_MAX", 16), ("FFGPU_RELABEL_KEEP_SCORE", 0), ("FFGPU_RELABEL_LABEL_SCORE", 1),
                      ("FFGPU_RELABEL_ENTRIES", 0), ("FFGPU_RELABEL_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val, name
    flat = " ".join(hdr.replace("*", " ").split())
    for sentence in ("} ffgpu_feature_spec;", "} ffgpu_label;", "} ffgpu_relabel_spec;",
                     "cfg without a [yolo] layer", "count = ncand = nfull = overflow = 0",
                     "plane (c, n) at ((c N + n) H W)", "out_stride >= D", "every element of every row is written",
                     "what ffgpu_exec_read_layer returns, bit for bit, NaN payloads and -0 included",
                     "divided by (float)(H W) with IEEE division", "no atomic, independent of n and N",
                     "Any NaN in the plane gives the quiet NaN 0x7fc00000", "zeros compare as -0 < +0",
                     "the accurate expf, not the fast intrinsic", "or with only -Inf, is all NaN", "A -Inf element in any other row gives 0",
                     "With r == 0 the row is all zeros", "At most two launches per call",
                     "aliases resolved: a trailing dropout or one-source route gives its source's tensor", "legal on every plan",
                     "legal only on FFGPU_KEEP_ALL executors", "Works on FFGPU_SPLIT2 executors", "A rejected call leaves the executor usable",
                     "value descending, as fp32 values compare; then index ascending", "NaN is never selected", "Missing entries are { -1, 0.0f }",
                     "One launch per call", "only entry 0 of each row is used", "index >= 0 and value >= min_value (a NaN value never)",
                     "type = type_base + index", "in the record's box[] where entry.box < count", "Every output byte is written",
                     "The outputs must not overlap the inputs", "names one box at most once"):
        assert sentence in flat, sentence
    inc = open(os.path.join(ROOT, "ffcnn_amd", "csrc", "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_feature.inc"' in inc and inc.index('#include "ffgpu_track.inc"') < inc.index('#include "ffgpu_feature.inc"')
    src = open(os.path.join(ROOT, "ffcnn_amd", "csrc", "ffgpu_feature.inc")).read()
    assert not re.search(r"\batomic\w*\s*\(", src) and "__expf" not in src


def test_feature_dim_is_pure_host_code(capi):
    """no device needed; 0 for arguments outside their ranges"""
    fd = capi.feature_dim
    assert [fd(255, 10, 10, 0), fd(255, 10, 10, 1), fd(255, 10, 10, 2), fd(1, 1, 1, 0), fd(1, 4096, 4096, 1), fd(2 ** 24, 1, 1, 2), fd(1024, 128, 128, 0)] == \
        [25500, 255, 255, 1, 1, 2 ** 24, 2 ** 24]
    assert [fd(0, 1, 1, 0), fd(1, 0, 1, 1), fd(1, 1, -1, 2), fd(1, 1, 1, 3), fd(1, 1, 1, -1), fd(2 ** 24 + 1, 1, 1, 1), fd(1025, 128, 128, 0),
            fd(1, 4097, 4096, 1), fd(2 ** 30, 2 ** 30, 2 ** 30, 0)] == [0] * 9
    for c, h, w in ((3, 7, 5), (129, 1, 1), (1, 13, 17)):
        for pool in (0, 1, 2):
            assert fd(c, h, w, pool) == featref.dim(c, h, w, pool)


# ------------------------------------------------------------------------------------------------- featref against literal scalar loops
def literal_topk(row, k):
    """selection by the contract's sentence: again and again the remaining element that no other remaining element precedes"""
    left = [i for i in range(len(row)) if not row[i] != row[i]]
    out = []
    while left and len(out) < k:
        best = left[0]
        for i in left[1:]:
            if row[i] > row[best] or (row[i] == row[best] and i < best):
                best = i
        out.append((best, row[best]))
        left.remove(best)
    return out + [(-1, F32(0))] * (k - len(out))


def test_topk_is_the_literal_loop():
    rng = np.random.default_rng(5500)
    rows = [np.array(r, F32) for r in ([1, 1, 1, 1, 1], [NAN] * 4, [0.0, -0.0, 0.0, -0.0, -1], [-0.0, 0.0], [INF, -INF, 3, INF, NAN, -INF], [2], [NAN, 5],
                                       [-INF, -INF, NAN], [1, 2, 3], [3, 2, 1, 3, 2, 1, 3])]
    for _ in range(40):
        d = int(rng.integers(1, 40))
        v = rng.integers(-3, 4, d).astype(F32)                                     # few distinct values: many ties
        v[rng.random(d) < 0.1] = NAN
        v[rng.random(d) < 0.1] = -0.0
        rows.append(v)
    seen = dict.fromkeys(("tie", "zero_tie", "nan", "short"), 0)
    for v in rows:
        for k in (1, 3, 8, 16):
            got = featref.topk(v[None, :], k)[0]
            want = literal_topk(list(v), k)
            assert [int(g["index"]) for g in got] == [w[0] for w in want], (v, k)
            assert np.array([g["value"] for g in got], F32).tobytes() == np.array([w[1] for w in want], F32).tobytes(), (v, k)
            seen["short"] += int(got[-1]["index"] < 0)
        seen["nan"] += int(np.isnan(v).any())
        seen["tie"] += int(len(set(v[~np.isnan(v)].tolist())) < (~np.isnan(v)).sum())
        seen["zero_tie"] += int((featref.bits(v) == 0x80000000).any() and (featref.bits(v) == 0).any())
    assert all(n > 0 for n in seen.values()), seen
    # by hand: +0 and -0 tie, the lower index wins and keeps its own sign; NaN is never selected; D < k pads
    got = featref.topk(np.array([[-0.0, 0.0, NAN, -1.0]], F32), 4)[0]
    assert [int(g["index"]) for g in got] == [0, 1, 3, -1] and featref.bits(got["value"]).tolist() == [0x80000000, 0, 0xbf800000, 0]


def literal_max(plane):
    """a scalar scan with the contract's order: -0 < +0, any NaN wins"""
    best = None
    for v in plane:
        if v != v:
            return featref.QNAN
        if best is None or v > best or (v == best == 0 and featref.bits(best).ravel()[0] == 0x80000000 and featref.bits(v).ravel()[0] == 0):
            best = v
    return best


def test_max_rules_are_the_literal_loop():
    rng = np.random.default_rng(5501)
    x = rng.integers(-2, 1, (5, 3, 2, 4)).astype(F32)                              # maxima are often zero
    x[rng.random(x.shape) < 0.3] = -0.0
    x[0, 0, 0, 0], x[1, 1] = NAN, -INF
    x[2, 2, 1, 3] = np.array([0xffc00001], np.uint32).view(F32)[0]                 # a negative NaN with a payload: still 0x7fc00000
    x[3, 0], x[3, 1], x[3, 2, 0, :2] = -0.0, 0.0, (-0.0, 0.0)
    got = featref.maxpool(x)
    seen = set()
    for c in range(5):
        for n in range(3):
            want = literal_max(list(x[c, n].reshape(-1)))
            assert featref.bits(got[n, c]) == featref.bits(want), (c, n, x[c, n])
            seen.add(int(featref.bits(want).ravel()[0]))
    assert {0x7fc00000, 0x80000000, 0, 0xff800000} <= seen
    assert featref.bits(featref.flat(x))[1].tolist() == featref.bits(x[:, 1]).reshape(-1).tolist()      # FLAT: CHW order, bit for bit


def literal_relabel(hdr, ent, labels, recs, lists, stride, first, spec):
    """dicts and lists only: copy, then patch"""
    S = stride if lists is not None else 128
    out = []
    for t, r in enumerate(recs):
        c = max(0, min(int(r["count"]), 128))
        if lists is not None:
            m = max(0, min(int(r["nfull"]), S))
            f0 = first[t] if first is not None else t * S
            lst = [list(lists[f0 + i].tolist()) for i in range(m)]
        else:
            lst = [list(r["box"][i].tolist()) for i in range(c)]
        out.append(dict(rec=[list(r["box"][i].tolist()) for i in range(c)] + [[0, 0.0, 0.0, 0.0, 0.0, 0.0]] * (128 - c),
                        lst=lst + [[0, 0.0, 0.0, 0.0, 0.0, 0.0]] * (S - len(lst)), c=c, m=len(lst)))
    for s in range(max(0, min(hdr[1], hdr[3]))):
        t, b, idx, val = int(ent[s]["target"]), int(ent[s]["box"]), int(labels[s][0]["index"]), F32(labels[s][0]["value"])
        if idx < 0 or not val >= spec.min_value or not 0 <= t < len(recs):
            continue
        for boxes, n in ((out[t]["lst"], out[t]["m"]), (out[t]["rec"], out[t]["c"])):
            if 0 <= b < n:
                boxes[b] = [spec.type_base + idx, val if spec.score_mode == 1 else boxes[b][1]] + boxes[b][2:]
    return out


def relabel_case(rng, ntargets, counts, capacity, per_target, with_lists, first_given=False):
    lists = [np.zeros(n, BOX) for n in counts]
    for b in lists:
        for k in range(len(b)):
            x, y = rng.integers(0, 200, 2)
            b[k] = (int(rng.integers(0, 5)), rng.integers(0, 9) / 8, x, y, x + int(rng.integers(1, 50)), y + int(rng.integers(1, 50)))
    recs = np.zeros(ntargets, DETS)
    for t, b in enumerate(lists):
        recs[t]["count"], recs[t]["nfull"], recs[t]["ncand"], recs[t]["overflow"] = min(len(b), 128), len(b), len(b) + 3, t & 5
        recs[t]["box"][:min(len(b), 128)] = b[:128]
    stride = max(1, max(counts)) + 2
    flat = first = None
    if with_lists:
        order = list(rng.permutation(ntargets)) if first_given else list(range(ntargets))
        first = [int(s) * stride + 1 for s in order] if first_given else None
        flat = np.zeros(ntargets * stride + 1, BOX)
        flat.view(np.uint8)[:] = 0x3C
        for t, b in enumerate(lists):
            f0 = first[t] if first_given else t * stride
            flat[f0:f0 + len(b)] = b
    srcs = [{"w": 260, "h": 260} for _ in range(ntargets)]
    seen = lists if with_lists else [b[:128] for b in lists]
    hdr, ent = cropref.select(srcs, seen, cropref.Spec(8, 8, per_target=per_target, min_score=0.25), capacity)
    k = int(rng.integers(1, 4))
    labels = np.zeros((capacity, k), LABEL)
    labels["index"] = rng.integers(-1, 6, (capacity, k))
    labels["value"] = rng.integers(0, 9, (capacity, k)) / 8
    labels["value"][rng.random((capacity, k)) < 0.1] = NAN
    return hdr, ent, labels, recs, flat, stride, first


def test_relabel_is_the_literal_loop():
    rng = np.random.default_rng(5502)
    seen = dict.fromkeys(("patched", "rejected", "behind_count", "empty_table", "cut"), 0)
    cases = [(3, (5, 0, 140), 9, 4, True, False), (2, (130, 131), 300, 200, True, True), (4, (3, 9, 0, 1), 4, 2, False, False), (2, (0, 0), 3, 1, True, False),
             (3, (7, 7, 7), 5, 7, True, True)]
    for ci, (nt, counts, cap, per, with_lists, fg) in enumerate(cases):
        for mode in (0, 1):
            hdr, ent, labels, recs, flat, stride, first = relabel_case(rng, nt, counts, cap, per, with_lists, fg)
            if ci == 4:                                                            # entries whose target is outside 0 .. ntargets-1 are ignored
                assert hdr[1] >= 3
                ent[0]["target"], ent[2]["target"] = nt + 3, -5
                seen["foreign_target"] = seen.get("foreign_target", 0) + 1
            spec = featref.RelabelSpec(0.25, 1000, mode)
            got_r, got_l = featref.relabel(hdr, ent, labels, recs, flat, stride, first, spec)
            want = literal_relabel(hdr, ent, labels, recs, flat, stride, first, spec)
            S = stride if with_lists else 128
            for t in range(nt):
                for f in ("count", "ncand", "overflow", "nfull"):
                    assert got_r[t][f] == recs[t][f]
                assert np.array([tuple(b) for b in want[t]["rec"]], BOX).tobytes() == got_r[t]["box"].tobytes(), (ci, mode, t)
                assert np.array([tuple(b) for b in want[t]["lst"]], BOX).tobytes() == got_l[t * S:(t + 1) * S].tobytes(), (ci, mode, t)
            seen["patched"] += int((got_r["box"]["type"] >= 1000).sum())
            seen["behind_count"] += int((got_l["type"].reshape(nt, S)[:, 128:] >= 1000).sum()) if S > 128 else 0
            ok = (labels[:hdr[1], 0]["index"] >= 0) & (labels[:hdr[1], 0]["value"] >= F32(0.25))
            seen["rejected"] += int((~ok).sum())
            seen["empty_table"] += int(hdr[1] == 0)
            seen["cut"] += int(hdr[0] > hdr[3])
            if mode == 0:
                assert (got_r["box"]["score"] == recs["box"]["score"]).all()
    assert all(n > 0 for n in seen.values()), seen


def test_softmax_and_l2_references():
    """the special rows of the contract, and the references against a plain float64 evaluation"""
    for row in ([1, NAN, 2], [1, INF], [-INF, -INF], [-INF]):
        assert np.isnan(featref.softmax64(np.array(row, F32))[0]).all(), row
    ref, bound = featref.softmax64(np.array([0, -INF, 0], F32))
    assert ref.tolist() == [0.5, 0.0, 0.5] and bound[1] == 2.0 ** -126
    ref, _ = featref.softmax64(np.array([1, 2, 3], F32))
    assert abs(ref.sum() - 1) < 1e-15 and np.allclose(ref, np.exp([1, 2, 3]) / np.exp([1, 2, 3]).sum())
    assert featref.l2_64(np.zeros(4, F32))[0].tolist() == [0.0] * 4
    ref, bound = featref.l2_64(np.array([3, 4], F32))
    assert ref.tolist() == [0.6, 0.8] and (bound > 0).all()
    m, b = featref.mean64(np.arange(24, dtype=F32).reshape(2, 3, 2, 2))
    assert m.shape == (3, 2) and m[1, 0] == 5.5 and m[2, 1] == 21.5 and (b > 0).all()


def test_features_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_features_dev(None, 1, 1, 1, 1, 0, 0, None, 1, None),
                 lambda: L.ffgpu_exec_features(None, None, None, 1, None),
                 lambda: L.ffgpu_topk_dev(None, 1, 1, 1, 1, None, None),
                 lambda: L.ffgpu_crops_relabel_dev(None, 1, None, 1, None, None, 0, None, 1, None, None, None, None),
                 lambda: L.ffgpu_exec_relabel(None, 0, None, 1, None, 1, 1, None, None, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs
