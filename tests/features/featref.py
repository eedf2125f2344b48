"""The numpy restatement of the feature / top-k / relabel contract of include/ffcnn_hip.h ("the crops classified on the device").  Nothing of the
kernels' method is in here: rows are built with reshapes and float64 sums, the top-k is a sort, the relabelling a loop over the table.
tests/test_features_abi.py pins the parts that could hide a mistake (top-k order, the MAX rules, relabel) to literal scalar loops."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (128,))])
LABEL_DTYPE = np.dtype([("index", "<i4"), ("value", "<f4")])
MAX_DET = 128
FLAT, MEAN, MAX = 0, 1, 2
NONE, SOFTMAX, L2 = 0, 1, 2
KEEP_SCORE, LABEL_SCORE = 0, 1
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
U = 2.0 ** -24                                                     # the unit roundoff of fp32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dim(c, h, w, pool):
    return c * h * w if pool == FLAT else c


# ---- pooling.  x: the tensor as (C, N, H, W) fp32 (the device layout); rows come back as (N, D)
def flat(x):
    """the frame's tensor in CHW order, bit for bit"""
    C, N, H, W = x.shape
    return np.ascontiguousarray(bits(x).transpose(1, 0, 2, 3).reshape(N, C * H * W)).view(np.float32)


def mean64(x):
    """(the float64 mean of each plane, the contract's error bound for an fp32 sum in any order followed by one division), both (N, C)"""
    C, N, H, W = x.shape
    hw = H * W
    with np.errstate(invalid="ignore", over="ignore"):
        p = x.astype(np.float64).reshape(C, N, hw)
        m = p.sum(axis=2) / hw
        g = (hw - 1) * U / (1 - (hw - 1) * U)
        bound = g * (np.abs(p).sum(axis=2) / hw) + U * np.abs(m) + 2.0 ** -149
    return m.T, bound.T


def maxpool(x):
    """the plane's maximum: any NaN gives the quiet NaN 0x7fc00000; of zeros -0 < +0"""
    C, N, H, W = x.shape
    p = np.ascontiguousarray(x, np.float32).reshape(C, N, H * W)
    nan = np.isnan(p).any(axis=2)
    m = np.where(nan, np.float32(0), np.max(np.where(np.isnan(p), -np.inf, p), axis=2)).astype(np.float32)
    zero = ~nan & (m == 0)                                         # a zero maximum: +0 if the plane holds one, else -0
    plus = (bits(p) == 0).any(axis=2)
    m[zero & plus] = np.float32(0.0)
    m[zero & ~plus] = np.float32(-0.0)
    m[nan] = QNAN
    return np.ascontiguousarray(m.T)


# ---- the row operations, in float64 on the fp32 row: (reference, bound) per element
def softmax64(row):
    row = np.asarray(row, np.float32)
    D = len(row)
    if np.isnan(row).any() or np.isposinf(row).any() or np.isneginf(row).all():
        return np.full(D, np.nan), np.zeros(D)
    x = row.astype(np.float64)
    m = x.max()
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x - m)
        ref = e / e.sum()
        gap = np.where(np.isinf(x), 0.0, m - x)                    # (-Inf: the reference is 0, only the absolute term is left)
        bound = (D + 16 + gap) * U * ref + 2.0 ** -126
    return ref, bound


def l2_64(row):
    row = np.asarray(row, np.float32)
    D = len(row)
    x = row.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        r = np.sqrt((x * x).sum())
        if r == 0:
            return np.zeros(D), np.zeros(D)
        ref = x / r
        return ref, (D / 2 + 3) * U * np.abs(ref) + 2.0 ** -149


# ---- top-k
def topk(rows, k):
    """(n, k) LABEL_DTYPE: value descending as fp32 values compare, then index ascending (+0 and -0 tie); NaN never; missing entries { -1, 0.0 }"""
    rows = np.asarray(rows, np.float32)
    out = np.zeros((len(rows), k), LABEL_DTYPE)
    out["index"] = -1
    for r, v in enumerate(rows):
        idx = np.nonzero(~np.isnan(v))[0]
        order = idx[np.lexsort((idx, -v[idx]))][:k]                # (lexsort: the LAST key is the primary one; -0.0 == 0.0 there as well)
        out[r, :len(order)]["index"] = order
        out[r, :len(order)]["value"] = v[order]
    return out


# ---- relabel
class RelabelSpec:
    def __init__(self, min_value=0.0, type_base=0, score_mode=KEEP_SCORE):
        self.min_value, self.type_base, self.score_mode = np.float32(min_value), int(type_base), int(score_mode)


def relabel(header, entries, labels, recs, lists, stride, first, spec, with_lists=True):
    """header = (total, taken, empty, capacity) and entries as cropref.select leaves them; labels: (capacity, k) LABEL_DTYPE; recs: DETS_DTYPE;
    lists: the flat BOX array or None (the records' own boxes, stride 128); first: list t's first box or None (t * stride).  Returns the
    relabelled (records, lists as a (ntargets * S) BOX array or None)."""
    n = len(recs)
    S = stride if lists is not None else MAX_DET
    out_r = np.zeros(n, DETS_DTYPE)
    out_l = np.zeros((n, S), BOX_DTYPE) if with_lists else None
    nrec, nlist = [], []
    for t in range(n):
        r = recs[t]
        c = max(0, min(int(r["count"]), MAX_DET))
        for f in ("count", "ncand", "overflow", "nfull"):
            out_r[t][f] = r[f]
        out_r[t]["box"][:c] = r["box"][:c]
        if lists is not None:
            m = max(0, min(int(r["nfull"]), S))
            f0 = first[t] if first is not None else t * S
            src = lists[f0:f0 + m]
        else:
            m, src = c, r["box"][:c]
        if with_lists:
            out_l[t, :m] = src
        nrec.append(c)
        nlist.append(m)
    taken = max(0, min(int(header[1]), int(header[3])))
    for s in range(taken):
        e = entries[s]
        t, b = int(e["target"]), int(e["box"])
        if not 0 <= t < n or b < 0:
            continue
        lab = labels[s, 0]
        if int(lab["index"]) < 0 or not (np.float32(lab["value"]) >= spec.min_value):      # (False for a NaN value)
            continue
        ty = np.int32((spec.type_base + int(lab["index"]) + 2 ** 31) % 2 ** 32 - 2 ** 31)
        if with_lists and b < nlist[t]:
            out_l[t, b]["type"] = ty
            if spec.score_mode == LABEL_SCORE:
                out_l[t, b]["score"] = lab["value"]
        if b < nrec[t]:
            out_r[t]["box"][b]["type"] = ty
            if spec.score_mode == LABEL_SCORE:
                out_r[t]["box"][b]["score"] = lab["value"]
    return out_r, (out_l.reshape(-1) if with_lists else None)
