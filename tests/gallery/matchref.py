"""The numpy restatement of the re-identification contract of include/ffcnn_hip.h ("re-identification on the device").  Nothing of the kernels' method
is in here: the similarity matrix is float64 dot products of the fp32 rows, the selection is features.featref.topk (a sort) over a given matrix with the
id mapping applied afterwards, the enrolment a literal loop over the queries.  tests/test_gallery_abi.py pins selection and enrolment to hand-written
scalar cases."""
import numpy as np

from features import featref

LABEL_DTYPE = featref.LABEL_DTYPE
HEAD_DTYPE = np.dtype([("count", "<i4"), ("issued", "<i4"), ("dropped", "<i4"), ("reserved", "<i4")])
QNAN = featref.QNAN
MAX_NQ, MAX_CAPACITY, MAX_D, TOPK_MAX = 4096, 2 ** 20, 4096, 16
U = 2.0 ** -24


def live(capacity, count=None, ids=None):
    """which gallery rows are there: g < count (None: capacity; clamped to 0 .. capacity) and ids[g] >= 0 (None: all)"""
    c = capacity if count is None else max(0, min(int(count), capacity))
    on = np.arange(capacity) < c
    if ids is not None:
        on &= np.asarray(ids)[:capacity] >= 0
    return on


def sim64(q, rows, count=None, ids=None):
    """(the (nq, capacity) float64 dot products of the fp32 rows, NaN for rows that are not there or are disabled; the sums of |a_k b_k|)"""
    q64, r64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(rows, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = q64[:, None, :] * r64[None, :, :]
        s, mag = prod.sum(axis=2), np.abs(prod).sum(axis=2)
    s[:, ~live(len(r64), count, ids)] = np.nan
    return s, mag


def bound(mag, d):
    """the bound of an fp32 dot product of d terms in any order, with or without fused multiply-adds: gamma_d sum|a_k b_k| + d 2^-149"""
    return d * U / (1 - d * U) * mag + d * 2.0 ** -149


def select(sim, k, ids=None):
    """(nq, k) LABEL_DTYPE from a similarity matrix (fp32; NaN = not there): featref.topk's order over the gallery rows g, then index = ids[g]"""
    out = featref.topk(np.asarray(sim, np.float32), k)
    if ids is not None:
        g = out["index"].copy()
        out["index"] = np.where(g >= 0, np.asarray(ids, np.int32)[np.maximum(g, 0)], -1)
    return out


def enroll(rows, ids, head, q, labels, min_value):
    """the contract, query by query; rows (capacity, d) fp32, ids (capacity,) i4 and head (a HEAD_DTYPE scalar array) are changed in place; labels is
    (nq, k) LABEL_DTYPE of which entry 0 counts.  Returns the (nq,) LABEL_DTYPE output."""
    q = np.asarray(q, np.float32)
    capacity = len(rows)
    min_value = np.float32(min_value)
    out = np.zeros(len(q), LABEL_DTYPE)
    count, issued, dropped = max(0, min(int(head["count"]), capacity)), int(head["issued"]), int(head["dropped"])
    for r in range(len(q)):
        lab = labels[r, 0]
        if int(lab["index"]) >= 0 and np.float32(lab["value"]) >= min_value:           # (False for a NaN value)
            out[r] = lab
        elif np.isfinite(q[r]).all() and count < capacity:
            rows[count].view(np.uint32)[:] = q[r].view(np.uint32)
            issued += 1
            ids[count] = issued
            out[r] = (issued, min_value)
            count += 1
        else:
            out[r] = (-1, 0.0)
            dropped += 1
    head["count"], head["issued"], head["dropped"] = count, issued, dropped
    return out
