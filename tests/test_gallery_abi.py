"""Re-identification on the device, without a GPU: the exported symbols, the layout of ffgpu_gallery in the ctypes mirror and in the header, the
contract's sentences in the header, ffgpu_match_workspace_bytes, tests/gallery/matchref.py (the numpy restatement the GPU tests compare with) pinned to
hand-written scalar cases -- ties, -0 against +0, NaN, k beyond the rows, a full gallery, a non-finite row -- and the device entry points failing the
way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gallery import matchref

SYMBOLS = ["ffgpu_match_workspace_bytes", "ffgpu_match_dev", "ffgpu_gallery_enroll_dev"]
NAN, INF = float("nan"), float("inf")
F32 = np.float32
LABEL = matchref.LABEL_DTYPE


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_gallery_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s
    for name in ("gallery", "match_workspace_bytes", "match_dev", "gallery_enroll_dev"):
        assert getattr(capi.FFGPU, name) is getattr(capi, name)


def test_gallery_struct_layout(capi):
    """ctypes and the header's own statement of the offsets agree, and the fields fill the struct: no hidden padding"""
    G = capi.Gallery
    fields = ("d_rows", "d_ids", "d_head", "row_stride", "capacity", "d")
    assert C.sizeof(G) == 40 and [getattr(G, f).offset for f in fields] == [0, 8, 16, 24, 32, 36]
    assert sum(getattr(G, f).size for f in fields) == C.sizeof(G)
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    m = re.search(r"\}\s*ffgpu_gallery;\s*/\*\s*(\d+) bytes:([^*]*)\*/", hdr)
    stated = {n: int(o) for n, o in re.findall(r"(\w+) (\d+)", m.group(2))}
    assert int(m.group(1)) == C.sizeof(G) and stated == {f: getattr(G, f).offset for f in fields}
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*ffgpu_gallery;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == list(fields)                           # the header declares them in this order
    g = capi.gallery(4096, 7, 5)
    assert (g.d_rows, g.d_ids, g.d_head, g.row_stride, g.capacity, g.d) == (4096, None, None, 5, 7, 5)
    g = capi.gallery(4096, 7, 5, d_ids=8, d_head=16, row_stride=9)
    assert (g.d_ids, g.d_head, g.row_stride) == (8, 16, 9)
    assert matchref.HEAD_DTYPE.itemsize == 16 and matchref.HEAD_DTYPE.names == ("count", "issued", "dropped", "reserved")


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    flat = " ".join(hdr.replace("*", " ").split())
    for sentence in ("} ffgpu_gallery;", "a HOST struct of device pointers, free again on return",
                     "row g at d_rows + g row_stride (floats), row_stride >= d", "d_ids[g] < 0: row g is disabled",
                     "{ int count, issued, dropped, reserved }", "NULL: count = capacity", "All-zero = the valid empty gallery",
                     "`count` is read ON THE DEVICE", "1 .. 2^20", "1 .. 4096",
                     "sim(q, g) is the dot product of query row q and gallery row g, in fp32", "it is a FIXED order",
                     "independent of q, nq, g, capacity, count, the strides and every alignment",
                     "a pair of rows gives the same bits wherever it stands", "A row behind count, or a disabled row, has sim = 0x7fc00000",
                     "row q at byte 8 k q", "sim descending, as fp32 values compare; then gallery row g ascending", "NaN is never selected",
                     "Missing entries are { -1, 0.0f }", "index is d_ids[g], or g when d_ids is NULL", "value is sim(q, g)",
                     "d_sim may be NULL", "sim_stride >= capacity", "nothing else is written", "The labels are the same bytes with and without d_sim",
                     "Every byte of d_out_labels is written", "nq is 1..4096, k is 1..FFGPU_TOPK_MAX", "Pointers need only 4-byte alignment",
                     "with the same bits either way", "At most two launches per call", "No synchronisation",
                     "A rejected call launches nothing and leaves everything usable", "pure host code; 0 for arguments outside their ranges",
                     "d_ids and d_head are required", "only entry 0 of each row is used, k is passed for the row pitch",
                     "matched when index >= 0 and value >= min_value (a NaN value never)", "if every element of the row is finite and a slot is left",
                     "the e-th enrolled row of the call takes slot count + e", "copied there bit for bit", "d_ids[slot] = issued + e + 1",
                     "out[r] = { that id, min_value }", "out[r] = { -1, 0.0f } and `dropped` counts it",
                     "count and issued have grown by the number enrolled", "it must not overlap d_labels",
                     "Two unknown queries of one call are two identities, even if their rows are equal",
                     "one workgroup that decides, then a grid that copies"):
        assert sentence in flat, sentence
    inc = open(os.path.join(ROOT, "ffcnn_amd", "csrc", "ffgpu_kernels.hip")).read()
    assert inc.index('#include "ffgpu_feature.inc"') < inc.index('#include "ffgpu_match.inc"')
    src = open(os.path.join(ROOT, "ffcnn_amd", "csrc", "ffgpu_match.inc")).read()
    assert not re.search(r"\batomic\w*\s*\(", src) and "__builtin_amdgcn_mfma_f32_16x16x4f32" in src
    assert "hipStreamSynchronize" not in src and "hipDeviceSynchronize" not in src and "hipMemcpy" not in src


def test_workspace_bytes_is_pure_host_code(capi):
    """no device needed; monotone in each argument; 0 outside the ranges"""
    wb = capi.match_workspace_bytes
    assert wb(1, 1, 1) >= 8
    for nq, cap, k in ((0, 1, 1), (-1, 1, 1), (4097, 1, 1), (1, 0, 1), (1, -5, 1), (1, 2 ** 20 + 1, 1), (1, 1, 0), (1, 1, 17), (1, 1, -1),
                       (2 ** 31 - 1, 2 ** 31 - 1, 16)):
        assert wb(nq, cap, k) == 0, (nq, cap, k)
    assert wb(4096, 2 ** 20, 16) > 2 ** 32                                         # (a size_t, not an int)
    nqs, caps, ks = (1, 2, 15, 16, 17, 63, 64, 65, 256, 4095, 4096), (1, 2, 63, 64, 65, 127, 128, 129, 1000, 65536, 2 ** 20 - 1, 2 ** 20), tuple(range(1, 17))
    for cap in caps:
        for k in ks:
            v = [wb(nq, cap, k) for nq in nqs]
            assert all(a > 0 for a in v) and v == sorted(v), (cap, k)
    for nq in nqs:
        for k in ks:
            v = [wb(nq, cap, k) for cap in caps]
            assert v == sorted(v), (nq, k)
        for cap in caps:
            v = [wb(nq, cap, k) for k in ks]
            assert v == sorted(v) and len(set(v)) == len(v), (nq, cap)


# ------------------------------------------------------------------------------------------------- matchref against hand-written cases
def labels(*pairs):
    return np.array(list(pairs), LABEL)


def test_matchref_selection_by_hand():
    # ties: the lower gallery row wins, whatever its id; ids repeat and each row still takes an entry
    sim = np.array([[2, 5, 5, 1, 5]], F32)
    assert matchref.select(sim, 3).tolist() == [[(1, 5.0), (2, 5.0), (4, 5.0)]]
    assert matchref.select(sim, 4, ids=[70, 9, 3, 9, 3]).tolist() == [[(9, 5.0), (3, 5.0), (3, 5.0), (70, 2.0)]]
    # -0 against +0: they tie, the lower row wins and keeps its own sign
    got = matchref.select(np.array([[-1, -0.0, 0.0], [-1, 0.0, -0.0]], F32), 2)
    assert got["index"].tolist() == [[1, 2], [1, 2]]
    assert got["value"].view(np.uint32).tolist() == [[0x80000000, 0], [0, 0x80000000]]
    # NaN is never selected; k beyond the rows pads with { -1, 0.0 }
    got = matchref.select(np.array([[NAN, 3, NAN, -INF, INF]], F32), 5, ids=[5, 6, 7, 8, 9])
    assert got["index"].tolist() == [[9, 6, 8, -1, -1]] and got["value"].view(np.uint32).tolist() == [[0x7f800000, 0x40400000, 0xff800000, 0, 0]]
    assert matchref.select(np.full((2, 3), NAN, F32), 2).tobytes() == labels((-1, 0), (-1, 0), (-1, 0), (-1, 0)).tobytes()
    assert matchref.select(np.array([[4]], F32), 16)[0].tolist() == [(0, 4.0)] + [(-1, 0.0)] * 15
    # the matrix: float64 dot products of the fp32 rows; rows behind count and disabled rows are NaN
    q = np.array([[1, 2, 3], [0, 0, 1]], F32)
    rows = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 1], [5, 5, 5]], F32)
    s, mag = matchref.sim64(q, rows)
    assert s.tolist() == [[1, 2, 6, 30], [0, 0, 1, 5]] and mag.tolist() == s.tolist()
    s, _ = matchref.sim64(q, rows, count=3, ids=[4, -1, 6, 7])
    assert np.isnan(s).tolist() == [[False, True, False, True]] * 2 and s[0, 2] == 6
    assert np.isnan(matchref.sim64(q, rows, count=0)[0]).all() and not np.isnan(matchref.sim64(q, rows, count=9)[0]).any()
    s, mag = matchref.sim64(np.array([[1, -1]], F32), np.array([[3, 3]], F32))
    assert s.tolist() == [[0]] and mag.tolist() == [[6]] and matchref.bound(mag, 2)[0, 0] == 2 * 2.0 ** -24 / (1 - 2 * 2.0 ** -24) * 6 + 2 * 2.0 ** -149


def test_matchref_enrolment_by_hand():
    T = F32(0.5)
    rows, ids, head = np.full((4, 2), 9, F32), np.full(4, -7, np.int32), np.zeros((), matchref.HEAD_DTYPE)
    rows[0], ids[0] = (1, 0), 11
    head["count"], head["issued"], head["dropped"], head["reserved"] = 1, 20, 2, 77
    q = np.array([[1, 0], [0, 1], [0, 1], [INF, 0], [3, -0.0], [2, 2], [1, 0], [7, 7]], F32)
    lab = np.zeros((8, 2), LABEL)
    lab[:, 1] = (99, 9.0)                                                          # entry 1 is never looked at
    lab[:, 0] = [(11, 1.0), (11, 0.0), (-1, 0.0), (-1, 0.0), (11, NAN), (11, 0.25), (11, 0.5), (5, 0.4999)]
    out = matchref.enroll(rows, ids, head, q, lab, T)
    # r0 matched; r1, r2 two identities though their rows are equal; r3 not finite: dropped; r4 a NaN value is no match: enrolled, -0 kept;
    # r5 the gallery is full: dropped; r6 value == min_value: matched; r7 full: dropped
    assert out.tolist() == [(11, 1.0), (21, 0.5), (22, 0.5), (-1, 0.0), (23, 0.5), (-1, 0.0), (11, 0.5), (-1, 0.0)]
    assert ids.tolist() == [11, 21, 22, 23] and head.tolist() == (4, 23, 5, 77)
    assert rows.view(np.uint32).tolist() == np.array([[1, 0], [0, 1], [0, 1], [3, -0.0]], F32).view(np.uint32).tolist()
    # a full gallery enrols nobody and keeps matching; an index < 0 never matches whatever its value
    out = matchref.enroll(rows, ids, head, q[:2], labels((22, 0.75), (-1, 5.0)).reshape(2, 1), T)
    assert out.tolist() == [(22, 0.75), (-1, 0.0)] and head.tolist() == (4, 23, 6, 77) and ids.tolist() == [11, 21, 22, 23]
    # the empty gallery of an all-zero head
    rows, ids, head = np.zeros((2, 1), F32), np.zeros(2, np.int32), np.zeros((), matchref.HEAD_DTYPE)
    out = matchref.enroll(rows, ids, head, np.array([[4], [NAN], [5], [6]], F32), labels(*[(-1, 0.0)] * 4).reshape(4, 1), 0.0)
    assert out.tolist() == [(1, 0.0), (-1, 0.0), (2, 0.0), (-1, 0.0)] and head.tolist() == (2, 2, 2, 0) and rows.tolist() == [[4], [5]] and ids.tolist() == [1, 2]


def test_gallery_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_match_dev(None, 1, 1, None, 1, None, None, 1, None, 0, None),
                 lambda: L.ffgpu_gallery_enroll_dev(None, None, 1, 1, None, 1, 0.0, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs
