"""Cutting the detections out of the frames, without a GPU: the exported symbols, the layout of ffgpu_crop_spec / ffgpu_crop in the ctypes mirror
and the constants in the header, tests/crops/cropref.py (the numpy restatement of the contract the GPU tests compare with) pinned to the
reference's own net_input through the oracle and to a literal per-pixel loop, its corner cases, and the device entry points failing the way every
entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from crops import cropref

SYMBOLS = ["ffgpu_crop_table_bytes", "ffgpu_crop_slot_bytes", "ffgpu_crop_boxes_bgr_dev", "ffgpu_crop_boxes_nv12_dev", "ffgpu_exec_crop_bgr",
           "ffgpu_exec_crop_nv12", "ffgpu_crops_to_source_dev"]
NAN, BIG = float("nan"), 1e30


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def boxes_of(rows):
    """rows: (x1, y1, x2, y2[, type[, score]])"""
    b = np.zeros(len(rows), cropref.BOX_DTYPE)
    for k, r in enumerate(rows):
        b[k] = (r[4] if len(r) > 4 else 0, r[5] if len(r) > 5 else 0.5, r[0], r[1], r[2], r[3])
    return b


def src(w, h):
    return {"w": w, "h": h}


def test_crop_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_crop_struct_layout(capi):
    S, E = capi.CropSpec, capi.Crop
    assert C.sizeof(S) == 72 and C.sizeof(E) == 48
    assert [getattr(S, f).offset for f in ("out_w", "out_h", "form", "per_target", "min_score", "nclasses", "classes", "margin_num", "margin_den",
                                           "mean", "norm", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 32, 36, 40, 52, 64]
    assert [getattr(E, f[0]).offset for f in E._fields_] == list(range(0, 48, 4))
    assert capi.CROP_DTYPE == cropref.CROP_DTYPE and capi.CROP_DTYPE.itemsize == 48 and cropref.BOX_DTYPE == capi.BOX_DTYPE
    assert (capi.CROP_F32, capi.CROP_U8, capi.CROP_ENTRIES, capi.CROP_MERGED) == (0, 1, 0, 1) == (cropref.F32, cropref.U8, 0, 1)
    sp = capi.crop_spec(96, 64, capi.CROP_U8, per_target=3, min_score=0.25, classes=[0, 1, 1], margin=(1, 8), mean=(1, 2, 3), norm=(4, 5, 6))
    assert (sp.out_w, sp.out_h, sp.form, sp.per_target, sp.min_score, sp.nclasses, sp.margin_num, sp.margin_den, sp.reserved) == (96, 64, 1, 3, 0.25, 3, 1, 8, 0)
    assert C.string_at(sp.classes, 3) == bytes([0, 1, 1]) and list(sp.mean) == [1, 2, 3] and list(sp.norm) == [4, 5, 6]
    sp = capi.crop_spec(32, 32)
    assert (sp.classes, sp.nclasses, sp.margin_num, sp.margin_den) == (None, 0, 0, 1)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    assert "} ffgpu_crop_spec;" in hdr and "} ffgpu_crop;" in hdr and "72 bytes" in hdr and "48 bytes" in hdr
    for name, val in (("FFGPU_CROP_F32", 0), ("FFGPU_CROP_U8", 1), ("FFGPU_CROP_ENTRIES", 0), ("FFGPU_CROP_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(ROOT, "ffcnn_amd", "csrc", "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_crop.inc"' in inc


def test_sizes_are_pure_host_code(capi):
    """no device needed: the table's and a slot's bytes, 0 for arguments outside their ranges"""
    assert [capi.crop_table_bytes(c) for c in (-1, 0, 1, 4, 1000)] == [0, 0, 64, 16 + 4 * 48, 16 + 48000]
    assert capi.crop_slot_bytes(320, 320, 0) == 3 * 320 * 320 * 4 and capi.crop_slot_bytes(5, 7, 0) == 3 * 5 * 7 * 4
    assert capi.crop_slot_bytes(5, 7, 1) == 7 * 16 and capi.crop_slot_bytes(1, 1, 1) == 4 and capi.crop_slot_bytes(96, 64, 1) == 64 * 288
    assert [capi.crop_slot_bytes(*a) for a in ((0, 1, 0), (1, 0, 1), (4097, 1, 0), (1, 4097, 1), (8, 8, 2), (8, 8, -1))] == [0] * 6
    for w, h in ((1, 1), (5, 7), (96, 64)):
        for form in (0, 1):
            assert capi.crop_slot_bytes(w, h, form) == cropref.slot_nbytes(cropref.Spec(w, h, form))


# ------------------------------------------------------------------------------------------------- cropref against the reference's net_input
def as_image(pix):
    """a region copied out as an image of its own, rows padded as net_input reads them (ffcnn.c:262)"""
    h, w = pix.shape[:2]
    rows = np.zeros((h, cropref.align4(3 * w)), np.uint8)
    rows[:, :3 * w] = pix.reshape(h, 3 * w)
    return rows


def regions_for(rng, w, h):
    """whole picture, seeded rectangles, one-pixel regions and the degenerate ones whose letterbox has sw == 0 or sh == 0 (where the picture allows)"""
    out = [(0, 0, w, h), (w - 1, h - 1, 1, 1), (0, 0, 1, 1), (0, h // 2, w, 1), (w // 2, 0, 1, h)]
    for _ in range(6):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        out.append((x0, y0, int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1))))
    return out


@pytest.mark.parametrize("geom", [(32, 32), (96, 64), (320, 320)])
def test_cropref_f32_slot_is_the_references_net_input(orc, capi, geom):
    """for regions of data/test.bmp and of random images: cropref's F32 slot == Oracle(w, h).set_input_image(the region copied out), bit for bit"""
    rng = np.random.default_rng(5300 + geom[0])
    W, H = geom
    rows, w, h = capi.load_bmp(os.path.join(capi.DATA, "test.bmp"))
    pictures = [np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))]
    pictures += [rng.integers(0, 256, (ph, pw, 3), dtype=np.uint8) for pw, ph in ((1, 1), (7, 5), (333, 257), (2000, 3), (3, 1500))]
    o = orc.Oracle(w=W, h=H)
    assert o.input.shape == (3, H, W)
    degenerate = 0
    try:
        for case, img in enumerate(pictures):
            for setting in (((0.0, 0.0, 0.0), (1 / 255.0,) * 3), ((104.0, 117.0, 123.0), (0.017, 0.0175, 0.0171))):
                for x0, y0, rw, rh in regions_for(rng, img.shape[1], img.shape[0]):
                    e = np.zeros(1, cropref.CROP_DTYPE)[0]
                    e["x0"], e["y0"], e["w"], e["h"] = x0, y0, rw, rh
                    e["sw"], e["sh"], e["s1"], e["s2"] = cropref.letterbox(rw, rh, W, H)
                    degenerate += int(e["sw"]) == 0 or int(e["sh"]) == 0
                    got = cropref.slot_f32(cropref.slot_pixels(img, e, W, H), e, *setting)
                    o.set_input_image(as_image(img[y0:y0 + rh, x0:x0 + rw]), rw, rh, *setting)
                    assert got.tobytes() == o.input.tobytes(), (case, x0, y0, rw, rh)
    finally:
        o.close()
    assert degenerate > 0


def test_cropref_slices_are_the_literal_loop():
    rng = np.random.default_rng(5310)
    for case in range(150):
        w, h, W, H = (int(v) for v in rng.integers(1, 24, 4))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        rw, rh = int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1))
        e = np.zeros(1, cropref.CROP_DTYPE)[0]
        e["x0"], e["y0"], e["w"], e["h"] = x0, y0, rw, rh
        e["sw"], e["sh"], e["s1"], e["s2"] = cropref.letterbox(rw, rh, W, H)
        a, b = cropref.slot_pixels(img, e, W, H), cropref.slot_pixels_literal(img, e, W, H)
        assert a.tobytes() == b.tobytes(), case
        u8 = cropref.slot_u8(a)
        assert u8.shape == (H, cropref.align4(3 * W)) and u8[:, :3 * W].tobytes() == a.tobytes() and not u8[:, 3 * W:].any()
        f = cropref.slot_f32(a, e, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0))
        for p in range(3):
            for y in range(H):
                for x in range(W):
                    inside = x < int(e["sw"]) and y < int(e["sh"])
                    want = (np.float32(a[y, x, 2 - p]) - np.float32((1.0, 2.0, 3.0)[p])) * np.float32((0.5, 0.25, 2.0)[p]) if inside else np.float32(0)
                    assert f[p, y, x] == want


def test_cropref_nv12_picture_is_the_headers_formula():
    """odd sizes, every matrix: pixel by pixel with nearest chroma at the picture's coordinates"""
    rng = np.random.default_rng(5311)
    for matrix in range(4):
        w, h = 7, 5
        Y = rng.integers(0, 256, (h, w + 2), dtype=np.uint8)
        UV = rng.integers(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2) + 2), dtype=np.uint8)
        pic = cropref.nv12_picture(Y, UV, w, h, matrix)
        yoff, cy, crv, cgu, cgv, cbu = cropref.MATS[matrix]
        for y in range(h):
            for x in range(w):
                c, d, e = int(Y[y, x]) - yoff, int(UV[y >> 1, 2 * (x >> 1)]) - 128, int(UV[y >> 1, 2 * (x >> 1) + 1]) - 128
                want = [min(max(v >> 8, 0), 255) for v in (cy * c + cbu * d + 128, cy * c - cgu * d - cgv * e + 128, cy * c + crv * e + 128)]
                assert list(pic[y, x]) == want


# ------------------------------------------------------------------------------------------------- selection
def entries_of(sources, lists, spec, capacity=8, stats=None):
    hdr, ent = cropref.select(sources, lists, spec, capacity, stats)
    return hdr, [tuple(int(e[f]) for f in ("target", "box", "x0", "y0", "w", "h")) for e in ent[:hdr[1]]]


def test_cropref_selection_properties():
    S = cropref.Spec
    # NaN corners are 0; a NaN score never qualifies; +-1e30 saturates and the region is the source
    hdr, ent = entries_of([src(20, 10)], [boxes_of([(NAN, NAN, 4.9, 3.2), (1, 1, 2, 2, 0, NAN), (-BIG, -BIG, BIG, BIG)])], S(8, 8, per_target=9))
    assert hdr == (2, 2, 0, 8) and ent == [(0, 0, 0, 0, 5, 4), (0, 2, 0, 0, 20, 10)]
    # inverted boxes and boxes wholly outside are counted in empty, wherever they stand, and take nothing
    stats = {}
    hdr, ent = entries_of([src(20, 10)], [boxes_of([(8, 2, 3, 5), (3, 7, 8, 2), (1, 1, 2, 2), (25, 1, 30, 4), (1, -9, 4, -2), (BIG, BIG, BIG, BIG), (5, 5, 5, 5)])],
                          S(8, 8, per_target=1), stats=stats)
    assert hdr == (1, 1, 5, 8) and ent == [(0, 2, 1, 1, 2, 2)] and stats["empty"] == 5 and stats["cut_per_target"] == 1
    # margins in 64-bit integers: (c - a + 1) num / den each way, clipped at each edge
    for box, margin, want, edges in (((4, 3, 11, 6), (1, 8), (3, 3, 10, 4), ""), ((4, 3, 11, 6), (4, 1), (0, 0, 20, 10), "lrtb"), ((0, 3, 3, 6), (1, 2), (0, 1, 6, 8), "l"),
                                     ((15, 0, 19, 1), (1, 1), (10, 0, 10, 4), "rt"), ((2, 8, 3, 9), (1, 1), (0, 6, 6, 4), "b"), ((-BIG, 2, BIG, 3), (4, 1), (0, 0, 20, 10), "lrtb")):
        stats = {}
        hdr, ent = entries_of([src(20, 10)], [boxes_of([box])], S(8, 8, margin=margin), stats=stats)
        assert ent == [(0, 0) + want], (box, margin, ent)
        assert {k[5:] for k in stats if k.startswith("clip_")} == set(edges), (box, stats)
    # the class filter: negative and >= nclasses types never pass; NULL classes passes everything
    lists = [boxes_of([(1, 1, 2, 2, t) for t in (-1, 0, 1, 2, 3, -2 ** 31, 2 ** 31 - 1, 256)])]
    assert [e[1] for e in entries_of([src(20, 10)], lists, S(8, 8, per_target=9, classes=[1, 0, 1]))[1]] == [1, 3]
    assert entries_of([src(20, 10)], lists, S(8, 8, per_target=9))[0][0] == 8
    # min_score is inclusive
    lists = [boxes_of([(1, 1, 2, 2, 0, 0.25), (1, 1, 2, 2, 0, np.float32(0.25) - np.float32(1e-7)), (1, 1, 2, 2, 0, 1.0)])]
    assert [e[1] for e in entries_of([src(20, 10)], lists, S(8, 8, per_target=9, min_score=0.25))[1]] == [0, 2]
    # order: targets ascending, list order inside; per_target cuts per target, capacity cuts the whole; a skipped source takes no part at all
    lists = [boxes_of([(1, 1, 2, 2)] * 3), boxes_of([(8, 2, 3, 5), (0, 0, 1, 1)]), boxes_of([(2, 2, 3, 3)] * 4)]
    stats = {}
    hdr, ent = entries_of([src(9, 9), None, src(9, 9)], lists, S(8, 8, per_target=2), capacity=3, stats=stats)
    assert hdr == (4, 3, 0, 3) and [e[:2] for e in ent] == [(0, 0), (0, 1), (2, 0)] and stats["cut_capacity"] == 1 and stats["cut_per_target"] == 3
    hdr, ent = cropref.select([src(9, 9), None, src(9, 9)], lists, S(8, 8, per_target=1), 5)
    assert hdr == (2, 2, 0, 5) and all(tuple(e) == (-1, 0, 0, 0.0, 0, 0, 0, 0, 0, 0, 1, 1) for e in ent[2:])
    raw = cropref.table_bytes(hdr, ent)
    assert len(raw) == 16 + 5 * 48 and list(raw[:16].view("<i4")) == [2, 2, 0, 5]
    # the entry's letterbox is net_input's
    hdr, ent = cropref.select([src(640, 424)], [boxes_of([(0, 0, 639, 423), (10, 10, 19, 409)])], S(320, 320, per_target=2), 2)
    assert [tuple(int(e[f]) for f in ("sw", "sh", "s1", "s2")) for e in ent] == [(320, 212, 640, 320), (8, 320, 400, 320)]


def test_cropref_map_back():
    dets = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", cropref.BOX_DTYPE, (128,))])
    hdr, ent = cropref.select([src(640, 424)], [boxes_of([(100, 50, 299, 149), (10, 10, 19, 409)])], cropref.Spec(320, 320, per_target=2), 3)
    recs = np.zeros(3, dets)
    for n in range(3):
        recs[n]["count"], recs[n]["nfull"], recs[n]["ncand"] = 2, 2, 7
        recs[n]["box"][:2] = boxes_of([(10, 20, 30, 40, 3, 0.75), (NAN, -BIG, BIG, 0.5)])
    out, _ = cropref.map_back(hdr, ent, recs)
    assert out[2].tobytes() == bytes(dets.itemsize)                                     # slot >= taken: a zero record
    b = out[0]["box"][0]                                                                # region 200 x 100 at (100, 50): s1 / s2 = 200 / 320
    assert (int(b["type"]), float(b["score"]), int(out[0]["ncand"])) == (3, 0.75, 7)
    assert [float(b[c]) for c in ("x1", "y1", "x2", "y2")] == [float(np.float32(v) * np.float32(200) / np.float32(320) + np.float32(o))
                                                               for v, o in ((10, 100), (20, 50), (30, 100), (40, 50))]
    b = out[1]["box"][1]
    assert np.isnan(b["x1"]) and b["y1"] == -np.inf or float(b["y1"]) < -1e29
    assert not out[0]["box"][2:].view(np.uint8).any()
    recs[0]["count"] = 1000                                                            # counts beyond their clamp
    assert cropref.map_back(hdr, ent, recs)[0][0]["count"] == 1000


def test_crop_without_device(capi):
    """with no HIP device every entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_crop_boxes_bgr_dev(None, None, 0, None, None, 1, None, None, None, 1, None),
                 lambda: L.ffgpu_crop_boxes_nv12_dev(None, None, 0, None, None, 1, None, None, None, 1, None),
                 lambda: L.ffgpu_exec_crop_bgr(None, 0, None, 1, None, None, None, 1, None),
                 lambda: L.ffgpu_exec_crop_nv12(None, 0, None, 1, None, None, None, 1, None),
                 lambda: L.ffgpu_crops_to_source_dev(None, 1, None, None, 0, None, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs
