"""Captions, without a GPU: the exported symbols, the layout of the item and spec structs in the ctypes mirror and the constants in the header, the
built-in font (pure host code) held to the properties include/ffcnn_hip.h states and pinned to a SHA-256, the host glue under ASan + UBSan
(san/text_driver.cc, run as a child process: every rejection with its message), tests/captions/textref.py (the numpy restatement of the contract the
GPU tests compare with) pinned to a literal per-pixel scalar loop and to the formatting cases, the seeded cases of the GPU fuzz held to the conditions
that keep it from passing vacuously, and the device entry points failing the way every entry point of the library does when no HIP device is visible.

A caption of the box composer is at most 16 + 1 + 4 + 1 + 12 = 34 characters (a 16-byte name, "100%"... "999%", "#2147483648?"), so the cut at
FFGPU_TEXT_MAX = 44 cannot be reached through it; the cut is checked where it can be: on textref.caption_text with a name table wider than the
ABI's, and on the rasteriser, where len above 44 reads as 44."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from captions import fuzzcases, textref

SYMBOLS = ["ffgpu_font_builtin", "ffgpu_draw_text_bgr_dev", "ffgpu_draw_text_nv12_dev", "ffgpu_caption_boxes_dev", "ffgpu_exec_caption_bgr",
           "ffgpu_exec_caption_nv12", "ffgpu_caption_scene_dev"]
NAN, INF = float("nan"), float("inf")
F32 = np.float32
ITEM = textref.ITEM_DTYPE
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
FONT_SHA256 = "b0c3d13512366859fb6965c0d5e8e872e8156ff963429796b0ea2ce693a243c3"


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_captions_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_captions_struct_layout(capi):
    T, P = capi.TextItem, capi.CaptionSpec
    assert (C.sizeof(T), C.sizeof(P)) == (64, 48)
    assert [getattr(T, f).offset for f in ("x", "y", "fg", "bg", "scale", "flags", "len", "reserved", "text")] == [0, 4, 8, 12, 16, 17, 18, 19, 20]
    assert [getattr(P, f).offset for f in ("min_score", "flags", "identity", "scale", "fg", "color", "palette", "npalette", "nnames", "d_names")] == \
        [0, 4, 8, 12, 16, 20, 24, 32, 36, 40]
    assert capi.TEXT_ITEM_DTYPE == ITEM and ITEM.itemsize == 64 and [ITEM.fields[f[0]][1] for f in T._fields_] == [getattr(T, f[0]).offset for f in T._fields_]
    assert (capi.TEXT_MAX, capi.TEXT_ITEMS, capi.TEXT_OPAQUE, capi.CAPTION_DETS) == (44, 256, 1, 128) == (textref.TEXT_MAX, textref.TEXT_ITEMS, textref.OPAQUE, textref.DETS)
    assert (capi.CAPTION_NAME, capi.CAPTION_SCORE, capi.CAPTION_ID, capi.CAPTION_OPAQUE) == (1, 2, 4, 8) == (textref.NAME, textref.SCORE, textref.ID, textref.CAPTION_OPAQUE)
    assert (capi.CAPTION_ENTRIES, capi.CAPTION_MERGED) == (0, 1) and (textref.NONE, textref.TYPE, textref.IDS) == (capi.ZONES_NONE, capi.ZONES_TYPE, capi.ZONES_IDS)
    sp = capi.caption_spec(name=True, score=False, ident=True, opaque=True, min_score=0.125, identity=capi.ZONES_TYPE, scale=3, fg=(1, 2, 3), color=(4, 5, 6),
                           palette=[(7, 8, 9), (10, 11, 12)], d_names=0x1000, nnames=5)
    assert (sp.min_score, sp.flags, sp.identity, sp.scale, list(sp.fg), list(sp.color), sp.npalette, sp.nnames, sp.d_names) == \
        (0.125, 13, 1, 3, [1, 2, 3, 0], [4, 5, 6, 0], 2, 5, 0x1000)
    assert bytes((C.c_ubyte * 8).from_address(sp.palette)) == bytes([7, 8, 9, 0, 10, 11, 12, 0])
    its = capi.text_items([(3, -4, "Ab"), (5, 6, b"\x00\xff~", (1, 2, 3), (4, 5, 6), 4, True)], 4)
    want = np.zeros(4, ITEM)
    want[0] = textref.make_item(3, -4, b"Ab", (255, 255, 255), (0, 0, 0), 1, False)
    want[1] = textref.make_item(5, 6, b"\x00\xff~", (1, 2, 3), (4, 5, 6), 4, True)
    assert its.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        capi.text_items([(0, 0, "x" * 45)])
    assert capi.names_bytes([b"", "p", b"fifteen-bytes-xx", b"sixteen bytes, ok!"]).tobytes() == fuzzcases.names_rows([b"", b"p", b"fifteen-bytes-xx", b"sixteen bytes, ok!"]).tobytes()


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    for phrase in ("} ffgpu_text_item;", "} ffgpu_caption_spec;", "64 bytes: x 0, y 4, fg 8, bg 12, scale 16, flags 17, len 18, text 20",
                   "48 bytes: min_score 0, flags 4, identity 8, scale 12, fg 16, color 20, palette 24, npalette 32, nnames 36,",
                   "Byte g * 8 + r is row r of glyph g", "bit 7 - c of that byte is column c", "0 <= px - x < 8 s n", "0 <= py - y < 8 s",
                   "text[(px - x) / (8 s)]", "((px - x) / s) % 8, row (py - y) / s", "a later item overwrites an earlier one",
                   "LAST item in slot order that writes any of the sample's up to four", "if at least one of the luma pixels the item writes in this sample is ink",
                   "The kernel is total over any item bytes", "y = b - 8 * scale when b >= 8 * scale", "p = (int)(score * 100.0f + 0.5f)", "clamped to 0..999",
                   "min(FFGPU_CAPTION_DETS, items_stride)", "every byte of d_items for the call's targets is written", "-v in decimal (taken in 64 bits) and ?",
                   "Redact, then draw, then caption", "Works on FFGPU_SPLIT2 executors", "THE VALUES ARE THE STATE'S WHEN THE KERNEL RUNS",
                   "every target of that stream shows the final totals", "tests/captions/textref.py", "Outlines of the zones' polygons and lines are not part of it"):
        assert phrase in hdr, phrase
    for name, val in (("FFGPU_TEXT_MAX", 44), ("FFGPU_TEXT_ITEMS", 256), ("FFGPU_TEXT_OPAQUE", 1), ("FFGPU_CAPTION_DETS", 128), ("FFGPU_CAPTION_NAME", 1),
                      ("FFGPU_CAPTION_SCORE", 2), ("FFGPU_CAPTION_ID", 4), ("FFGPU_CAPTION_OPAQUE", 8), ("FFGPU_CAPTION_ENTRIES", 0), ("FFGPU_CAPTION_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_text.inc"' in inc and inc.index('#include "ffgpu_zones.inc"') < inc.index('#include "ffgpu_text.inc"')
    host = open(os.path.join(CSRC, "ffgpu_text_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    kern = open(os.path.join(CSRC, "ffgpu_text.inc")).read()
    assert "atomic" not in kern.replace("no atomics", "") and "printf" not in kern


# ------------------------------------------------------------------------------------------------- the built-in font
def test_builtin_font_is_pure_host_code_and_keeps_its_properties(capi):
    f = capi.font_builtin()
    assert f.shape == (256, 8) and f.dtype == np.uint8
    ascii_ = f[32:127]
    assert not (ascii_ & 1).any() and not ascii_[:, 7].any()                            # column 7 and row 7 empty: adjacent cells do not touch
    empty = ~f.any(axis=1)
    assert empty[32] and empty.sum() == 1                                               # space, and nothing else
    assert len({g.tobytes() for g in ascii_}) == 95
    unknown = np.array([0xf8, 0x88, 0x88, 0x88, 0x88, 0x88, 0xf8, 0], np.uint8)        # a hollow box
    for g in list(range(32)) + list(range(127, 256)):
        assert f[g].tobytes() == unknown.tobytes(), g
    assert unknown.tobytes() not in {g.tobytes() for g in ascii_}
    assert hashlib.sha256(f.tobytes()).hexdigest() == FONT_SHA256
    guard = np.full(2048 + 16, 0xA5, np.uint8)                                          # exactly 2 048 bytes are written
    capi.lib().ffgpu_font_builtin(guard.ctypes.data + 8)
    assert guard[8:-8].tobytes() == f.tobytes() and (guard[:8] == 0xA5).all() and (guard[-8:] == 0xA5).all()
    inc = open(os.path.join(CSRC, "ffgpu_font8.inc")).read()
    assert inc.count("F8(") == 1 + 96 and "/* 'A' */ F8(01110, 10001, 10001, 10001, 11111, 10001, 10001)," in inc      # drawn in the repository, row by row


# ------------------------------------------------------------------------------------------------- textref against a literal scalar loop
def literal_pixel(it, font, px, py):
    """the contract's sentence for one pixel of one item: None (not written), else (is_ink, value bytes)"""
    s = min(max(int(it["scale"]), 1), 4)
    n = min(int(it["len"]), 44)
    dx, dy = px - int(it["x"]), py - int(it["y"])
    if not (0 <= dx < 8 * s * n and 0 <= dy < 8 * s):
        return None
    glyph = int(it["text"][dx // (8 * s)])
    ink = bool((int(font[glyph * 8 + dy // s]) >> (7 - (dx // s) % 8)) & 1)
    if ink:
        return True, [int(v) for v in it["fg"][:3]]
    if int(it["flags"]) & 1:
        return False, [int(v) for v in it["bg"][:3]]
    return None


def literal_bgr(buf, off, w, h, pitch, items, font):
    for it in items:
        for py in range(h):
            for px in range(w):
                hit = literal_pixel(it, font, px, py)
                if hit:
                    for c in range(3):
                        buf[off + py * pitch + 3 * px + c] = hit[1][c]


def literal_nv12(buf, y_off, uv_off, w, h, pitch_y, pitch_uv, items, font):
    for it in items:
        for sy in range((h + 1) // 2):
            for sx in range((w + 1) // 2):
                wrote, ink = False, False
                for py in (2 * sy, 2 * sy + 1):
                    for px in (2 * sx, 2 * sx + 1):
                        if px < w and py < h:
                            hit = literal_pixel(it, font, px, py)
                            if hit:
                                buf[y_off + py * pitch_y + px] = hit[1][0]
                                wrote, ink = True, ink or hit[0]
                if wrote:
                    src = it["fg"] if ink else it["bg"]
                    buf[uv_off + sy * pitch_uv + 2 * sx], buf[uv_off + sy * pitch_uv + 2 * sx + 1] = int(src[1]), int(src[2])


def test_textref_is_the_literal_loop():
    """seeded items, a random font, scales 1..4, overlap, clipping on all four sides, BGR with row padding, NV12 with odd w and h"""
    rng = np.random.default_rng(5750)
    sides = set()
    for case in range(10):
        w, h = int(rng.integers(9, 40)) | 1, int(rng.integers(7, 30)) | 1
        font = rng.integers(0, 256, 2048, dtype=np.uint8)
        items = np.array([fuzzcases.rand_item(rng, w, h) for _ in range(6)], ITEM)
        items[0]["scale"], items[1]["scale"], items[2]["scale"], items[3]["scale"] = 1, 2, 3, 4
        if case == 0:
            items[4]["len"], items[4]["scale"], items[5]["scale"] = 99, 0, 200         # read as 44 characters at scale 1, and as scale 4
        for it in items:
            s, n = textref.clamped(it)
            x, y = int(it["x"]), int(it["y"])
            sides |= {k for k, c in (("left", x < 0), ("top", y < 0), ("right", x + 8 * s * n > w), ("bottom", y + 8 * s > h)) if c}
        pitch = 3 * w + 5
        start = rng.integers(0, 256, 16 + pitch * h + 16, dtype=np.uint8)
        a, b = start.copy(), start.copy()
        textref.draw_bgr(a, 16, w, h, pitch, items, font)
        literal_bgr(b, 16, w, h, pitch, items, font)
        assert a.tobytes() == b.tobytes() and (a != start).any(), case
        pad = start.copy().reshape(-1)[16:16 + pitch * h].reshape(h, pitch)[:, 3 * w:]
        assert a[16:16 + pitch * h].reshape(h, pitch)[:, 3 * w:].tobytes() == pad.tobytes() and a[:16].tobytes() == start[:16].tobytes()
        pitch_y, pitch_uv = w + 3, w + 1 + 4
        uv_off = 16 + pitch_y * h + 16
        start = rng.integers(0, 256, uv_off + pitch_uv * ((h + 1) // 2) + 16, dtype=np.uint8)
        a, b = start.copy(), start.copy()
        textref.draw_nv12(a, 16, uv_off, w, h, pitch_y, pitch_uv, items, font)
        literal_nv12(b, 16, uv_off, w, h, pitch_y, pitch_uv, items, font)
        assert a.tobytes() == b.tobytes() and (a != start).any(), case
    assert sides == {"left", "top", "right", "bottom"}


def test_a_len_above_44_draws_44_characters_and_an_item_far_away_nothing():
    font = np.random.default_rng(5751).integers(1, 256, 2048, dtype=np.uint8)
    long_, cut = textref.make_item(0, 0, b"x" * 44, (9, 9, 9), (1, 1, 1), 1, True), None
    cut = long_.copy()
    long_["len"] = 255
    a, b = np.zeros(3 * 400 * 8, np.uint8), np.zeros(3 * 400 * 8, np.uint8)
    textref.draw_bgr(a, 0, 400, 8, 1200, [long_], font)
    textref.draw_bgr(b, 0, 400, 8, 1200, [cut], font)
    assert a.tobytes() == b.tobytes() and a.reshape(8, 400, 3)[:, :352].all() and not a.reshape(8, 400, 3)[:, 352:].any()
    for x, y in ((2 ** 31 - 1, 0), (-2 ** 31, 0), (0, 2 ** 31 - 1), (0, -2 ** 31), (-2 ** 31, -2 ** 31), (2 ** 31 - 1, 2 ** 31 - 1)):
        far = textref.make_item(x, y, b"x" * 44, (9, 9, 9), (1, 1, 1), 4, True)
        assert textref.masks(far, font, 400, 8) is None


# ------------------------------------------------------------------------------------------------- the formatting cases
NAMES = fuzzcases.names_rows([b"", b"p", b"fifteen-bytes-xx"[:15], b"sixteen bytes, ok"[:16]] + [b"n%d" % k for k in range(4, 80)])


def text_of(type_=2, score=0.5, v=0, flags=textref.NAME | textref.SCORE | textref.ID, identity=textref.IDS, names=NAMES):
    return textref.caption_text(type_, F32(score), v, textref.Spec(flags, identity=identity, names=names))


def test_formatting_cases():
    name_only = dict(flags=textref.NAME)
    assert [text_of(t, **name_only) for t in (0, 79, 80, -1, 2 ** 31 - 1, -2 ** 31)] == [b"", b"n79", b"80", b"-1", b"2147483647", b"-2147483648"]
    assert [text_of(t, **name_only) for t in (0, 1, 2, 3)] == [b"", b"p", b"fifteen-bytes-x", b"sixteen bytes, o"]       # 0, 1, 15 and 16 bytes without NUL
    assert [text_of(t, flags=textref.NAME, names=None) for t in (0, 3, -7)] == [b"0", b"3", b"-7"]
    assert text_of(0) == b"50%" and text_of(0, v=3) == b"50% #3"                        # an empty name is dropped with its space
    want_p = {0.0: 0, 0.004999: 0, 0.005: 1, 0.995: 100, 1.0: 100, 9.99: 999, 1e9: 999, INF: 999}
    for s, p in want_p.items():
        assert textref.score_percent(F32(s)) == p and text_of(score=s, flags=textref.SCORE) == b"%d%%" % p, s
    assert textref.score_percent(F32(-1.0)) == 0 and textref.score_percent(F32(0.125)) == 13 and textref.score_percent(F32(0.93)) == 93
    assert [text_of(v=v, flags=textref.ID) for v in (0, 1, -1, 2 ** 31 - 1, -2 ** 31)] == [b"", b"#1", b"#1?", b"#2147483647", b"#2147483648?"]
    # the longest caption the ABI can produce keeps under the cut; a wider name table shows the cut itself
    longest = text_of(3, 9.99, -2 ** 31)
    assert longest == b"sixteen bytes, o 999% #2147483648?" and len(longest) == 34 < textref.TEXT_MAX
    sp = textref.Spec(textref.NAME | textref.SCORE | textref.ID, identity=textref.IDS)
    sp.names = [b"a name of thirty-two bytes ......"[:32]]
    assert textref.caption_text(0, F32(1.0), -2 ** 31, sp) == b"a name of thirty-two bytes ..... 100% #21474" and len(textref.caption_text(0, F32(1.0), -2 ** 31, sp)) == 44


@pytest.mark.parametrize("identity", [textref.NONE, textref.TYPE, textref.IDS])
def test_every_part_combination_under_every_identity(identity):
    """the seven non-empty combinations of NAME, SCORE and ID: the text through caption_boxes (the id taken from where the identity says) against the
    parts spelled out here"""
    b = np.zeros(2, textref.BOX_DTYPE)
    b[0] = (5, 0.93, 20.9, 40.2, 60, 80)
    b[1] = (-3, 0.25, 20, 7.9, 60, 80)
    recs = np.zeros(1, textref.DETS_DTYPE)
    recs[0]["nfull"] = 2
    ids = np.zeros((1, 8 + 2), "<i4")
    ids[0, 8:] = (12, -4)
    for flags in range(1, 8):
        sp = textref.Spec(flags | textref.CAPTION_OPAQUE, identity=identity, scale=2, fg=(1, 2, 3), palette=[(10, 11, 12), (20, 21, 22), (30, 31, 32)], names=NAMES)
        got = textref.caption_boxes(recs, b, 2, None, sp, ids if identity == textref.IDS else None, 4)
        for k, (name, pct, v) in enumerate(((b"n5", b"93%", 12), (b"-3", b"25%", -4))):
            v = {textref.NONE: 0, textref.TYPE: int(b[k]["type"]), textref.IDS: v}[identity]
            parts = []
            if flags & 1 and identity != textref.TYPE:
                parts.append(name)
            if flags & 2:
                parts.append(pct)
            if flags & 4 and v:
                parts.append(b"#%d" % v if v > 0 else b"#%d?" % -v)
            it = got[0, k]
            assert bytes(it["text"][:int(it["len"])]) == b" ".join(parts) and not it["text"][int(it["len"]):].any(), (flags, k)
            assert (int(it["scale"]), int(it["flags"]), int(it["reserved"]), list(it["fg"])) == (2, 1, 0, [1, 2, 3, 0])
        assert (int(got[0, 0]["x"]), int(got[0, 0]["y"]), list(got[0, 0]["bg"])) == (20, 40 - 16, [30, 31, 32, 0])       # 5 mod 3; above the box
        assert (int(got[0, 1]["x"]), int(got[0, 1]["y"]), list(got[0, 1]["bg"])) == (20, 7, [10, 11, 12, 0])             # -3 mod 3 = 0; no room above: inside
        assert not got[0, 2:].view(np.uint8).any()


def test_considered_boxes_stop_at_the_smaller_of_128_and_items_stride_and_a_nan_score_never_counts():
    b = np.zeros(300, textref.BOX_DTYPE)
    b["score"], b["type"] = 0.5, np.arange(300)
    b["score"][[0, 5]] = (NAN, 0.1)
    recs = np.zeros(1, textref.DETS_DTYPE)
    recs[0]["nfull"] = 300
    sp = textref.Spec(textref.NAME, min_score=0.25)
    for stride, n in ((256, 128), (128, 128), (127, 127), (1, 1)):
        got = textref.caption_boxes(recs, b, 300, None, sp, None, stride)[0]
        want = [k for k in range(300) if k not in (0, 5)][:n]
        assert [int(bytes(it["text"][:int(it["len"])])) for it in got[:n]] == want and not got[n:].view(np.uint8).any()
    recs[0]["nfull"] = 4                                                               # the list's length is the record's, clamped to the stride
    assert (textref.caption_boxes(recs, b, 300, None, sp, None, 16)[0]["len"] > 0).sum() == 3
    recs[0]["nfull"] = -1
    assert not textref.caption_boxes(recs, b, 300, None, sp, None, 16).view(np.uint8).any()


# ------------------------------------------------------------------------------------------------- the GPU fuzz's seeds
def test_fuzz_seeds_meet_the_conditions_on_the_reference_alone(capi):
    """the seeded cases of the GPU fuzz (tests/captions/fuzzcases.py) through textref, no device -- a condition on the inputs: per surface format at
    least a quarter of the targets have two items that write a common pixel with different values, a quarter an item clipped by an edge, (NV12) a
    quarter a chroma sample whose luma pixels two different items write, and a sample whose deciding item writes only paper there; every scale and both
    OPAQUE settings occur; a target whose items all have len == 0 comes out unchanged; an item has len > 44 and one scale > 4 in its raw bytes"""
    tot = fuzzcases.check_text_stats(capi.font_builtin())
    print(tot)
    for nv12 in (False, True):
        cs = fuzzcases.text_cases(nv12)
        assert sorted(cs) == sorted(fuzzcases.TEXT_NAMES)
        assert {c.stride for c in cs.values()} >= {3, 7, 64, 256} and max(c.n for c in cs.values()) > 64
        assert any(t is None for c in cs.values() for t in c.targets) and any(c.font is None for c in cs.values()) and any(c.font is not None for c in cs.values())
        assert any(int(it["x"]) in (-2 ** 31, 2 ** 31 - 1) for it in cs["hostile"].items.reshape(-1))
        for c in cs.values():
            assert (c.want(capi.font_builtin()) != c.start).any(), c.what
    odd = [g for c in fuzzcases.text_cases(True).values() for g in c.targets if g is not None]
    assert any(g["w"] % 2 and g["h"] % 2 for g in odd) and any(g["w"] % 2 == 0 for g in odd)
    print(fuzzcases.check_box_stats())
    bs = fuzzcases.box_cases()
    assert sorted(bs) == sorted(fuzzcases.BOX_NAMES) and {c.spec.identity for c in bs.values()} == {textref.NONE, textref.TYPE, textref.IDS}
    assert any(c.flat is None for c in bs.values()) and any(c.first is not None for c in bs.values()) and max(c.n for c in bs.values()) > 128
    assert [int(r["nfull"]) for r in bs["lists"].recs] == [0, 1, 127, 128, 129, 255, 256, 257, 6]
    assert any(np.isnan(c.flat["score"]).any() for c in bs.values() if c.flat is not None)
    ss = fuzzcases.scene_cases()
    assert sorted(ss) == sorted(fuzzcases.SCENE_NAMES) and max(c.n for c in ss.values()) > 512 and {c.items_stride for c in ss.values()} >= {16, 256}
    assert any(-1 in c.streams for c in ss.values())
    for c in ss.values():
        used = c.want_items["len"] > 0
        assert used[:, :8].any() and used[:, 8:16].any() and not used[:, 16:].any() and not used[:, :16].all(), c.what
    assert {int(s["nzones"]) for c in ss.values() for s in c.scenes} >= {0, 8, 11} and {int(z["nverts"]) for c in ss.values() for s in c.scenes for z in s["zone"]} >= {2, 3, 8, 9}
    texts = {bytes(it["text"][:int(it["len"])]) for c in ss.values() for it in c.want_items.reshape(-1)}
    assert any(t.endswith(b" 4294967295") for t in texts) and any(b"/4294967295" in t for t in texts) and any(t.startswith(b"Z7 ") for t in texts)


# ------------------------------------------------------------------------------------------------- without a device; the host glue
def test_captions_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_draw_text_bgr_dev(None, 1, None, None, 1, None),
                 lambda: L.ffgpu_draw_text_nv12_dev(None, 1, None, None, 1, None),
                 lambda: L.ffgpu_caption_boxes_dev(None, None, 0, None, 1, None, None, None, 1, None),
                 lambda: L.ffgpu_caption_scene_dev(None, None, 1, 1, None, 64, None, 1, None, None, 16, None),
                 lambda: L.ffgpu_exec_caption_bgr(None, 0, None, 1, None, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_caption_nv12(None, 0, None, 1, None, None, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


def test_host_glue_under_the_sanitizers():
    """san/text_driver.cc: the built-in font's table, the caption spec's plan and every argument check of ffgpu_text_host.hpp on the CPU under
    ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "text"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_text_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"text_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 80, out[-1]
    assert not any("WRONG" in ln for ln in out)
    for ln in ("font.margins_empty holds", "font.space_is_the_only_empty_glyph holds", "font.ascii_pairwise_different holds", "font.other_codes_are_the_unknown_glyph holds",
               "boxes.null_spec -1 op: NULL spec", "boxes.null_items -1 op: NULL items", "boxes.stride_0 -1 op: items_stride 0 is outside 1..256",
               "boxes.stride_257 -1 op: items_stride 257 is outside 1..256", "boxes.min_score_nan -1 op: min_score nan is not in [0, 1]",
               "boxes.min_score_high -1 op: min_score 1.5 is not in [0, 1]", "boxes.flags_no_part -1 op: flags 0x8 name no part (FFGPU_CAPTION_NAME | _SCORE | _ID)",
               "boxes.flags_16 -1 op: unknown flags 0x11", "boxes.identity_3 -1 op: identity 3 is none of FFGPU_ZONES_NONE, _TYPE, _IDS",
               "boxes.scale_0 -1 op: scale 0 is outside 1..4", "boxes.scale_5 -1 op: scale 5 is outside 1..4",
               "boxes.npalette_without_palette -1 op: npalette 3 (0 with a NULL palette, else 1..256)", "boxes.nnames_neg -1 op: nnames -1 (0 with NULL names, else >= 1)",
               "boxes.nnames_without_names -1 op: nnames 80 (0 with NULL names, else >= 1)", "boxes.ids_missing -1 op: NULL ids with identity FFGPU_ZONES_IDS",
               "boxes.ids_unwanted_type -1 op: ids given without identity FFGPU_ZONES_IDS", "scene.stride_15 -1 op: items_stride 15 is outside 16..256",
               "scene.events_stride_63 -1 op: events_stride 63 is below FFGPU_ZONES_ROW = 64", "scene.stream_high -1 op: target 1: stream 2 is outside -1 .. 1",
               "scene.spec_parts_ignored 0 ", "text.null_targets -1 op: NULL targets", "text.ntargets_0 -1 op: 0 targets (ntargets >= 1)"):
        assert ln in out, ln
