"""Preview surfaces, without a GPU: the six exported symbols, the layout of the two structs in the ctypes mirror and the constants in the header, the
phrases of the contract, ffgpu_preview_rect and ffgpu_preview_grid against tests/preview/previewref.py over a table of geometries, the host glue under
ASan + UBSan (san/preview_driver.cc, run as a child process: every rejection with its message), previewref (the numpy restatement of the contract the
GPU tests compare with) pinned to a deliberately naive second implementation -- Python loops per destination sample over the fine grid of sw ow
units --, the four properties of the rule by name, the seeded cases of the GPU fuzz held to the conditions that keep it from passing vacuously, and
the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from preview import fuzzcases, previewref

SYMBOLS = ["ffgpu_preview_spec_check", "ffgpu_preview_rect", "ffgpu_preview_grid", "ffgpu_preview_tile", "ffgpu_preview_bgr_dev", "ffgpu_preview_nv12_dev"]
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module", autouse=True)
def feature(capi):
    """every test of this file is a test of the feature, those that pin previewref and the fuzz's seeds too: a reference is worth what the library it
    restates carries, so each of them needs the built library to export the family"""
    missing = [s for s in SYMBOLS if s not in getattr(capi, "EXPORTS", ()) or not hasattr(capi.lib(), s)]
    assert not missing, "libffcnn_hip.so lacks %s" % missing


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_preview_symbols_exported(capi):
    assert len(SYMBOLS) == 6
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_preview_struct_layout(capi):
    P, S = capi.PreviewPane, capi.PreviewSpec
    assert C.sizeof(P) == 32 and C.sizeof(S) == 16
    assert [getattr(P, f).offset for f in ("sx", "sy", "sw", "sh", "dx", "dy", "dw", "dh")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [getattr(S, f).offset for f in ("fit", "flags", "fill", "reserved")] == [0, 4, 8, 12]
    assert (capi.PREVIEW_STRETCH, capi.PREVIEW_FIT, capi.PREVIEW_KEEP_BARS, capi.PREVIEW_MAX_SIDE, capi.PREVIEW_MAX_PANES) == (0, 1, 1, 8192, 4096) == \
        (previewref.STRETCH, previewref.FIT, previewref.KEEP_BARS, previewref.MAX_SIDE, previewref.MAX_PANES)
    p = capi.preview_pane((1, 2, 3, 4), (5, 6, 7, 8))
    assert (p.sx, p.sy, p.sw, p.sh, p.dx, p.dy, p.dw, p.dh) == (1, 2, 3, 4, 5, 6, 7, 8)
    assert bytes(capi.preview_pane()) == bytes(32)
    sp = capi.preview_spec(capi.PREVIEW_FIT, (9, 8, 7), keep_bars=True)
    assert (sp.fit, sp.flags, list(sp.fill), sp.reserved) == (1, 1, [9, 8, 7, 0], 0)
    capi.preview_spec_check(sp)
    for field, v, msg in (("fit", 2, "fit 2 is neither"), ("flags", 2, "unknown flags 0x2"), ("reserved", 1, "reserved must be 0")):
        bad = capi.preview_spec()
        setattr(bad, field, v)
        with pytest.raises(Exception, match=re.escape(msg)):
            capi.preview_spec_check(bad)
    bad = capi.preview_spec()
    bad.fill[3] = 1
    with pytest.raises(Exception, match=re.escape("fill[3] must be 0")):
        capi.preview_spec_check(bad)
    assert capi.preview_tile()[:2] == (fuzzcases.TILE_W, fuzzcases.TILE_H) and 1 <= capi.preview_tile()[2] < 130


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    text = re.sub(r"\s*\n \*\s*", " ", hdr)                                             # (a phrase may run over a line of the comment)
    for phrase in ("} ffgpu_preview_pane;", "} ffgpu_preview_spec;", "tests/preview/previewref.py", "32 bytes: sx 0, sy 4, sw 8, sh 12, dx 16, dy 20, dw 24, dh 28",
                   "16 bytes: fit 0, flags 4, fill 8, reserved 12", "out = { sx, sy, sw, sh, X0, Y0, ow, oh }", "NV12 requires sx, sy, dx and dy even",
                   "if sw dh >= sh dw then ow = dw and oh = clamp((2 sh dw + sw) / (2 sw), 1, dh)", "ow = clamp((2 sw dh + sh) / (2 sh), 1, dw)",
                   "ox = (dw - ow) >> 1, oy = (dh - oh) >> 1, for NV12 both rounded down to even", "The IMAGE is the ow x oh rectangle at (X0, Y0); the BARS are the rest of the pane",
                   "one rule for every ratio, down or up", "Destination sample (i, j) covers [i sw, (i + 1) sw) horizontally, in units of 1 / ow source samples",
                   "source sample x covers [x ow, (x + 1) ow)", "wx(i, x) is the length of their intersection",
                   "out(i, j) = (sum_y wy(j, y) * sum_x wx(i, x) * v(x, y) + (D >> 1)) / D, rounded down", "the division is exact, not a float reciprocal",
                   "ow == sw and oh == sh gives a byte copy", "integer ratios k x l give the rounded mean of each k x l block", "a constant plane stays constant",
                   "mirroring the source mirrors the image", "the three channels are resampled independently",
                   "the source region is ((sw + 1) / 2) x ((sh + 1) / 2) at (sx / 2, sy / 2)", "the destination region ((ow + 1) / 2) x ((oh + 1) / 2) at (X0 / 2, Y0 / 2)",
                   "destination chroma sample (i, j) is written by the pane whose rectangle holds luma pixel (2 i, 2 j)", "as image when that pixel lies in the IMAGE, as bar otherwise",
                   "`matrix` of the frames is not read", "With FFGPU_PREVIEW_KEEP_BARS they are not written", "is skipped; its sizes are not looked at",
                   "The gaps of a wall are the caller's memset", "dx = gap + col (cw + gap), dy = gap + row (ch + gap)", "HOST arrays, free again on return",
                   "is the only writer of those bytes", "stream order is the only barrier", "There is no executor form",
                   "two panes with the same destination pixel address whose rectangles intersect (both indices)", "draw with a thickness near the ratio before scaling"):
        assert phrase in text, phrase
    assert hdr.index("---- motion maps:") < hdr.index("---- preview surfaces:")
    for name, val in (("FFGPU_PREVIEW_STRETCH", 0), ("FFGPU_PREVIEW_FIT", 1), ("FFGPU_PREVIEW_KEEP_BARS", 1), ("FFGPU_PREVIEW_MAX_SIDE", 8192), ("FFGPU_PREVIEW_MAX_PANES", 4096)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert inc.index('#include "ffgpu_motion.inc"') < inc.index('#include "ffgpu_preview.inc"')
    host = open(os.path.join(CSRC, "ffgpu_preview_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    assert int(re.search(r"#define PREVIEW_TW\s+(\d+)", host).group(1)) == fuzzcases.TILE_W and int(re.search(r"#define PREVIEW_TH\s+(\d+)", host).group(1)) == fuzzcases.TILE_H
    kern = open(os.path.join(CSRC, "ffgpu_preview.inc")).read()
    assert "atomic" not in kern.replace("No atomics", "") and "printf" not in kern and "asm" not in kern and "__threadfence" not in kern
    assert kern.count("__global__") == 1 and "template <int CH>\n__global__" in kern    # one kernel template
    assert "static_assert(sizeof(PreviewArgs)" in kern and "4096 - 256" in kern
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("ffgpu_motion_host.hpp ffgpu_preview_host.hpp") == 2 and "san/preview_driver.cc" in mk


# ------------------------------------------------------------------------------------------------- the host functions against previewref
GEOMETRIES = [  # (src_w, src_h, dst_w, dst_h, pane)
    (1, 1, 1, 1, (0,) * 8), (8192, 8192, 8192, 8192, (0,) * 8), (8192, 1, 1, 8192, (0,) * 8), (1, 8192, 8192, 1, (0,) * 8), (9000, 9000, 9000, 9000, (8, 8, 8192, 8192, 808, 808, 8192, 8192)),
    (100, 60, 50, 40, (0,) * 8), (60, 100, 50, 40, (0,) * 8), (100, 60, 50, 40, (3, 5, 10, 50, 1, 1, 40, 30)), (100, 60, 50, 40, (2, 4, 10, 50, 0, 2, 40, 30)),
    (200, 1, 8, 8, (0,) * 8), (1, 200, 8, 8, (0,) * 8), (200, 2, 9, 9, (0, 0, 200, 1, 0, 0, 9, 9)), (100, 60, 50, 36, (0,) * 8), (60, 100, 38, 50, (0,) * 8),
    (640, 424, 1920, 1080, (160, 52, 320, 320, 480, 270, 480, 270)), (1920, 1080, 480, 270, (0,) * 8), (7, 5, 3, 2, (0,) * 8), (5, 3, 17, 11, (0,) * 8),
    (64, 48, 97, 61, (0, 0, 0, 0, 2, 2, 45, 17)), (64, 48, 97, 61, (1, 0, 5, 5, 0, 0, 0, 0)), (64, 48, 97, 61, (0, 0, 0, 0, 0, 3, 11, 11)),
    (64, 48, 97, 61, (0, 0, 10, 0, 0, 0, 0, 0)), (64, 48, 97, 61, (0, 0, 0, 0, 0, 0, 0, 9)), (64, 48, 97, 61, (1, 0, 0, 0, 0, 0, 0, 0)), (64, 48, 97, 61, (0, 0, 0, 0, 0, 2, 0, 0)),
    (64, 48, 97, 61, (60, 0, 5, 5, 0, 0, 0, 0)), (64, 48, 97, 61, (0, 0, 0, 0, 90, 0, 8, 8)), (64, 48, 97, 61, (0, -2, 5, 5, 0, 0, 0, 0)), (9000, 10, 50, 40, (0,) * 8),
    (64, 48, 9000, 61, (0,) * 8), (2 ** 31 - 1, 2 ** 31 - 1, 10, 10, (2 ** 31 - 2, 2 ** 31 - 2, 1, 1, 0, 0, 0, 0)), (64, 48, 97, 61, (2 ** 31 - 1, 0, 5, 5, 0, 0, 0, 0))]


@pytest.mark.parametrize("nv12", [False, True])
def test_preview_rect_equals_previewref(capi, nv12):
    seen = {"ok": 0, "reject": 0, "fit_w": 0, "fit_h": 0, "clamp": 0, "even": 0}
    for fit in (previewref.STRETCH, previewref.FIT):
        for g in GEOMETRIES:
            pane = capi.preview_pane(g[4][:4], g[4][4:])
            try:
                want = previewref.resolve(g[0], g[1], g[2], g[3], g[4], fit, nv12)
            except previewref.Reject:
                want = None
            if want is None:
                with pytest.raises(Exception, match="pane 0"):
                    capi.preview_rect(g[0], g[1], g[2], g[3], pane, capi.preview_spec(fit), nv12)
                seen["reject"] += 1
                continue
            assert capi.preview_rect(g[0], g[1], g[2], g[3], pane, capi.preview_spec(fit), nv12) == want, (g, fit)
            seen["ok"] += 1
            dw, dh = (g[4][6], g[4][7]) if g[4][6] else (g[2], g[3])
            sx, sy, sw, sh, X0, Y0, ow, oh = want
            if fit:
                seen["fit_w"] += ow < dw
                seen["fit_h"] += oh < dh
                seen["clamp"] += (oh == 1 and 2 * sh * dw + sw < 2 * sw) or (ow == 1 and 2 * sw * dh + sh < 2 * sh)
                seen["even"] += nv12 and (((dw - ow) >> 1) & 1 or ((dh - oh) >> 1) & 1)
    assert seen["ok"] >= 20 and seen["reject"] >= 10 and seen["fit_w"] >= 2 and seen["fit_h"] >= 2 and seen["clamp"] >= 2 and (not nv12 or seen["even"] >= 1), seen


def test_preview_grid_equals_previewref(capi):
    ok = bad = 0
    for nv12 in (False, True):
        for args in ((6, 2, 97, 61, 2), (5, 3, 97, 61, 2), (16, 4, 1920, 1080, 0), (64, 8, 1920, 1080, 4), (1, 1, 1, 1, 0), (7, 7, 50, 9, 1), (130, 13, 78, 40, 0),
                     (0, 1, 10, 10, 0), (4, 0, 10, 10, 0), (4, 5, 10, 10, 0), (4, 2, 10, 10, -1), (4, 2, 10, 10, 4), (4, 2, 3, 10, 0), (4, 2, 10, 10, 2 ** 31 - 1), (3, 1, 8192, 5, 0)):
            try:
                want = previewref.grid(*args, nv12=nv12)
            except previewref.Reject:
                with pytest.raises(Exception, match="preview_grid"):
                    capi.preview_grid(*args, nv12=nv12)
                bad += 1
                continue
            got = capi.preview_grid(*args, nv12=nv12)
            assert [(p.dx, p.dy, p.dw, p.dh) for p in got] == want and all((p.sx, p.sy, p.sw, p.sh) == (0, 0, 0, 0) for p in got), args
            ok += 1
    assert ok >= 12 and bad >= 12
    assert [(p.dx, p.dy, p.dw, p.dh) for p in capi.preview_grid(6, 2, 97, 61, 2)][5] == (49, 40, 45, 17)


def test_host_glue_under_the_sanitizers():
    """san/preview_driver.cc: the spec, resolve, the grid and every argument check of ffgpu_preview_host.hpp on the CPU under ASan + UBSan, as a child
    process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "preview"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_preview_san")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"preview_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) >= len(out) - 1 >= 100, out[-1]
    text = "\n".join(out)
    for msg in ("NULL srcs", "NULL dsts", "NULL panes", "NULL spec", "0 panes (1..4096)", "4097 panes (1..4096)", "fit 3 is neither FFGPU_PREVIEW_STRETCH nor FFGPU_PREVIEW_FIT",
                "unknown flags 0x4", "unknown flags 0x80000000", "fill[3] must be 0", "spec: reserved must be 0", "source 1: bad size 0 x 48", "destination 3: bad size 40 x -1",
                "source 0: reserved must be 0", "destination 1: reserved must be 0", "source 0: pitch 100 is below 3 w = 192", "destination 0: pitch 100 is below 3 w = 120",
                "source 0: pitch_y 10 is below w = 64", "is odd (U V pairs are read", "is odd (U V pairs are written", "destination 1: matrix 4",
                "pane 1: a source region of 31 x 0 (both 0 for the whole frame, or neither)", "pane 3: a pane of 0 x 14 (both 0 for the whole surface, or neither)",
                "the whole frame as the source region wants sx = sy = 0, not (1, 0)", "the whole surface as the pane wants dx = dy = 0, not (0, 2)",
                "pane 1: the source region 31 x 17 at (40, 4) is outside the frame of 65 x 48", "pane 3: the pane 18 x 14 at (20, 18) is outside the surface of 40 x 30",
                "pane 0: a pane of 8193 x 14 (1..8192 each)", "a source region of 8193 x 10 (1..8192 each)", "pane 1: NV12 wants even sx, sy, dx, dy, not (3, 4) and (20, 0)",
                "pane 3: NV12 wants even sx, sy, dx, dy, not (0, 0) and (20, 17)", "pane 1: the source and the destination are the same pixels",
                "panes 0 and 3 overlap in one destination surface", "4 panes in 5 columns", "gap 1 (from 0, even for NV12)", "leave no room in 10 x 10"):
        assert msg in text, msg


def test_preview_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_preview_bgr_dev(None, None, None, 1, None, None), lambda: L.ffgpu_preview_nv12_dev(None, None, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


# ------------------------------------------------------------------------------------------------- previewref against a naive second implementation
def naive_resample(plane, ow, oh):
    """lists of lists, one channel: destination sample i is the sum of the sw fine units u in [i sw, (i + 1) sw) of a row stretched to sw ow units, unit
    u lying in source sample u // ow; likewise down the columns; then the rounded division"""
    sh, sw = len(plane), len(plane[0])
    rows = [[sum(row[u // ow] for u in range(i * sw, (i + 1) * sw)) for i in range(ow)] for row in plane]
    D = sw * sh
    return [[(sum(rows[u // oh][i] for u in range(j * sh, (j + 1) * sh)) + D // 2) // D for i in range(ow)] for j in range(oh)]


def test_previewref_equals_the_naive_one():
    rng = np.random.default_rng(9200)
    shapes = [(1, 1, 1, 1), (7, 5, 3, 2), (5, 3, 17, 11), (40, 40, 40, 40), (40, 38, 20, 19), (39, 1, 1, 40), (1, 40, 40, 1), (40, 40, 1, 1), (2, 3, 40, 39)]
    while len(shapes) < 40:
        shapes.append(tuple(int(v) for v in rng.integers(1, 41, 4)))
    for sw, sh, ow, oh in shapes:
        ch = int(rng.integers(1, 4))
        v = rng.integers(0, 256, (sh, sw, ch), dtype=np.uint8)
        if rng.random() < 0.3:
            v |= 0xf8                                                                 # bright: the rounding near 255
        got = previewref.resample(v if ch > 1 else v[:, :, 0], ow, oh).reshape(oh, ow, ch)
        for c in range(ch):
            assert got[:, :, c].tolist() == naive_resample(v[:, :, c].tolist(), ow, oh), (sw, sh, ow, oh, c)
        assert previewref.weights(sw, ow).sum(axis=1).tolist() == [sw] * ow


# ------------------------------------------------------------------------------------------------- the four properties of the rule
def test_equal_sizes_give_a_byte_copy():
    v = np.random.default_rng(9201).integers(0, 256, (13, 29, 3), dtype=np.uint8)
    assert previewref.resample(v, 29, 13).tobytes() == v.tobytes()


def test_integer_ratios_give_the_rounded_block_mean():
    v = np.random.default_rng(9202).integers(0, 256, (12, 35), dtype=np.uint8)
    k, l = 5, 3                                                                        # 35 x 12 -> 7 x 4
    blocks = v.reshape(4, l, 7, k).astype(np.int64).sum(axis=(1, 3))
    assert previewref.resample(v, 7, 4).tolist() == ((blocks + (k * l) // 2) // (k * l)).tolist()


def test_a_constant_plane_stays_constant():
    for val in (0, 1, 127, 254, 255):
        for sw, sh, ow, oh in ((7, 5, 3, 2), (5, 3, 17, 11), (8192, 3, 5, 7), (31, 33, 32, 30)):
            assert (previewref.resample(np.full((sh, sw), val, np.uint8), ow, oh) == val).all(), (val, sw, sh, ow, oh)


def test_mirroring_the_source_mirrors_the_image():
    v = np.random.default_rng(9203).integers(0, 256, (23, 31, 3), dtype=np.uint8)
    for ow, oh in ((7, 9), (40, 50), (31, 5)):
        out = previewref.resample(v, ow, oh)
        assert previewref.resample(v[:, ::-1], ow, oh).tobytes() == np.ascontiguousarray(out[:, ::-1]).tobytes()
        assert previewref.resample(v[::-1], ow, oh).tobytes() == np.ascontiguousarray(out[::-1]).tobytes()


# ------------------------------------------------------------------------------------------------- the fuzz is not vacuous
@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_cases_are_not_vacuous(capi, fmt):
    cases = fuzzcases.cases(fmt)
    assert tuple(cases) == fuzzcases.NAMES
    TW, TH, njobs = capi.preview_tile()
    seen = dict(down_x=0, up_x=0, frac_x=0, down_y=0, up_y=0, frac_y=0, big=0, bars_lr=0, bars_tb=0, kept=0, odd_sx=0, padded=0, odd_wh=0, skipped=0)
    for name, c in cases.items():
        assert c.want.tobytes() != c.start.tobytes(), name
        live = c.live()
        seen["skipped"] += c.n - len(live)
        for p in live:
            (sx, sy, sw, sh, X0, Y0, ow, oh), (dx, dy, dw, dh) = c.resolved(p)
            seen["down_x"] += sw > ow; seen["up_x"] += sw < ow; seen["frac_x"] += sw % ow != 0 and ow % sw != 0
            seen["down_y"] += sh > oh; seen["up_y"] += sh < oh; seen["frac_y"] += sh % oh != 0 and oh % sh != 0
            seen["big"] += ow >= 2 * TW + 1 and oh >= 2 * TH + 1
            seen["bars_lr"] += X0 > dx and X0 + ow < dx + dw
            seen["bars_tb"] += Y0 > dy and Y0 + oh < dy + dh
            seen["odd_sx"] += sx & 1
            s = c.srcs[p]
            seen["padded"] += (s[3] > 3 * s[1]) if fmt == "bgr" else (s[4] > s[2])
            seen["odd_wh"] += fmt == "nv12" and c.size(s)[0] & 1 and c.size(s)[1] & 1
            # at least one image byte differs from what the surface held and from the fill
            img, img0 = c.luma_view(c.want, p, (X0, Y0, ow, oh)), c.luma_view(c.start, p, (X0, Y0, ow, oh))
            fill = np.tile(np.asarray(c.fill if fmt == "bgr" else c.fill[:1], np.uint8), ow)[None, :]
            assert ((img != img0) & (img != fill)).any(), (name, p)
            if c.keep and (ow < dw or oh < dh):
                pane, pfill = c.luma_view(c.want, p, (dx, dy, dw, dh)).copy(), np.tile(np.asarray(c.fill if fmt == "bgr" else c.fill[:1], np.uint8), dw)[None, :]
                assert pane.tobytes() != c.luma_view(c.start, p, (dx, dy, dw, dh)).tobytes()
                k = 3 if fmt == "bgr" else 1
                pane[Y0 - dy:Y0 - dy + oh, k * (X0 - dx):k * (X0 - dx + ow)] = pfill[:, :k * ow]
                seen["kept"] += bool((pane != pfill).any())
    assert all(v >= 1 for k, v in seen.items() if k not in ("odd_sx", "odd_wh")), seen
    assert seen["odd_sx"] >= 1 if fmt == "bgr" else seen["odd_wh"] >= 1, seen
    # the wall: four or more panes on one surface, and a byte between them that stays
    w = cases["wall"]
    assert len(w.live()) >= 4 and len({d[0] for d in w.dsts if d is not None}) == 1 and None in w.srcs
    dw_, dh_ = w.size(w.surfaces[0])
    covered = np.zeros((dh_, dw_), bool)
    for k in range(w.n):
        dx, dy, dw, dh = w.panes[k][4:]
        covered[dy:dy + dh, dx:dx + dw] = True
    gap = ~covered
    assert gap[2:-2, 2:-2].any()                                                       # a gap byte between panes, not only the surface's rim
    ch = 3 if fmt == "bgr" else 1
    surf = (w.surfaces[0][0], w.surfaces[0][3] if fmt == "bgr" else w.surfaces[0][4])
    got, was = (previewref.view(b, surf[0], dh_, ch * dw_, surf[1]).reshape(dh_, dw_, ch) for b in (w.want, w.start))
    assert (got[gap] == was[gap]).all() and (got[covered] != was[covered]).any()
    assert fuzzcases.cases(fmt)["launch table"].n == 130 > 4 * njobs and njobs not in (1, 64, 67, 130)
    assert cases["seam 67x35 to 16x9"].dsts[0][0] & 1 and cases["fit clamp"].resolved(0)[0][7] == 1
    assert cases["64x64 copy"].trace["bar_bytes"] == 0 and cases["fit wide in tall"].trace["bar_bytes"] > 0


def test_the_wide_sum_needs_64_bits():
    """the lazily built NV12 case: 255 D passes 2^32 on the Y plane, the U V plane stays below; a 32-bit outer sum gives other bytes"""
    c = fuzzcases.wide_sum()
    (sx, sy, sw, sh, X0, Y0, ow, oh), _ = c.resolved(0)
    assert (sw, sh, ow, oh) == (8192, 2064, 3, 2) and 255 * sw * sh >= 2 ** 32 > 255 * ((sw + 1) // 2) * ((sh + 1) // 2)
    oy, _, w, h, py, _ = c.frames[0]
    y = previewref.view(c.start, oy, h, w, py)
    assert int(y.min()) >= 250
    # by cumulative sums in int64: every destination sample covers whole source samples here but for the two seams in x
    img = c.luma_view(c.want, 0, (X0, Y0, ow, oh))
    assert int(img.min()) >= 250
    cols = y.astype(np.int64).sum(axis=0)                                              # the sum of a column over all rows
    half = y[:1032].astype(np.int64).sum(axis=0)
    wx = previewref.weights(8192, 3)
    D = sw * sh
    top = (wx @ half) * 2                                                              # wy == oh == 2 on every row of the upper half: sh / oh = 1032 whole rows
    assert img[0].tolist() == ((top + D // 2) // D).tolist() and img[1].tolist() == (((wx @ (cols - half)) * 2 + D // 2) // D).tolist()
    assert int(top.max()) >= 2 ** 32 and (((top & 0xffffffff) + D // 2) // D).tolist() != img[0].tolist()
