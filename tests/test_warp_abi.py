"""Warp surfaces, without a GPU: the nine exported symbols, the layout of the three structs in the ctypes mirror and the constants in the header, the
sentences of the contract, ffgpu_warp_mesh_size and ffgpu_warp_mesh_orient against tests/warp/warpref.py EXACTLY, the homography and lens builders
within one unit, ffgpu_warp_point on meshes of extreme values, the host glue under ASan + UBSan (san/warp_driver.cc, run as a child process: every
rejection with its message), warpref (the numpy restatement of the contract the GPU tests compare with) pinned to a deliberately naive second
implementation -- Python loops per destination pixel with Python integers --, the five properties of the rule by name, the seeded cases of the GPU
fuzz held to the conditions that keep it from passing vacuously, and the device entry points failing the way every entry point of the library does
when no HIP device is visible."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from warp import fuzzcases, warpref

SYMBOLS = ["ffgpu_warp_spec_check", "ffgpu_warp_mesh_size", "ffgpu_warp_mesh_orient", "ffgpu_warp_mesh_homography", "ffgpu_warp_mesh_lens", "ffgpu_warp_point",
           "ffgpu_warp_tile", "ffgpu_warp_bgr_dev", "ffgpu_warp_nv12_dev"]
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
IMIN, IMAX = warpref.INT_MIN, warpref.INT_MAX


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module", autouse=True)
def feature(capi):
    """every test of this file is a test of the feature, those that pin warpref and the fuzz's seeds too: a reference is worth what the library it
    restates carries, so each of them needs the built library to export the family"""
    missing = [s for s in SYMBOLS if s not in getattr(capi, "EXPORTS", ()) or not hasattr(capi.lib(), s)]
    assert not missing, "libffcnn_hip.so lacks %s" % missing


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_warp_symbols_exported(capi):
    assert len(SYMBOLS) == 9
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_warp_struct_layout(capi):
    M, S, L = capi.WarpMesh, capi.WarpSpec, capi.WarpLens
    assert (C.sizeof(M), C.sizeof(S), C.sizeof(L)) == (24, 16, 120)
    assert [getattr(M, f).offset for f in ("xy", "mw", "mh", "cell", "reserved")] == [0, 8, 12, 16, 20]
    assert [getattr(S, f).offset for f in ("filter", "border", "fill", "reserved")] == [0, 4, 8, 12]
    assert [getattr(L, f).offset for f in ("model", "reserved", "dst", "src", "k", "p")] == [0, 4, 8, 40, 72, 104]
    assert (capi.WARP_MESH_ONE, capi.WARP_SUB, capi.WARP_BILINEAR, capi.WARP_NEAREST, capi.WARP_FILL, capi.WARP_CLAMP, capi.WARP_MAX_SIDE, capi.WARP_MAX_JOBS,
            capi.WARP_LENS_BROWN, capi.WARP_LENS_EQUIDISTANT) == (256, 32, 0, 1, 0, 1, 8192, 4096, 0, 1) == \
        (warpref.MESH_ONE, warpref.SUB, warpref.BILINEAR, warpref.NEAREST, warpref.FILL, warpref.CLAMP, warpref.MAX_SIDE, warpref.MAX_JOBS, warpref.LENS_BROWN, warpref.LENS_EQUIDISTANT)
    m = capi.warp_mesh(0x1000, 70, 40, 16)
    assert (m.xy, m.mw, m.mh, m.cell, m.reserved) == (0x1000, 6, 4, 16, 0)
    sp = capi.warp_spec(capi.WARP_NEAREST, capi.WARP_CLAMP, (9, 8, 7))
    assert (sp.filter, sp.border, list(sp.fill), sp.reserved) == (1, 1, [9, 8, 7, 0], 0)
    capi.warp_spec_check(sp)
    for field, v, msg in (("filter", 2, "filter 2 is neither"), ("border", -1, "border -1 is neither"), ("reserved", 1, "reserved must be 0")):
        bad = capi.warp_spec()
        setattr(bad, field, v)
        with pytest.raises(Exception, match=re.escape(msg)):
            capi.warp_spec_check(bad)
    bad = capi.warp_spec()
    bad.fill[3] = 1
    with pytest.raises(Exception, match=re.escape("fill[3] must be 0")):
        capi.warp_spec_check(bad)
    ln = capi.warp_lens(capi.WARP_LENS_EQUIDISTANT, (1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12), (13, 14))
    assert (ln.model, ln.reserved, list(ln.dst), list(ln.src), list(ln.k), list(ln.p)) == (1, 0, [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14])
    assert capi.warp_tile()[:3] == (fuzzcases.TILE_W, fuzzcases.TILE_H, warpref.LDS_BYTES) == (warpref.TILE_W, warpref.TILE_H, 16384) and 1 <= capi.warp_tile()[3] < 130


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    text = re.sub(r"\s*\n \*\s*", " ", hdr)                                             # (a phrase may run over a line of the comment)
    for phrase in ("} ffgpu_warp_mesh;", "} ffgpu_warp_spec;", "} ffgpu_warp_lens;", "tests/warp/warpref.py", "24 bytes: xy 0, mw 8, mh 12, cell 16, reserved 20",
                   "16 bytes: filter 0, border 4, fill 8, reserved 12", "120 bytes: model 0, reserved 4, dst 8, src 40, k 72, p 104",
                   "mw = (dw - 1) / c + 2 by mh = (dh - 1) / c + 2 points", "c one of 8, 16, 32, 64", "in units of 1 / 256 source pixel (FFGPU_WARP_MESH_ONE)",
                   "an integer position is the centre of that source pixel", "8-byte aligned, rows of mw pairs",
                   "Any int32 value is legal: the kernel never reads a byte outside the source frame, whatever the mesh holds",
                   "ci = i >> s, a = i & (c - 1), cj = j >> s, b = j & (c - 1)", "(ci, cj), (ci + 1, cj), (ci, cj + 1), (ci + 1, cj + 1)",
                   "S  = (c - b) * ((c - a) * P00 + a * P10) + b * ((c - a) * P01 + a * P11)", "X8 = (S + (1 << (2 s - 1))) >> (2 s)", "(the shift is arithmetic)",
                   "x5 = (X8 + 4) >> 3", "Neighbouring cells share points, so the map is continuous", "x0 = x5 >> 5, fx = x5 & 31",
                   "the taps are (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)",
                   "out = ((32 - fy) * ((32 - fx) * v00 + fx * v10) + fy * ((32 - fx) * v01 + fx * v11) + 512) >> 10", "the one tap ((x5 + 16) >> 5, (y5 + 16) >> 5)",
                   "a tap outside the source frame has the fill colour's channel as its value", "a pixel whose taps are all outside is the fill",
                   "each tap coordinate is clamped to 0 .. sw - 1 and 0 .. sh - 1", "the three channels share the position",
                   "Destination chroma sample (i, j) takes the mesh at luma pixel (2 i, 2 j)", "xc5 = (X8 + 8) >> 4", "((sw + 1) / 2) x ((sh + 1) / 2) under the same filter and border",
                   "The fill is Y U V", "`matrix` of the frames is not read", "chroma is treated as co-sited", "the identity mesh is a byte copy",
                   "the eight orientations permute bytes exactly", "an integer translation shifts the frame and fills", "a constant plane stays constant under CLAMP",
                   "NEAREST writes only source bytes or the fill", "The operator does no area averaging", "scale down with the preview operator afterwards",
                   "Untouched: row padding, memory round the destination, every source byte, the mesh", "Doubles are evaluated in the order written, without contraction",
                   "floor(v * 256 + 0.5) saturated to int32", "a non-finite value or a non-positive perspective denominator gives INT32_MIN",
                   "0: (i, j)   1: (j, H - 1 - i)   2: (W - 1 - i, H - 1 - j)   3: (W - 1 - j, i)", "4: (W - 1 - i, j)   5: (W - 1 - j, H - 1 - i)   6: (i, H - 1 - j)   7: (j, i)",
                   "xy may be NULL to ask for the sizes only", "x = ((h0 i + h1 j) + h2) / ((h6 i + h7 j) + h8)", "y = ((h3 i + h4 j) + h5) / ((h6 i + h7 j) + h8)",
                   "An affine map is h6 = h7 = 0, h8 = 1", "xn = (i - dst_cx) / dst_fx,  yn = (j - dst_cy) / dst_fy,  r2 = xn xn + yn yn", "rad = 1 + ((k3 r2 + k2) r2 + k1) r2",
                   "xd = xn rad + ((2 p1) (xn yn) + p2 (r2 + (2 xn) xn))", "yd = yn rad + (p1 (r2 + (2 yn) yn) + (2 p2) (xn yn))", "r = sqrt(r2),  theta = atan(r),  t2 = theta theta",
                   "theta_d = theta (1 + ((((k4 t2 + k3) t2 + k2) t2 + k1) t2))", "scale = theta_d / r, or 1 where r is 0", "x = src_fx xd + src_cx, y = src_fy yd + src_cy",
                   "out = { X8, Y8 }", "HOST arrays, free again on return", "into the WHOLE of dsts[n]", "a pane of a larger surface is a frame descriptor into it",
                   "is the only writer of those bytes", "inside the bounding box of the mesh points of the cells the tile touches, plus one pixel",
                   "where that box, clipped to the frame, fits the LDS budget", "The choice is uniform per workgroup and both forms give the same bytes",
                   "the bytes of LDS the staged form may fill", "stream order is the only barrier", "There is no executor form", "its sizes and its mesh are not looked at",
                   "a NULL, misaligned or wrongly sized mesh, or a bad cell", "two jobs with the same destination pixel address (both indices)"):
        assert phrase in text, phrase
    assert hdr.index("---- preview surfaces:") < hdr.index("---- warp surfaces:")
    for name, val in (("FFGPU_WARP_MESH_ONE", 256), ("FFGPU_WARP_SUB", 32), ("FFGPU_WARP_BILINEAR", 0), ("FFGPU_WARP_NEAREST", 1), ("FFGPU_WARP_FILL", 0), ("FFGPU_WARP_CLAMP", 1),
                      ("FFGPU_WARP_MAX_SIDE", 8192), ("FFGPU_WARP_MAX_JOBS", 4096), ("FFGPU_WARP_LENS_BROWN", 0), ("FFGPU_WARP_LENS_EQUIDISTANT", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert inc.index('#include "ffgpu_preview.inc"') < inc.index('#include "ffgpu_warp.inc"')
    host = open(os.path.join(CSRC, "ffgpu_warp_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    assert int(re.search(r"#define WARP_TW\s+(\d+)", host).group(1)) == fuzzcases.TILE_W and int(re.search(r"#define WARP_TH\s+(\d+)", host).group(1)) == fuzzcases.TILE_H
    kern = open(os.path.join(CSRC, "ffgpu_warp.inc")).read()
    assert "atomic" not in kern.replace("No atomics", "") and "printf" not in kern and "asm" not in kern and "__threadfence" not in kern and "float" not in kern
    assert kern.count("__global__") == 1 and "template <int CH>\n__global__" in kern    # one kernel template
    assert "static_assert(sizeof(WarpArgs)" in kern and "4096 - 256" in kern
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("ffgpu_preview_host.hpp ffgpu_warp_host.hpp") == 2 and "san/warp_driver.cc" in mk


# ------------------------------------------------------------------------------------------------- the exact builders against warpref
SIDES = [(1, 1), (8192, 8192), (8192, 1), (1, 8192), (37, 23), (64, 16), (65, 17), (8, 8), (9, 9), (1920, 1080)]


def test_mesh_size_equals_warpref(capi):
    ok = bad = 0
    for dw, dh in SIDES + [(0, 5), (5, 0), (8193, 5), (5, 8193), (-1, -1), (2 ** 31 - 1, 5)]:
        for cell in warpref.CELLS + (0, 4, 7, 12, 128, -8):
            try:
                want = warpref.mesh_size(dw, dh, cell)
            except warpref.Reject:
                with pytest.raises(Exception, match="warp_mesh_size"):
                    capi.warp_mesh_size(dw, dh, cell)
                bad += 1
                continue
            assert capi.warp_mesh_size(dw, dh, cell) == want, (dw, dh, cell)
            ok += 1
    assert ok == 40 and bad >= 60
    assert capi.warp_mesh_size(1, 1, 8) == (2, 2) and capi.warp_mesh_size(8192, 8192, 8) == (1025, 1025) and capi.warp_mesh_size(65, 17, 64) == (3, 2)


def test_mesh_orient_equals_warpref_exactly(capi):
    n = 0
    for sw, sh in SIDES:
        for orient in range(8):
            for cell in warpref.CELLS:
                if max(sw, sh) == 8192 and cell < 64 and orient not in (1, 6):
                    continue                                                            # (the million-point meshes: two orientations of them)
                wh, xy = capi.warp_mesh_orient(sw, sh, orient, cell)
                want_wh, want = warpref.mesh_orient(sw, sh, orient, cell)
                assert wh == want_wh and xy.shape == want.shape and xy.tobytes() == want.tobytes(), (sw, sh, orient, cell)
                n += 1
    assert n >= 200
    for args in ((37, 23, 8, 8), (37, 23, -1, 8), (0, 23, 0, 8), (37, 8193, 0, 8), (37, 23, 0, 9)):
        with pytest.raises(Exception, match="warp_mesh_orient"):
            capi.warp_mesh_orient(*args)
        with pytest.raises(warpref.Reject):
            warpref.mesh_orient(*args)


def orient_matrix(sw, sh, orient):
    """the orientations written as homographies"""
    W1, H1 = sw - 1, sh - 1
    return ((1, 0, 0, 0, 1, 0), (0, 1, 0, -1, 0, H1), (-1, 0, W1, 0, -1, H1), (0, -1, W1, 1, 0, 0), (-1, 0, W1, 0, 1, 0), (0, -1, W1, -1, 0, H1), (1, 0, 0, 0, -1, H1),
            (0, 1, 0, 1, 0, 0))[orient] + (0, 0, 1)


def test_mesh_homography(capi):
    """exact where the coefficients are integers; otherwise every point within 1 unit of warpref (an ulp of a double below 2^23 cannot move the rounding
    of v * 256 by more)"""
    for sw, sh in ((37, 23), (1, 1), (8192, 8192), (640, 424)):
        for orient in range(8):
            cell = warpref.CELLS[orient & 3] if sw < 8192 else 64
            (dw, dh), want = warpref.mesh_orient(sw, sh, orient, cell)
            got = capi.warp_mesh_homography(dw, dh, cell, orient_matrix(sw, sh, orient))
            assert got.tobytes() == want.tobytes() == warpref.mesh_homography(dw, dh, cell, orient_matrix(sw, sh, orient)).tobytes(), (sw, sh, orient)
    for h in ((1, 0, -17, 0, 1, 40, 0, 0, 1), (1, 0, 0, 0, 1, 0, 0, 0, 4), (-1, 0, 99, 0, 1, 0, 0, 0, 1), (2, 0, 0.5, 0, 2, 0.5, 0, 0, 1)):
        assert capi.warp_mesh_homography(100, 60, 16, h).tobytes() == warpref.mesh_homography(100, 60, 16, h).tobytes(), h
    rng = np.random.default_rng(9500)
    worst = 0
    hs = [fuzzcases.ROT30, (600 / 64, 0, 0, 0, 200 / 16, 0, 0, 0, 1), (1.1, 0.02, -3.3, 0.01, 0.9, 7.7, 1e-4, -2e-4, 1.0), (1, 0, 0, 0, 1, 0, -1 / 64, 0, 1), (1e300, 0, 1e9, 0, -1e300, -1e9, 0, 0, 1),
          (float("nan"), 0, 0, 0, float("inf"), 0, 0, 0, 1), (1, 0, 0, 0, 1, 0, 0, 0, float("nan")), (1, 0, 0, 0, 1, 0, 0, 0, 0)]
    hs += [tuple(rng.normal(0, 1, 6)) + (rng.normal(0, 1e-3), rng.normal(0, 1e-3), 1.0) for _ in range(12)]
    for h in hs:
        for dw, dh, cell in ((48, 48, 16), (1920, 1080, 32), (7, 5, 8)):
            got, want = capi.warp_mesh_homography(dw, dh, cell, h), warpref.mesh_homography(dw, dh, cell, h)
            d = np.abs(got.astype(np.int64) - want.astype(np.int64))
            assert d.max() <= 1, (h, dw, dh, int(d.max()))
            assert ((got == IMIN) == (want == IMIN)).all() or d.max() <= 1
            worst = max(worst, int(d.max()))
    assert (capi.warp_mesh_homography(48, 48, 16, (1, 0, 0, 0, 1, 0, -1 / 16, 0, 1))[:, 1:] == IMIN).all()       # the denominator 1 - i / 16 is 0 from the second column on
    for args, msg in (((48, 48, 5, hs[0]), "cell 5"), ((0, 48, 8, hs[0]), "a destination of 0 x 48")):
        with pytest.raises(Exception, match=msg):
            capi.warp_mesh_homography(*args)


def test_mesh_lens(capi):
    """every point within 1 unit of warpref: the operations are the same IEEE doubles in the same order but atan, which may differ by an ulp between
    libm and numpy; one ulp of a double below 2^23 cannot move floor(v * 256 + 0.5) by more than 1.  Derived, not measured."""
    K = dict(fuzzcases.LENS)
    lenses = [K, dict(K, model=warpref.LENS_EQUIDISTANT, k=(-0.01, 0.002, -0.0003, 0.00004)), dict(K, model=warpref.LENS_EQUIDISTANT, k=(0, 0, 0, 0), dst=(30.0, 31.0, 10.0, 60.0)),
              dict(model=warpref.LENS_BROWN, dst=(1000.0, 1000.0, 959.5, 539.5), src=(1000.0, 1000.0, 959.5, 539.5), k=(-0.3, 0, 0, 0), p=(0, 0)),
              dict(model=warpref.LENS_BROWN, dst=(1.0, 1.0, 0.0, 0.0), src=(1e9, -1e9, 0.0, 0.0), k=(1e300, 1e300, 1e300, 0), p=(0, 0)),
              dict(model=warpref.LENS_EQUIDISTANT, dst=(1e-300, 1.0, 0.0, 0.0), src=(1.0, 1.0, 0.0, 0.0), k=(0, 0, 0, 0), p=(0, 0))]
    for ln in lenses:
        for dw, dh, cell in ((96, 64, 32), (1920, 1080, 16), (7, 5, 8), (1, 1, 64)):
            got = capi.warp_mesh_lens(dw, dh, cell, capi.warp_lens(ln["model"], ln["dst"], ln["src"], ln["k"], ln["p"]))
            want = warpref.mesh_lens(dw, dh, cell, **ln)
            assert got.shape == want.shape and np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1, (ln, dw, dh)
    # no distortion and equal cameras: the identity
    same = capi.warp_mesh_lens(96, 64, 8, capi.warp_lens(capi.WARP_LENS_BROWN, (64.0, 64.0, 32.0, 16.0), (64.0, 64.0, 32.0, 16.0)))
    assert same.tobytes() == warpref.mesh_orient(96, 64, 0, 8)[1].tobytes()
    for ln, msg in ((capi.warp_lens(2, (1, 1, 0, 0), (1, 1, 0, 0)), "model 2 is neither"), (capi.warp_lens(0, (0, 1, 0, 0), (1, 1, 0, 0)), "finite and above 0"),
                    (capi.warp_lens(0, (1, float("inf"), 0, 0), (1, 1, 0, 0)), "finite and above 0"), (None, "NULL lens")):
        with pytest.raises(Exception, match=msg):
            capi.warp_mesh_lens(96, 64, 8, ln)


def test_warp_point_equals_warpref(capi):
    """the interpolation rule on host meshes holding INT32_MIN and INT32_MAX, every pixel of the destination"""
    rng = np.random.default_rng(9501)
    for dw, dh, cell in ((20, 12, 8), (33, 17, 16), (65, 66, 64), (1, 1, 32)):
        mw, mh = warpref.mesh_size(dw, dh, cell)
        for kind in range(4):
            xy = rng.integers(-2 ** 31, 2 ** 31, (mh, mw, 2)).astype(np.int32)
            if kind < 3:
                xy[rng.random(xy.shape) < 0.4] = IMIN
                xy[rng.random(xy.shape) < 0.4] = IMAX
            if kind == 1:
                xy[...] = IMAX
            if kind == 2:
                xy[...] = IMIN
            X8, Y8 = warpref.points(xy, cell, dw, dh)
            assert X8.min() >= IMIN and X8.max() <= IMAX
            for j in range(dh):
                for i in range(0, dw, 1 if dw < 40 else 3):
                    assert capi.warp_point(xy, cell, dw, dh, i, j) == (int(X8[j, i]), int(Y8[j, i])), (dw, dh, cell, kind, i, j)
    xy = warpref.mesh_orient(20, 12, 0, 8)[1]
    for args, msg in (((xy, 8, 20, 12, 20, 0), "pixel (20, 0) is outside"), ((xy, 8, 20, 12, 0, -1), "pixel (0, -1) is outside"), ((xy, 16, 20, 12, 0, 0), "4 x 3 points, a destination of 20 x 12 with cells of 16 has 3 x 2"),
                      ((xy, 8, 28, 12, 0, 0), "4 x 3 points, a destination of 28 x 12 with cells of 8 has 5 x 3")):
        with pytest.raises(Exception, match=re.escape(msg)):
            capi.warp_point(*args)


def test_host_glue_under_the_sanitizers():
    """san/warp_driver.cc: the spec, the builders into buffers of exactly the mesh's size, the interpolation rule and every argument check of
    ffgpu_warp_host.hpp on the CPU under ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child:
    the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "warp"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_warp_san")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"warp_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) >= len(out) - 1 >= 150, out[-1]
    text = "\n".join(out)
    for msg in ("NULL srcs", "NULL dsts", "NULL meshes", "NULL spec", "0 jobs (1..4096)", "4097 jobs (1..4096)", "filter 3 is neither FFGPU_WARP_BILINEAR nor FFGPU_WARP_NEAREST",
                "border 4 is neither FFGPU_WARP_FILL nor FFGPU_WARP_CLAMP", "fill[3] must be 0", "spec: reserved must be 0", "source 1: bad size 0 x 48",
                "destination 3: bad size 40 x -1", "source 0: reserved must be 0", "destination 1: reserved must be 0", "source 0: pitch 100 is below 3 w = 192",
                "destination 0: pitch 100 is below 3 w = 120", "source 0: pitch_y 10 is below w = 64", "is odd (U V pairs are read", "is odd (U V pairs are written",
                "destination 1: matrix 4", "job 0: a source of 8193 x 48 (1..8192 each)", "job 3: a destination of 40 x 8193 (1..8192 each)", "job 1: mesh: NULL xy",
                "job 3: mesh: xy 0x20300c is not 8-byte aligned", "job 0: mesh: 6 x 6 points, a destination of 40 x 30 with cells of 8 has 6 x 5",
                "job 0: mesh: cell 12 is none of 8, 16, 32, 64", "job 1: mesh: reserved must be 0", "job 1: the source and the destination are the same pixels",
                "jobs 0 and 3 have the same destination", "orient 8 (0..7)", "model 2 is neither FFGPU_WARP_LENS_BROWN nor FFGPU_WARP_LENS_EQUIDISTANT",
                "must be finite and above 0", "pixel (20, 0) is outside the destination of 20 x 12", "NULL h", "NULL lens", "NULL out_dst_wh"):
        assert msg in text, msg


def test_warp_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_warp_bgr_dev(None, None, None, 1, None, None), lambda: L.ffgpu_warp_nv12_dev(None, None, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


# ------------------------------------------------------------------------------------------------- warpref against a naive second implementation
def naive_warp(plane, xy, cell, dw, dh, filt, border, fill, chroma=False):
    """lists of lists of channel lists, Python integers, one destination sample at a time: the header's sentences in their order"""
    s = {8: 3, 16: 4, 32: 5, 64: 6}[cell]
    sh, sw, nch = len(plane), len(plane[0]), len(plane[0][0])
    c = cell

    def tap(x, y, ch):
        if border == warpref.CLAMP:
            x, y = min(max(x, 0), sw - 1), min(max(y, 0), sh - 1)
        return plane[y][x][ch] if 0 <= x < sw and 0 <= y < sh else fill[ch]

    out = []
    for jj in range((dh + 1) // 2 if chroma else dh):
        row = []
        for ii in range((dw + 1) // 2 if chroma else dw):
            i, j = (2 * ii, 2 * jj) if chroma else (ii, jj)
            ci, a, cj, b = i >> s, i & (c - 1), j >> s, j & (c - 1)
            pos = []
            for k in (0, 1):
                P00, P10, P01, P11 = (int(xy[cj][ci][k]), int(xy[cj][ci + 1][k]), int(xy[cj + 1][ci][k]), int(xy[cj + 1][ci + 1][k]))
                S = (c - b) * ((c - a) * P00 + a * P10) + b * ((c - a) * P01 + a * P11)
                X8 = (S + (1 << (2 * s - 1))) >> (2 * s)
                pos.append((X8 + 8) >> 4 if chroma else (X8 + 4) >> 3)
            x5, y5 = pos
            if filt == warpref.NEAREST:
                row.append([tap((x5 + 16) >> 5, (y5 + 16) >> 5, ch) for ch in range(nch)])
                continue
            x0, fx, y0, fy = x5 >> 5, x5 & 31, y5 >> 5, y5 & 31
            row.append([((32 - fy) * ((32 - fx) * tap(x0, y0, ch) + fx * tap(x0 + 1, y0, ch)) + fy * ((32 - fx) * tap(x0, y0 + 1, ch) + fx * tap(x0 + 1, y0 + 1, ch)) + 512) >> 10
                        for ch in range(nch)])
        out.append(row)
    return out


def test_warpref_equals_the_naive_one():
    rng = np.random.default_rng(9502)
    n = 0
    for trial in range(36):
        sw, sh, dw, dh = (int(v) for v in rng.integers(1, 41, 4))
        cell = warpref.CELLS[trial % 4]
        filt, border = (trial >> 2) & 1, (trial >> 3) & 1
        xy = (fuzzcases.extreme_mesh if trial % 9 == 8 else fuzzcases.random_mesh)(rng, sw, sh, dw, dh, cell)[0]
        fill = [int(v) for v in rng.integers(0, 256, 3)]
        bgr = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        assert warpref.warp_plane(bgr, xy, cell, dw, dh, filt, border, fill).tolist() == naive_warp(bgr.tolist(), xy.tolist(), cell, dw, dh, filt, border, fill), trial
        y = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        assert warpref.warp_plane(y, xy, cell, dw, dh, filt, border, fill)[:, :, None].tolist() == naive_warp(y[:, :, None].tolist(), xy.tolist(), cell, dw, dh, filt, border, fill), trial
        uv = rng.integers(0, 256, ((sh + 1) // 2, (sw + 1) // 2, 2), dtype=np.uint8)
        got = warpref.warp_chroma(uv, xy, cell, dw, dh, filt, border, fill[1:])
        assert got.shape == ((dh + 1) // 2, (dw + 1) // 2, 2) and got.tolist() == naive_warp(uv.tolist(), xy.tolist(), cell, dw, dh, filt, border, fill[1:], chroma=True), trial
        n += 1
    assert n == 36


# ------------------------------------------------------------------------------------------------- the five properties of the rule
FILTERS = ((warpref.BILINEAR, warpref.FILL), (warpref.BILINEAR, warpref.CLAMP), (warpref.NEAREST, warpref.FILL), (warpref.NEAREST, warpref.CLAMP))


def test_the_identity_mesh_is_a_byte_copy():
    rng = np.random.default_rng(9503)
    for w, h, cell in ((1, 1, 8), (29, 13, 8), (65, 17, 64), (37, 23, 16)):
        v = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        uv = rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8)
        xy = warpref.mesh_orient(w, h, 0, cell)[1]
        for filt, border in FILTERS:
            assert warpref.warp_plane(v, xy, cell, w, h, filt, border, (1, 2, 3)).tobytes() == v.tobytes()
            assert warpref.warp_chroma(uv, xy, cell, w, h, filt, border, (2, 3)).tobytes() == uv.tobytes()


def test_the_eight_orientations_permute_bytes_exactly():
    rng = np.random.default_rng(9504)
    v = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    by_numpy = [v, np.rot90(v, -1), np.rot90(v, 2), np.rot90(v, 1), v[:, ::-1], np.rot90(v[:, ::-1], -1), v[::-1], v.transpose(1, 0, 2)]
    for orient in range(8):
        (dw, dh), xy = warpref.mesh_orient(37, 23, orient, 16)
        for filt, border in FILTERS:
            out = warpref.warp_plane(v, xy, 16, dw, dh, filt, border, (1, 2, 3))
            assert out.tobytes() == np.ascontiguousarray(by_numpy[orient]).tobytes(), (orient, filt, border)
            # orient k followed by its inverse restores the bytes
            (bw, bh), back = warpref.mesh_orient(dw, dh, warpref.INVERSE[orient], 8)
            assert (bw, bh) == (37, 23) and warpref.warp_plane(out, back, 8, bw, bh, filt, border, (1, 2, 3)).tobytes() == v.tobytes()


def test_an_integer_translation_shifts_the_frame_and_fills():
    v = np.random.default_rng(9505).integers(0, 256, (20, 30, 3), dtype=np.uint8)
    for tx, ty in ((3, 0), (-4, 5), (0, -7), (31, 2)):
        xy = warpref.mesh_homography(30, 20, 8, (1, 0, tx, 0, 1, ty, 0, 0, 1))
        want = np.empty_like(v)
        want[...] = np.array((9, 8, 7), np.uint8)
        for j in range(20):
            for i in range(30):
                if 0 <= i + tx < 30 and 0 <= j + ty < 20:
                    want[j, i] = v[j + ty, i + tx]
        for filt in (warpref.BILINEAR, warpref.NEAREST):
            assert warpref.warp_plane(v, xy, 8, 30, 20, filt, warpref.FILL, (9, 8, 7)).tobytes() == want.tobytes(), (tx, ty, filt)


def test_a_constant_plane_stays_constant_under_clamp():
    rng = np.random.default_rng(9506)
    for val in (0, 1, 127, 254, 255):
        xy, cell = fuzzcases.extreme_mesh(rng, 30, 20, 40, 24, 8)
        for filt in (warpref.BILINEAR, warpref.NEAREST):
            assert (warpref.warp_plane(np.full((20, 30), val, np.uint8), xy, cell, 40, 24, filt, warpref.CLAMP, (77, 0, 0)) == val).all(), (val, filt)


def test_nearest_writes_only_source_bytes_or_the_fill():
    rng = np.random.default_rng(9507)
    v = (rng.integers(0, 64, (20, 30), dtype=np.uint8) * 4).astype(np.uint8)          # multiples of 4; the fill is not one
    xy, cell = fuzzcases.random_mesh(rng, 30, 20, 40, 24, 16)
    out = warpref.warp_plane(v, xy, cell, 40, 24, warpref.NEAREST, warpref.FILL, (201, 0, 0))
    assert set(np.unique(out).tolist()) <= set(np.unique(v).tolist()) | {201} and (out == 201).any() and (out != 201).any()
    assert (warpref.warp_plane(v, xy, cell, 40, 24, warpref.BILINEAR, warpref.FILL, (201, 0, 0)) % 4 != 0).any()      # (the bilinear filter does blend)


# ------------------------------------------------------------------------------------------------- the fuzz is not vacuous
@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_cases_are_not_vacuous(capi, fmt):
    cases = fuzzcases.cases(fmt)
    assert tuple(cases) == fuzzcases.NAMES
    TW, TH, budget, njobs = capi.warp_tile()
    seen = dict(skipped=0, padded=0, odd_addr=0, odd_wh=0, cells=set(), panes=0)
    for name, c in cases.items():
        assert c.want.tobytes() != c.start.tobytes(), name
        live = c.live()
        seen["skipped"] += c.n - len(live)
        for k in live:
            s, d = c.srcs[k], c.dsts[k]
            (sw, sh), (dw, dh) = c.size(s), c.size(d)
            seen["padded"] += (d[3] > 3 * dw) if fmt == "bgr" else (d[4] > dw)
            seen["odd_addr"] += d[0] & 1
            seen["odd_wh"] += dw & 1 and dh & 1
            seen["cells"].add(c.meshes[k][1])
            assert c.luma_view(c.want, k).tobytes() != c.luma_view(c.start, k).tobytes(), (name, k)
            assert c.meshes[k][0].shape == warpref.mesh_size(dw, dh, c.meshes[k][1])[::-1] + (2,)
    assert seen["skipped"] >= 1 and seen["padded"] >= 4 and seen["odd_addr"] >= 4 and seen["odd_wh"] >= 4 and seen["cells"] == set(warpref.CELLS), seen
    # the random meshes: a tenth of the pixels with every tap inside the frame, a tenth with a tap outside, half with both fractions non-zero
    for name in fuzzcases.RANDOM + fuzzcases.WIDE:
        inside, outside, frac = cases[name].tap_stats(0)
        assert inside >= 0.1 and outside >= 0.1 and frac >= 0.5, (name, inside, outside, frac)
    assert {(cases[n].filt, cases[n].border) for n in fuzzcases.RANDOM} == set(FILTERS) == {(cases[n].filt, cases[n].border) for n in fuzzcases.WIDE}
    # the two forms of the read (BGR planes have both; the planes of NV12 frames are always read directly): every tile of the random cases is staged and
    # most tiles of the wide ones direct -- so each filter and border runs on each path; the budget case has a tile within 64 bytes of the budget (it
    # fills it) and one a row over it; the minifying mesh's footprint is far over any budget
    if fmt == "bgr":
        paths = {name: [v <= budget for k in c.live() for plane in c.lds_bytes(k) for v in plane] for name, c in cases.items()}
        assert all(all(paths[n]) for n in fuzzcases.RANDOM) and not any(paths["minify 600x200 to 64x16"])
        for n in fuzzcases.WIDE:                                                            # (a narrow tile at the right edge touches few cells: it may still fit)
            for plane in cases[n].lds_bytes(0):
                assert 2 * sum(v > budget for v in plane) > len(plane), (n, plane)
        b = cases["budget"]
        assert b.lds_bytes(0)[0] == [budget] and budget - 64 <= b.lds_bytes(0)[0][0] <= budget < b.lds_bytes(1)[0][0] <= budget + 512
        assert min(v for plane in cases["minify 600x200 to 64x16"].lds_bytes(0) for v in plane) > 3 * budget
        assert sum(all(p) for p in paths.values()) >= 8 and sum(not all(p) for p in paths.values()) >= 6          # (the four wide cases, the minifying mesh, the budget)
    else:
        assert all(c.lds_bytes(k) == [] for c in cases.values() for k in c.live())
    for k in cases["cells"].live():
        inside, outside, frac = cases["cells"].tap_stats(k)
        assert inside >= 0.1 and outside >= 0.1 and frac >= 0.5, ("cells", k)
    # FILL and CLAMP differ where a tap is outside, the two filters where a fraction is not zero
    r = cases["random fill bilinear"]
    for filt, border in FILTERS[1:]:
        other = warpref.warp(r.start.copy(), fmt, r.srcs, r.dsts, r.meshes, filt, border, r.fill)
        assert (other != r.want).sum() > 100, (filt, border)
    # the identities are copies, the orientations permutations, the extreme meshes hold the extreme values and mostly fill
    for name in ("identity 64x16", "identity 65x17"):
        c = cases[name]
        s, d = c.srcs[0], c.dsts[0]
        w, h = c.size(s)
        ch, sp = (3, s[3]) if fmt == "bgr" else (1, s[4])
        assert c.luma_view(c.want, 0).tobytes() == warpref.view(c.start, s[0], h, ch * w, sp).tobytes()
    assert cases["identity 64x16"].size(cases["identity 64x16"].dsts[0]) == (TW, TH) and cases["identity 65x17"].size(cases["identity 65x17"].dsts[0]) == (TW + 1, TH + 1)
    o = cases["orientations 37x23"]
    assert o.n == 8 and [o.size(d) for d in o.dsts] == [(37, 23), (23, 37)] * 4
    src = warpref.view(o.start, o.srcs[0][0], 23, (3 if fmt == "bgr" else 1) * 37, o.srcs[0][3] if fmt == "bgr" else o.srcs[0][4])
    for k in range(8):
        assert sorted(o.luma_view(o.want, k).reshape(-1).tolist()) == sorted(src.reshape(-1).tolist()), k
    e = cases["extreme"]
    assert all((m[0] == IMIN).any() and (m[0] == IMAX).any() for m in e.meshes) and e.tap_stats(0)[1] > 0.5 and e.tap_stats(0)[0] > 0
    # the half-pixel translation blends, the minifying mesh strides over the source, the lens bends
    assert all(v == 1.0 for v in [cases["half pixel 33x9"].tap_stats(0)[2]])
    m = cases["minify 600x200 to 64x16"]
    x5, y5 = warpref.luma_positions(m.meshes[0][0], 8, 64, 16)
    assert int(x5.max() - x5.min()) >> 5 >= 580 and int(y5.max() - y5.min()) >> 5 >= 180
    ln = cases["lens 96x64"].meshes[0][0].astype(np.int64)
    ident = warpref.mesh_orient(96, 64, 0, 32)[1].astype(np.int64)
    assert np.abs(ln - ident).max() > 3 * 256 and cases["lens 96x64"].tap_stats(0)[0] > 0.9
    assert np.abs(cases["rotate 30"].meshes[0][0][0, 0].astype(np.int64) - np.array([256 * 23.5 * (1 - math.cos(math.pi / 6) + math.sin(math.pi / 6)),
                                                                                     256 * 23.5 * (1 - math.sin(math.pi / 6) - math.cos(math.pi / 6))])).max() <= 1
    # the launch table: more jobs than two launches take, panes of one surface, a skipped job among them
    t = cases["launch table"]
    assert t.n == 130 > 2 * njobs and njobs not in (1, 64 + 3, 130) and t.srcs[77] is None and len({d[0] for d in t.dsts}) == 130
    seen["panes"] = sum(1 for d in t.dsts if d[0] != t.surfaces[0][0])
    assert seen["panes"] == 129


def test_cases_build_quickly():
    """the cases are small: both formats' arenas together stay below 4 MB"""
    assert sum(len(c.start) for fmt in fuzzcases.FORMATS for c in fuzzcases.cases(fmt).values()) < 4 << 20
