"""Heat maps, without a GPU: the nine exported symbols, the layout of the two spec structs in the ctypes mirror and the constants in the header, the
phrases of the contract, the host glue under ASan + UBSan (san/heat_driver.cc, run as a child process: every rejection with its message), the built-in
palette of the library against heatref's, tests/heat/heatref.py (the numpy restatement of the contract the GPU tests compare with) pinned to a
deliberately naive second implementation -- Python loops per pixel and per box over a dict of cells -- some properties by name, the seeded cases of the
GPU fuzz held to the conditions that keep it from passing vacuously, and the device entry points failing the way every entry point of the library
does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from heat import fuzzcases, heatref

SYMBOLS = ["ffgpu_heat_state_bytes", "ffgpu_heat_spec_check", "ffgpu_heat_blend_spec_check", "ffgpu_heat_palette", "ffgpu_heat_reset_dev",
           "ffgpu_heat_boxes_dev", "ffgpu_exec_heat", "ffgpu_heat_blend_bgr_dev", "ffgpu_heat_blend_nv12_dev"]
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
F32 = np.float32
MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module", autouse=True)
def feature(capi):
    """every test of this file is a test of the feature, those that pin heatref and the fuzz's seeds too: a reference is worth what the library it
    restates carries, so each of them needs the built library to export the family"""
    missing = [s for s in SYMBOLS if s not in capi.EXPORTS or not hasattr(capi.lib(), s)]
    assert not missing, "libffcnn_hip.so lacks %s" % missing


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_heat_symbols_exported(capi):
    assert len(SYMBOLS) == 9
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_heat_struct_layout(capi):
    Sp, Bs = capi.HeatSpec, capi.HeatBlendSpec
    assert (C.sizeof(Sp), C.sizeof(Bs)) == (56, 48)
    assert [getattr(Sp, f).offset for f in ("gw", "gh", "cell_log2", "mode", "flags", "anchor", "spread", "gain", "decay_shift", "min_score", "classes", "nclasses",
                                            "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 52]
    assert [getattr(Bs, f).offset for f in ("gw", "gh", "cell_log2", "full_scale", "floor", "opacity", "sampling", "flags", "palette", "reserved")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert (capi.HEAT_MAX, capi.HEAT_DETS, capi.HEAT_ROW, capi.HEAT_ANCHOR, capi.HEAT_BOX, capi.HEAT_NEAREST, capi.HEAT_SMOOTH, capi.HEAT_RAMP_ALPHA, capi.HEAT_ENTRIES,
            capi.HEAT_MERGED, capi.HEAT_STATE_HEADER) == (MAX, 128, 8, 0, 1, 0, 1, 1, 0, 1, 16) == \
        (heatref.MAX, heatref.DETS, heatref.ROW, heatref.ANCHOR, heatref.BOX, heatref.NEAREST, heatref.SMOOTH, heatref.RAMP_ALPHA, 0, 1, heatref.STATE_HEADER)
    assert capi.HEAT_ROW_HEADER == heatref.HEADER and capi.BOX_DTYPE == heatref.BOX_DTYPE and capi.DETS_DTYPE == heatref.DETS_DTYPE
    sp = capi.heat_spec(7, 3, 4, capi.HEAT_ANCHOR, 1, 2, 9, 5, 0.5, classes=[1, 0, 2])
    assert (sp.gw, sp.gh, sp.cell_log2, sp.mode, sp.flags, sp.anchor, sp.spread, sp.gain, sp.decay_shift, sp.min_score, sp.nclasses, sp.reserved) == \
        (7, 3, 4, 0, 0, 1, 2, 9, 5, 0.5, 3, 0)
    assert bytes((C.c_ubyte * 3).from_address(sp.classes)) == bytes([1, 0, 1])
    capi.heat_spec_check(sp)
    sp.mode = capi.HEAT_BOX
    with pytest.raises(Exception, match=re.escape("spread 2 with FFGPU_HEAT_BOX (0 then)")):
        capi.heat_spec_check(sp)
    pal = np.arange(768, dtype=np.uint8).reshape(256, 3)
    bs = capi.heat_blend_spec(7, 3, 4, 100, 5, 60, smooth=True, ramp_alpha=True, palette=pal)
    assert (bs.gw, bs.gh, bs.cell_log2, bs.full_scale, bs.floor, bs.opacity, bs.sampling, bs.flags, list(bs.reserved)) == (7, 3, 4, 100, 5, 60, 1, 1, [0, 0])
    assert bytes((C.c_ubyte * 8).from_address(bs.palette)) == bytes([0, 1, 2, 0, 3, 4, 5, 0])
    capi.heat_blend_spec_check(bs)
    bs.full_scale = -1
    with pytest.raises(Exception, match="negative full_scale -1"):
        capi.heat_blend_spec_check(bs)
    assert capi.heat_blend_spec(1, 1, 1).palette is None
    assert capi.heat_state_bytes(3, 5, 3) == 3 * 80 == heatref.state_nbytes(3, 5, 3) and capi.heat_state_bytes(65536, 128, 128) == 65536 * (16 + 65536)
    assert capi.heat_state_bytes(1, 1, 1) == 32 and capi.heat_state_bytes(2, 17, 5) == 2 * 368 == heatref.state_nbytes(2, 17, 5)
    assert [capi.heat_state_bytes(*a) for a in ((0, 1, 1), (65537, 1, 1), (1, 0, 1), (1, 129, 1), (1, 1, 0), (1, 1, 129), (-1, -1, -1))] == [0] * 7
    st = heatref.State(2, 3, 2)
    st.hdr[1] = (5, 77, 0, 0)
    st.cells[1, 1, 2] = 77
    hdr, cells = capi.heat_state(np.frombuffer(st.tobytes(), np.uint8), 2, 3, 2)
    assert hdr.tolist() == [[0, 0, 0, 0], [5, 77, 0, 0]] and cells.tobytes() == st.cells.tobytes() and int(cells[1, 1, 2]) == 77


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    text = re.sub(r"\s*\n \*\s*", " ", hdr)                                             # (a phrase may run over a line of the comment)
    for phrase in ("} ffgpu_heat_spec;", "} ffgpu_heat_blend_spec;", "tests/heat/heatref.py",
                   "56 bytes: gw 0, gh 4, cell_log2 8, mode 12, flags 16, anchor 20, spread 24, gain 28, decay_shift 32,", "min_score 36, classes 40, nclasses 48, reserved 52",
                   "48 bytes: gw 0, gh 4, cell_log2 8, full_scale 12, floor 16, opacity 20, sampling 24, flags 28, palette 32, reserved 40",
                   "a 16-byte header { int frames; unsigned peak; int reserved[2]; }", "all-zero is the valid empty state", "the stream's block rounded up to 16 bytes",
                   "cell (i, j) covers x in [i c, (i + 1) c - 1] and y in [j c, (j + 1) c - 1]", "it need not match any frame's size",
                   "a cell is read as unsigned and clamped to FFGPU_HEAT_MAX where it is read", "a dashboard copies it out as it is",
                   "score >= min_score (a NaN score never qualifies", "until FFGPU_HEAT_DETS are; further qualifying boxes are counted in `dropped`",
                   "every cell becomes v - ((v + (1 << k) - 1) >> k)", "old heat reaches exactly zero", "Decay also runs for a frame without boxes",
                   "sums are taken in 64 bits and the cell is min(sum, FFGPU_HEAT_MAX)", "do not depend on order",
                   "px = (x1 + x2) * 0.5f; py = anchor ? y2 : (y1 + y2) * 0.5f", "If A lies outside [0, gw c - 1] x [0, gh c - 1]",
                   "every grid cell at Chebyshev distance d <= spread from (i, j) receives gain >> d", "cells beyond the grid are simply not there",
                   "If a > c, b > d, or the clipped region is empty, the box is counted in `outside`", "from (X0 >> k, Y0 >> k) to (X1 >> k, Y1 >> k) receives gain",
                   "spread must be 0", "peak = the largest cell; frames += 1", "{ considered, dropped, outside, frame, peak, saturated, 0, 0 }",
                   "AS IT IS WHEN THE LAUNCH RUNS IN STREAM ORDER", "several frames of one stream in one call all show the same map",
                   "streams[t] == -1 leaves the target untouched", "a pixel with x >= gw c or y >= gh c is untouched", "a peak of 0 draws nothing in that target",
                   "L(i, j) = min(255, (cell(i, j) * 255) / F), in 64-bit integers, rounded down", "i0 = (x - h) >> k, an arithmetic shift, so i0 may be -1",
                   "level = (L00 (c - fx)(c - fy) + L10 fx (c - fy) + L01 (c - fx) fy + L11 fx fy + c c / 2) >> (2 k)", "a pixel with level < max(floor, 1) is not written",
                   "a = (level * opacity + 127) / 255", "new = (old (255 - a) + pal[level][ch] a + 127) / 255", "takes the level and alpha of luma pixel (2 i, 2 j)",
                   "The state is only read", "ch = (c0 (v1 - v) + c1 (v - v0) + (v1 - v0) / 2) / (v1 - v0)", "Y = (29 B + 150 G + 77 R + 128) >> 8",
                   "U = ((128 B - 85 G - 43 R + 128) >> 8) + 128", "V = ((-21 B - 107 G + 128 R + 128) >> 8) + 128",
                   "Redact and blur first, then the heat blend, then draw, outline, trails and caption", "64 records per launch", "64 targets per launch",
                   "There is no executor form: the blend reads state, not records", "A rejected call leaves the state as it was", "a non-zero spread with FFGPU_HEAT_BOX",
                   "a negative full_scale"):
        assert phrase in text, phrase
    assert hdr.index("---- track trails:") < hdr.index("---- heat maps:")
    for name, val in (("FFGPU_HEAT_DETS", 128), ("FFGPU_HEAT_ROW", 8), ("FFGPU_HEAT_ANCHOR", 0), ("FFGPU_HEAT_BOX", 1), ("FFGPU_HEAT_NEAREST", 0), ("FFGPU_HEAT_SMOOTH", 1),
                      ("FFGPU_HEAT_RAMP_ALPHA", 1), ("FFGPU_HEAT_ENTRIES", 0), ("FFGPU_HEAT_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    assert int(re.search(r"#define FFGPU_HEAT_MAX\s+(0x[0-9a-f]+)", hdr).group(1), 16) == MAX
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_heat.inc"' in inc and inc.index('#include "ffgpu_trails.inc"') < inc.index('#include "ffgpu_heat.inc"')
    host = open(os.path.join(CSRC, "ffgpu_heat_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    assert int(re.search(r"#define HEAT_ARG_ENTRIES\s+(\d+)", host).group(1)) == 64 and int(re.search(r"#define HEAT_ARG_TARGETS\s+(\d+)", host).group(1)) == 64
    kern = open(os.path.join(CSRC, "ffgpu_heat.inc")).read()
    assert "atomic" not in kern.replace("global atomic", "") and "printf" not in kern and "asm" not in kern and "__threadfence" not in kern
    assert "block_consider(" in kern and kern.count("block_fold(") >= 2 and "k_heat_accumulate" in kern and "k_heat_blend" in kern     # the workgroup primitives, not copies
    assert "static_assert(sizeof(HeatArgs)" in kern and "sizeof(HeatBlendArgs)" in kern and "4096 - 256" in kern


# ------------------------------------------------------------------------------------------------- the palette; the host glue
def test_palette_equals_heatref(capi):
    for nv12 in (False, True):
        got = capi.heat_palette(nv12)
        assert got.shape == (256, 4) and got.tobytes() == heatref.palette(nv12).tobytes(), nv12
    assert capi.heat_palette()[[0, 64, 128, 192, 255], :3].tolist() == [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255]]
    assert capi.lib().ffgpu_heat_palette(0, None) < 0 and "NULL out" in capi.last_error()


def test_host_glue_under_the_sanitizers():
    """san/heat_driver.cc: the state's size, the plans of the two specs, the palette and every argument check of ffgpu_heat_host.hpp on the CPU under
    ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "heat"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_heat_san")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"heat_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 120, out[-1]
    text = "\n".join(out)
    for msg in ("a grid of 0 x 23 cells (1..128 each)", "cell_log2 9 is outside 1..8", "mode 2 is neither FFGPU_HEAT_ANCHOR nor FFGPU_HEAT_BOX", "unknown flags 0x1",
                "anchor 2 is neither 0 nor 1", "spread 5 is outside 0..4", "spread 2 with FFGPU_HEAT_BOX (0 then)", "gain 65537 is outside 1..65536",
                "decay_shift 17 is outside 0..16", "nclasses 3 (0 with NULL classes, else 1..256)", "reserved must be 0", "negative full_scale -1", "floor 256 is outside 0..255",
                "opacity 0 is outside 1..255", "sampling 2 is neither FFGPU_HEAT_NEAREST nor FFGPU_HEAT_SMOOTH", "unknown flags 0x2", "NULL streams", "NULL spec", "NULL state",
                "NULL rows", "NULL targets", "0 targets", "nstreams 65537", "the state must be 16-byte aligned", "target 1: stream 2 is outside -1 .. 1", "target 3: stream -2",
                "target 1: bad size 0 x 33", "target 0: pitch 100 is below 3 w = 195", "is odd (U V pairs are written"):
        assert msg in text, msg
    r = subprocess.run([exe, "palette"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().split() == [heatref.palette(False).tobytes().hex(), heatref.palette(True).tobytes().hex()]


def test_heat_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_heat_reset_dev(None, 1, 1, 1, -1, None),
                 lambda: L.ffgpu_heat_boxes_dev(None, None, 0, None, None, 1, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_heat(None, 0, None, 1, None, None, 1, None, None),
                 lambda: L.ffgpu_heat_blend_bgr_dev(None, 1, None, None, 1, None, None),
                 lambda: L.ffgpu_heat_blend_nv12_dev(None, 1, None, None, 1, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


# ------------------------------------------------------------------------------------------------- heatref against a naive second implementation
def naive_f2i(v):
    v = float(F32(v))
    if v != v:
        return 0
    return MAX if v >= 2.0 ** 31 else -2 ** 31 if v <= -2.0 ** 31 else int(v)


def naive_frame(grid, frames, boxes, sp):
    """one frame over a dict of cells { (i, j): value }, box by box, cell by cell; returns the row"""
    c = 1 << sp.cell_log2
    for key in grid:
        grid[key] = min(grid[key], MAX)
    qual = [b for b in boxes if float(b["score"]) >= float(sp.min_score) and sp.allowed(b["type"])]
    dropped, qual = max(0, len(qual) - 128), qual[:128]
    if sp.decay_shift:
        for key in grid:
            v = grid[key]
            loss = -(-v // (1 << sp.decay_shift))                                   # v / 2^k, rounded up
            grid[key] = v - loss
    outside, add = 0, {}
    for b in qual:
        if sp.mode == heatref.ANCHOR:
            with np.errstate(all="ignore"):
                ax = naive_f2i((F32(b["x1"]) + F32(b["x2"])) * F32(0.5))
                ay = naive_f2i(F32(b["y2"]) if sp.anchor else (F32(b["y1"]) + F32(b["y2"])) * F32(0.5))
            if not (0 <= ax < sp.gw * c and 0 <= ay < sp.gh * c):
                outside += 1
                continue
            for j in range(sp.gh):
                for i in range(sp.gw):
                    d = max(abs(i - ax // c), abs(j - ay // c))
                    if d <= sp.spread:
                        add[i, j] = add.get((i, j), 0) + sp.gain // 2 ** d
        else:
            x0, y0, x1, y1 = (naive_f2i(b[k]) for k in ("x1", "y1", "x2", "y2"))
            hit = [(i, j) for j in range(sp.gh) for i in range(sp.gw)
                   if x0 <= x1 and y0 <= y1 and max(x0, i * c) <= min(x1, i * c + c - 1) and max(y0, j * c) <= min(y1, j * c + c - 1)]
            if not hit:
                outside += 1
            for key in hit:
                add[key] = add.get(key, 0) + sp.gain
    for key, v in add.items():
        grid[key] = min(grid[key] + v, MAX)
    peak = max(grid.values())
    return [len(qual), dropped, outside, frames, peak, sum(v == MAX for v in grid.values()), 0, 0]


def naive_level(grid, peak, bs, x, y):
    """the level of pixel (x, y) inside the extent, or None: nothing is drawn"""
    F = bs.full_scale if bs.full_scale >= 1 else min(peak, MAX)
    if F == 0:
        return None
    c = 1 << bs.cell_log2

    def L(i, j):
        return min(255, min(grid[min(max(i, 0), bs.gw - 1), min(max(j, 0), bs.gh - 1)], MAX) * 255 // F)
    if not bs.smooth:
        return L(x // c, y // c)
    h = c // 2
    i0, j0, fx, fy = (x - h) // c, (y - h) // c, (x - h) % c, (y - h) % c          # (Python's // and %: the floor and its remainder)
    return (L(i0, j0) * (c - fx) * (c - fy) + L(i0 + 1, j0) * fx * (c - fy) + L(i0, j0 + 1) * (c - fx) * fy + L(i0 + 1, j0 + 1) * fx * fy + c * c // 2) // (c * c)


def naive_alpha(bs, lev):
    if lev is None or lev < max(bs.floor, 1):
        return 0
    return (lev * bs.opacity + 127) // 255 if bs.ramp_alpha else bs.opacity


def naive_blend(buf, d, fmt, grid, peak, bs):
    pal = heatref.palette(fmt == "nv12") if bs.palette is None else bs.palette
    c = 1 << bs.cell_log2
    w, h = (d[1], d[2]) if fmt == "bgr" else (d[2], d[3])
    for y in range(h):
        for x in range(w):
            if x >= bs.gw * c or y >= bs.gh * c:
                continue
            lev = naive_level(grid, peak, bs, x, y)
            a = naive_alpha(bs, lev)
            if a == 0:
                continue
            where = [(d[0] + y * d[3] + 3 * x + ch, ch) for ch in range(3)] if fmt == "bgr" else [(d[0] + y * d[4] + x, 0)]
            if fmt == "nv12" and x % 2 == 0 and y % 2 == 0:
                where += [(d[1] + (y // 2) * d[5] + x + ch - 1, ch) for ch in (1, 2)]
            for at, ch in where:
                buf[at] = (int(buf[at]) * (255 - a) + int(pal[lev][ch]) * a + 127) // 255


@pytest.mark.parametrize("mode", [heatref.ANCHOR, heatref.BOX])
def test_heatref_accumulate_equals_the_naive_dict(mode):
    rng = np.random.default_rng(7400 + mode)
    for trial in range(40):
        gw, gh, k = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
        sp = heatref.Spec(gw, gh, k, mode, int(rng.integers(0, 2)), 0 if mode else int(rng.integers(0, 5)), int(rng.choice([1, 3, 65536])), int(rng.choice([0, 1, 4, 16])),
                          float(rng.choice([0.0, 0.5])), None if trial % 3 else [1, 1, 0, 1])
        st = heatref.State(1, gw, gh)
        if trial % 4 == 0:
            st.cells[:] = rng.integers(0, 2 ** 32, st.cells.shape, dtype=np.uint64)
        grid = {(i, j): int(st.cells[0, j, i]) for j in range(gh) for i in range(gw)}
        for f in range(4):
            boxes = fuzzcases.rand_boxes(rng, int(rng.integers(0, 8)), gw << k, gh << k, 0.15)
            rec = np.zeros(1, heatref.DETS_DTYPE)
            rec[0]["count"], rec[0]["box"][:len(boxes)] = len(boxes), boxes
            rows = heatref.accumulate(rec, None, 0, None, [0], sp, st)
            assert rows[0].tolist() == naive_frame(grid, f, boxes, sp), (trial, f)
            assert {(i, j): int(st.cells[0, j, i]) for j in range(gh) for i in range(gw)} == grid and st.hdr[0].tolist() == [f + 1, max(grid.values()), 0, 0]


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
@pytest.mark.parametrize("smooth", [False, True])
def test_heatref_blend_equals_the_naive_loops(fmt, smooth):
    rng = np.random.default_rng(7500 + smooth)
    for trial in range(12):
        gw, gh, k = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
        pal = None if trial % 2 else rng.integers(0, 256, (256, 3), dtype=np.uint8)
        bs = heatref.BlendSpec(gw, gh, k, int(rng.choice([0, 0, 50, 900])), int(rng.choice([0, 1, 128])), int(rng.choice([1, 90, 255])), smooth, bool(trial & 2), pal)
        sizes = [(int(rng.integers(1, 21)), int(rng.integers(1, 18))) for _ in range(3)]
        top = int(rng.choice([0, 60, 1000, 2 ** 32 - 1]))

        def fill(st, r):                                                             # cells up to `top`, a peak that may be 0 or below the cells
            st.raw[:] = 0
            st.cells[:] = np.where(r.random(st.cells.shape) < 0.6, r.integers(0, top + 1, st.cells.shape, dtype=np.uint64), 0).astype(np.uint32)
            st.hdr[:, 1] = int(r.choice([0, top // 2, top]))
        if trial == 5:
            fill = fuzzcases.junk
        c = fuzzcases.BlendCase(7510 + trial, fmt, bs, 2, sizes + [None], [0, 1, -1, 0], fill)
        want = c.start.copy()
        for d, s in zip(c.desc, c.streams):
            if d is not None and s >= 0:
                grid = {(i, j): int(c.state.cells[s, j, i]) for j in range(gh) for i in range(gw)}
                naive_blend(want, d, fmt, grid, int(c.state.hdr[s, 1]), bs)
        assert c.want.tobytes() == want.tobytes(), (trial, sizes)


# ------------------------------------------------------------------------------------------------- properties by name
def test_the_division_identity():
    """n / 255 as the kernel forms it, over every numerator a blend or a ramped alpha can have"""
    n = np.arange(65152 + 1, dtype=np.int64)
    assert 255 * 255 + 127 == 65152 and ((n + 1 + (n >> 8)) >> 8).tolist() == (n // 255).tolist()
    kern = open(os.path.join(CSRC, "ffgpu_heat.inc")).read()
    assert "return (n + 1u + (n >> 8)) >> 8;" in kern


def one_box(x, y, type_=0):
    rec = np.zeros(1, heatref.DETS_DTYPE)
    rec[0]["count"], rec[0]["box"][0] = 1, (type_, 1.0, x, y, x, y)
    return rec


def empty():
    return np.zeros(1, heatref.DETS_DTYPE)


def test_decay_reaches_exactly_zero():
    for k in (1, 4, 16):
        sp = heatref.Spec(2, 1, 3, heatref.ANCHOR, 0, 0, 65536, k)
        st = heatref.State(1, 2, 1)
        heatref.accumulate(one_box(3, 3), None, 0, None, [0], sp, st)
        assert st.cells[0].tolist() == [[65536, 0]]                                  # (decay runs before the deposit: the frame's own deposit is whole)
        seen, frames = [int(st.cells[0, 0, 0])], 0
        while seen[-1]:
            heatref.accumulate(empty(), None, 0, None, [0], sp, st)
            seen.append(int(st.cells[0, 0, 0]))
            frames += 1
            assert seen[-1] < seen[-2] and frames < 2 ** 18                         # at least 1 per frame: it ends
        assert seen[-1] == 0 and st.hdr[0].tolist() == [frames + 1, 0, 0, 0]


def test_saturation_does_not_depend_on_list_order():
    rng = np.random.default_rng(7600)
    sp = heatref.Spec(3, 2, 3, heatref.ANCHOR, 0, 2, 65536, 0)
    boxes = fuzzcases.rand_boxes(rng, 100, 24, 16, 0.0)
    boxes["score"] = 1
    got = []
    for perm in (np.arange(100), rng.permutation(100), np.arange(100)[::-1]):
        st = heatref.State(1, 3, 2)
        st.cells[:] = MAX - 20 * 65536
        st.cells[0, 1, 2] = 0                                                        # (one cell far from the ceiling)
        rec = np.zeros(1, heatref.DETS_DTYPE)
        rec[0]["count"], rec[0]["box"][:100] = 100, boxes[perm]
        rows = heatref.accumulate(rec, None, 0, None, [0], sp, st)
        got.append((st.tobytes(), rows.tobytes()))
    assert got[0] == got[1] == got[2] and int(rows[0, 5]) >= 1 and (st.cells < MAX).any()


def test_two_records_in_one_call_equal_two_calls():
    c = fuzzcases.acc_cases()["grid 3x2 box"]
    st = c.state0.copy()
    rows = np.zeros((c.n, heatref.ROW), "<i4")
    for t in range(c.n):
        rows[t] = heatref.accumulate(c.recs[t:t + 1], c.flat, c.stride, [c.first[t]], [c.streams[t]], c.spec, st)[0]
    assert rows.tobytes() == c.rows.tobytes() and st.tobytes() == c.state.tobytes()


# ------------------------------------------------------------------------------------------------- the seeds of the GPU fuzz
def test_accumulate_seeds_meet_the_conditions_on_the_reference_alone():
    cases = fuzzcases.acc_cases()
    assert tuple(cases) == fuzzcases.ACC_NAMES
    tot = {}
    for c in cases.values():
        for k, v in c.trace.items():
            tot[k] = tot.get(k, 0) + v
    for k in ("anchor_border_lo", "anchor_border_hi", "anchor_negative", "anchor_beyond", "spread_over_edge", "box_several_cells", "box_clipped", "box_outside",
              "reached_max", "decay_to_zero", "top_bit"):
        assert tot.get(k, 0) > 0, k
    assert sum(int(c.rows[:, 1].sum()) for c in cases.values()) > 0 and int(cases["long list"].rows[0, 1]) == 172      # dropped
    assert sum(int(c.rows[:, 2].sum()) for c in cases.values()) > 0                                                    # outside
    assert 2 * sum(c.grid_changed for c in cases.values()) >= len(cases)
    assert (cases["junk state"].state0.cells >> 31).any() and int(cases["saturate"].rows[-1, 5]) == 6 and int(cases["saturate"].rows[0, 3]) == -2
    assert {(c.spec.gw, c.spec.gh) for c in cases.values()} == {(1, 1), (3, 2), (17, 5), (128, 128)}
    assert {c.spec.cell_log2 for c in cases.values()} == {1, 3, 6, 8} and {c.spec.decay_shift for c in cases.values()} == {0, 1, 4, 16}
    assert {c.spec.spread for c in cases.values()} == {0, 1, 4} and {c.spec.gain for c in cases.values()} >= {1, 65536} and {c.spec.mode for c in cases.values()} == {0, 1}
    assert cases["records 65"].n == 65 and cases["records 130"].n == 130 and -1 in cases["records 130"].streams and cases["grid 3x2 box"].first is not None
    assert np.isnan(cases["nan min_score"].spec.min_score) and not cases["nan min_score"].rows[:, 0].any() and cases["grid 3x2 box"].spec.classes == [True, False, True, True]
    assert cases["own boxes"].flat is None and int(cases["own boxes"].rows[2, 0]) == 128 and int(cases["clamped counts"].rows[0, 0]) > 2
    assert 2 not in cases["grid 17x5 anchor"].streams and max(int(r["nfull"]) for r in cases["long list"].recs) == 300
    nonfinite = sum(int((~np.isfinite(c.flat[k])).sum()) for c in cases.values() if c.flat is not None for k in ("x1", "y1", "x2", "y2"))
    assert nonfinite > 0 and any((c.flat["x1"] > c.flat["x2"]).any() for c in cases.values() if c.flat is not None)
    for c in cases.values():
        assert c.state_off % 16 == 0 and (c.want != c.start).any()
        lo = min(o for _, o, _ in c.regions())
        assert c.want[:lo].tobytes() == c.start[:lo].tobytes()


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_blend_seeds_meet_the_conditions_on_the_reference_alone(fmt):
    cases = fuzzcases.blend_cases(fmt)
    assert tuple(cases) == fuzzcases.BLEND_NAMES
    tot = {}
    for c in cases.values():
        for k, v in c.trace.items():
            tot[k] = tot.get(k, 0) + v
        assert not c.grid_nonzero() or (c.want != c.start).any(), c.what               # every case with a non-zero grid changes a byte
        n = heatref.state_nbytes(c.nstreams, c.bspec.gw, c.bspec.gh)
        assert c.want[c.state_off:c.state_off + n].tobytes() == c.start[c.state_off:c.state_off + n].tobytes()          # the state is only read
    assert 2 * sum(c.inside_unchanged for c in cases.values()) >= len(cases)
    for k in ("right_of_extent", "below_extent", "smooth_i0_negative", "smooth_i1_clamped", "block_below_next_to_drawn", "level_clamped", "auto_peak_zero", "ramp_alpha_zero"):
        assert tot.get(k, 0) > 0, k
    assert {c.bspec.opacity for c in cases.values()} >= {1, 255} and {c.bspec.floor for c in cases.values()} == {0, 1, 128}
    assert {c.bspec.cell_log2 for c in cases.values()} >= {1, 3, 6, 8} and {c.bspec.smooth for c in cases.values()} == {False, True}
    assert any(c.bspec.palette is not None for c in cases.values()) and any(c.bspec.palette is None for c in cases.values())
    sizes = {wh for c in cases.values() for wh in c.targets if wh}
    assert sizes >= {(1, 1), (2, 3), (5, 4), (63, 66), (64, 65), (65, 64), (66, 63), (129, 70)}
    c65 = cases["targets 65"]
    assert len(c65.targets) == 65 and None in c65.targets and -1 in c65.streams and c65.targets[64] is None and c65.streams[63] == -1
    assert any(d is not None and d[0] % 2 == 1 for c in cases.values() for d in c.desc)                                   # odd base addresses
    if fmt == "nv12":
        assert all(d[1] % 2 == 0 for c in cases.values() for d in c.desc if d) and any(d[1] % 4 == 2 for c in cases.values() for d in c.desc if d)
    junk = cases["junk state"]
    assert (junk.state.cells >> 31).any() and (junk.state.hdr[:, 1] >> 31).any()
