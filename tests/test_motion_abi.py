"""Motion maps, without a GPU: the seven exported symbols, the layout of the spec struct in the ctypes mirror and the constants in the header, the
phrases of the contract, the host glue under ASan + UBSan (san/motion_driver.cc, run as a child process: every rejection with its message),
tests/motion/motionref.py (the numpy restatement of the contract the GPU tests compare with) pinned to a deliberately naive second implementation --
Python loops per pixel and per box --, some properties by name, the seeded cases of the GPU fuzz held to the conditions that keep it from passing
vacuously, and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from motion import fuzzcases, motionref

SYMBOLS = ["ffgpu_motion_state_bytes", "ffgpu_motion_spec_check", "ffgpu_motion_reset_dev", "ffgpu_motion_update_bgr_dev", "ffgpu_motion_update_nv12_dev",
           "ffgpu_motion_gate_dev", "ffgpu_exec_motion_gate"]
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
F32 = np.float32


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module", autouse=True)
def feature(capi):
    """every test of this file is a test of the feature, those that pin motionref and the fuzz's seeds too: a reference is worth what the library it
    restates carries, so each of them needs the built library to export the family"""
    missing = [s for s in SYMBOLS if s not in getattr(capi, "EXPORTS", ()) or not hasattr(capi.lib(), s)]
    assert not missing, "libffcnn_hip.so lacks %s" % missing


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_motion_symbols_exported(capi):
    assert len(SYMBOLS) == 7
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_motion_struct_layout(capi):
    Sp = capi.MotionSpec
    assert C.sizeof(Sp) == 64
    assert [getattr(Sp, f).offset for f in ("w", "h", "cell_log2", "threshold", "learn_shift", "learn_shift_changed", "min_pixels", "cover", "warmup", "flags", "min_score",
                                            "nclasses", "classes", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56]
    assert (capi.MOTION_DETS, capi.MOTION_ROW, capi.MOTION_WORDS, capi.MOTION_MAX_SIDE, capi.MOTION_GATE_INVERT, capi.MOTION_ENTRIES, capi.MOTION_MERGED,
            capi.MOTION_STATE_HEADER) == (128, 16, 8, 8192, 1, 0, 1, 16) == \
        (motionref.DETS, motionref.ROW, motionref.WORDS, motionref.MAX_SIDE, motionref.GATE_INVERT, 0, 1, motionref.STATE_HEADER)
    assert capi.MOTION_ROW_HEADER == motionref.ROW_HEADER and capi.MOTION_WORDS_HEADER == motionref.WORDS_HEADER
    assert capi.BOX_DTYPE == motionref.BOX_DTYPE and capi.DETS_DTYPE == motionref.DETS_DTYPE
    sp = capi.motion_spec(65, 33, 4, 20, 3, 9, 16, 64, 30, True, 0.5, classes=[1, 0, 2])
    assert (sp.w, sp.h, sp.cell_log2, sp.threshold, sp.learn_shift, sp.learn_shift_changed, sp.min_pixels, sp.cover, sp.warmup, sp.flags, sp.min_score, sp.nclasses,
            list(sp.reserved)) == (65, 33, 4, 20, 3, 9, 16, 64, 30, 1, 0.5, 3, [0, 0])
    assert bytes((C.c_ubyte * 3).from_address(sp.classes)) == bytes([1, 0, 1])
    capi.motion_spec_check(sp)
    sp.min_pixels = 257
    with pytest.raises(Exception, match=re.escape("min_pixels 257 is outside 1..256")):
        capi.motion_spec_check(sp)
    assert capi.motion_spec(1, 1, 2).classes is None and capi.motion_spec(1, 1, 2).flags == 0
    for args in ((1, 1, 1, 2), (3, 7, 5, 3), (2, 17, 9, 2), (1, 1920, 1080, 4), (2, 67, 35, 3), (65536, 8192, 8192, 2), (5, 64, 64, 6)):
        assert capi.motion_state_bytes(*args) == motionref.state_nbytes(*args) > 0, args
    assert capi.motion_state_bytes(1, 1, 1, 2) == 48 and capi.motion_state_bytes(1, 1920, 1080, 4) == 16 + 2 * 1920 * 1080 + 4 * 120 * 68
    for args in ((0, 1, 1, 2), (65537, 1, 1, 2), (1, 0, 1, 2), (1, 8193, 1, 2), (1, 1, 0, 2), (1, 1, 8193, 2), (1, 1, 1, 1), (1, 1, 1, 7), (-1, -1, -1, -1)):
        assert capi.motion_state_bytes(*args) == 0 == motionref.state_nbytes(*args), args
    st = motionref.State(2, 17, 9, 2)
    st.hdr[1] = (5, 0, 0, 0)
    st.plane[1, 8, 16] = 0xabcd
    st.cells[1, 2, 4] = 13
    hdr, plane, cells = capi.motion_state(np.frombuffer(st.tobytes(), np.uint8), 2, 17, 9, 2)
    assert hdr.tolist() == [[0, 0, 0, 0], [5, 0, 0, 0]] and plane.shape == (2, 9, 17) and int(plane[1, 8, 16]) == 0xabcd and plane.tobytes() == st.plane.tobytes()
    assert cells.shape == (2, 3, 5) and int(cells[1, 2, 4]) == 13 and cells.tobytes() == st.cells.tobytes()


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    text = re.sub(r"\s*\n \*\s*", " ", hdr)                                             # (a phrase may run over a line of the comment)
    for phrase in ("} ffgpu_motion_spec;", "tests/motion/motionref.py",
                   "64 bytes: w 0, h 4, cell_log2 8, threshold 12, learn_shift 16, learn_shift_changed 20, min_pixels 24, cover 28,",
                   "warmup 32, flags 36, min_score 40, nclasses 44, classes 48, reserved 56", "a header { int frames; int reserved[3]; }", "all-zero is the valid empty",
                   "h rows of ALIGN(w, 8) unsigned short", "luma in 8.8 fixed point", "the padding shorts of a row are never written", "rounded up to 16 bytes",
                   "Plane and cells are documented, readable products", "gw = ceil(w / c) by gh = ceil(h / c) cells", "The trails family's \"motion row\" is a different thing",
                   "NV12: the Y byte (the UV plane is not read)", "y = (29 B + 150 G + 77 R + 128) >> 8", "cur = y << 8, bg the stored short (any value) and d = cur - bg as int",
                   "If the header's `frames` is 0 the pixel is not changed and bg = cur", "CHANGED when |d| > threshold << 8",
                   "k = learn_shift_changed for a changed pixel, learn_shift for any other", "bg += sgn(d) * ((|d| + (1 << k) - 1) >> k)", "the model reaches cur exactly",
                   "k == 16: bg stays", "Every cell of the stream is written", "frames += 1 (modulo 2^32)",
                   "{ frame (frames before the increment), changed (pixels), active (cells with count >= min_pixels), x0, y0, x1, y1, warm, 0 x 8 }",
                   "x1 = min(c * (max i + 1), w) - 1", "with no active cell it is (0, 0, -1, -1)", "warm = (frames after the increment) > warmup",
                   "streams[t] == -1 or a NULL pixel address leaves the state alone, and the row is zero", "whose w or h differ from the spec's is rejected",
                   "byte for byte what one call per frame leaves", "AS IT IS WHEN THE LAUNCH RUNS IN STREAM ORDER", "with the cap FFGPU_MOTION_DETS",
                   "If a > c, b > d or the clip is empty the box is counted in `outside` and touched = active = 0", "cells from (X0 >> k, Y0 >> k) to (X1 >> k, Y1 >> k)",
                   "The stream is WARM when frames > warmup", "touched >= 1 and active * 256 >= cover * touched", "the gate fails open",
                   "{ considered, dropped, outside, moving, warm, frames, 0, 0 }", "then { touched, active } per list box, zero for a box that was not considered",
                   "laid out by the zones gated record's rules word for word", "The outputs must not overlap the inputs", "every output byte of the entry is written, as zero",
                   "update, forward, gate, then track, redact, draw or heat ON THE GATED RECORD", "FFGPU_MOTION_GATE_INVERT gives the boxes that stand still",
                   "ROUND r -- the r-th occurrence of every stream in the call -- behind round r - 1", "a workgroup owns a tile of 64 x 64 pixels",
                   "The update launch only reads `frames`", "No atomics", "A rejected call leaves the state as it was", "64 records per launch"):
        assert phrase in text, phrase
    assert hdr.index("---- heat maps:") < hdr.index("---- motion maps:")
    for name, val in (("FFGPU_MOTION_DETS", 128), ("FFGPU_MOTION_ROW", 16), ("FFGPU_MOTION_WORDS", 8), ("FFGPU_MOTION_GATE_INVERT", 1), ("FFGPU_MOTION_MAX_SIDE", 8192),
                      ("FFGPU_MOTION_ENTRIES", 0), ("FFGPU_MOTION_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_motion.inc"' in inc and inc.index('#include "ffgpu_heat.inc"') < inc.index('#include "ffgpu_motion.inc"')
    host = open(os.path.join(CSRC, "ffgpu_motion_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    assert int(re.search(r"#define MOTION_ARG_TARGETS\s+(\d+)", host).group(1)) == 64 and int(re.search(r"#define MOTION_TILE\s+(\d+)", host).group(1)) == 64
    kern = open(os.path.join(CSRC, "ffgpu_motion.inc")).read()
    assert "atomic" not in kern.replace("No atomics", "") and "printf" not in kern and "asm" not in kern and "__threadfence" not in kern
    assert "block_consider(" in kern and kern.count("block_fold(") >= 2 and "block_rank(" in kern                # the workgroup primitives, not copies
    assert "k_motion_update" in kern and "k_motion_row" in kern and "k_motion_gate" in kern
    assert "static_assert(sizeof(MotionArgs)" in kern and "sizeof(MotionGateArgs)" in kern and "4096 - 256" in kern


def test_host_glue_under_the_sanitizers():
    """san/motion_driver.cc: the state's layout, the spec's plan, every argument check of ffgpu_motion_host.hpp and the rounds of an update call on the
    CPU under ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "motion"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_motion_san")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"motion_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 100, out[-1]
    text = "\n".join(out)
    for msg in ("a model of 0 x 33 pixels (1..8192 each)", "a model of 65 x 8193 pixels", "cell_log2 1 is outside 2..6", "cell_log2 7 is outside 2..6", "threshold 0 is outside 1..255",
                "threshold 256 is outside 1..255", "learn_shift -1 is outside 0..16", "learn_shift 17 is outside 0..16", "learn_shift_changed 17 is outside 0..16",
                "min_pixels 0 is outside 1..256", "min_pixels 17 is outside 1..16", "cover 0 is outside 1..256", "cover 257 is outside 1..256", "warmup -1 is outside 0..65535",
                "warmup 65536 is outside 0..65535", "unknown flags 0x2", "unknown flags 0x80000000", "nclasses 3 (0 with NULL classes, else 1..256)", "nclasses 257",
                "reserved must be 0", "NULL targets", "NULL streams", "NULL spec", "NULL state", "NULL rows", "NULL words", "0 targets", "-1 targets", "nstreams 0", "nstreams 65537",
                "the state must be 16-byte aligned", "target 1: stream 2 is outside -1 .. 1", "target 3: stream -2", "target 1: bad size 0 x 33",
                "target 3: 64 x 33 pixels, the spec's model is 65 x 33", "target 5: 65 x 34 pixels, the spec's model is 65 x 33", "target 0: reserved must be 0",
                "target 0: pitch 100 is below 3 w = 195", "target 0: pitch_y 10 is below w = 65", "is odd (U V pairs are written", "target 1: matrix 4",
                "d_out_lists without d_out_records"):
        assert msg in text, msg


def test_motion_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_motion_reset_dev(None, 1, 1, 1, 2, -1, None),
                 lambda: L.ffgpu_motion_update_bgr_dev(None, 1, None, None, None, 1, None, None),
                 lambda: L.ffgpu_motion_update_nv12_dev(None, 1, None, None, None, 1, None, None),
                 lambda: L.ffgpu_motion_gate_dev(None, None, 0, None, None, 1, None, None, 1, None, None, None, None),
                 lambda: L.ffgpu_exec_motion_gate(None, 0, None, 1, None, None, 1, None, None, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


# ------------------------------------------------------------------------------------------------- motionref against a naive second implementation
def naive_update(frames, plane, cells, pixels, sp):
    """one frame over lists of lists, pixel by pixel: pixels[y][x] is (B, G, R) or a luma; plane and cells are changed in place; returns (the row,
    frames afterwards)"""
    c = 1 << sp.cell_log2
    for j in range(len(cells)):
        for i in range(len(cells[0])):
            cells[j][i] = 0
    total = 0
    for y in range(sp.h):
        for x in range(sp.w):
            p = pixels[y][x]
            luma = p if isinstance(p, int) else (29 * p[0] + 150 * p[1] + 77 * p[2] + 128) // 256
            cur, bg = luma * 256, plane[y][x]
            if frames == 0:
                plane[y][x] = cur
                continue
            dist = cur - bg if cur >= bg else bg - cur
            changed = dist > sp.threshold * 256
            k = sp.learn_shift_changed if changed else sp.learn_shift
            step = 0 if k == 16 else -(-dist // (1 << k))                             # dist / 2^k, rounded up
            plane[y][x] = bg + step if cur >= bg else bg - step
            if changed:
                cells[y // c][x // c] += 1
                total += 1
    act = [(i, j) for j in range(len(cells)) for i in range(len(cells[0])) if cells[j][i] >= sp.min_pixels]
    row = [frames - 2 ** 32 if frames >= 2 ** 31 else frames, total, len(act)]
    if act:
        row += [c * min(i for i, _ in act), c * min(j for _, j in act), min(c * (max(i for i, _ in act) + 1), sp.w) - 1, min(c * (max(j for _, j in act) + 1), sp.h) - 1]
    else:
        row += [0, 0, -1, -1]
    frames = (frames + 1) % 2 ** 32
    return row + [1 if frames > sp.warmup else 0] + [0] * 8, frames


def naive_f2i(v):
    v = float(F32(v))
    if v != v:
        return 0
    return 2 ** 31 - 1 if v >= 2.0 ** 31 else -2 ** 31 if v <= -2.0 ** 31 else int(v)


def naive_gate(boxes, frames, cells, sp):
    """one record, box by box and cell by cell: returns (the 8 words, { list index: (touched, active) }, the selected list indices)"""
    c = 1 << sp.cell_log2
    qual = [i for i, b in enumerate(boxes) if float(b["score"]) >= float(sp.min_score) and sp.allowed(b["type"])]
    dropped, qual = max(0, len(qual) - 128), qual[:128]
    warm = frames > sp.warmup
    per, sel, outside, nmoving = {}, [], 0, 0
    for i in qual:
        x1, y1, x2, y2 = (naive_f2i(boxes[i][f]) for f in ("x1", "y1", "x2", "y2"))
        touched = act = 0
        for j in range(len(cells)):
            for ii in range(len(cells[0])):
                # the cell's pixels inside the frame, the box and its own square
                lo_x, hi_x, lo_y, hi_y = max(ii * c, x1, 0), min(ii * c + c - 1, x2, sp.w - 1), max(j * c, y1, 0), min(j * c + c - 1, y2, sp.h - 1)
                if x1 <= x2 and y1 <= y2 and lo_x <= hi_x and lo_y <= hi_y:
                    touched += 1
                    act += cells[j][ii] >= sp.min_pixels
        outside += touched == 0
        moving = not warm or (touched >= 1 and act * 256 >= sp.cover * touched)
        nmoving += moving
        per[i] = (touched, act)
        if moving != sp.invert:
            sel.append(i)
    return [len(qual), dropped, outside, nmoving, int(warm), frames - 2 ** 32 if frames >= 2 ** 31 else frames, 0, 0], per, sel


NAIVE_UPDATES = [(fmt, name) for fmt in fuzzcases.FORMATS for name in ("1x1", "7x5 cell 8", "17x9", "67x35 odd", "wrap", "threshold edge", "learn 0", "learn 1 converges",
                                                                        "learn 15", "learn 16", "freeze changed", "skipped", "3 streams x 4", "junk frames 0")]


@pytest.mark.parametrize("fmt,name", NAIVE_UPDATES)
def test_motionref_update_equals_the_naive_one(fmt, name):
    """the seeded case replayed pixel by pixel from the state it starts with: rows, planes, cells and frames equal motionref's"""
    c = fuzzcases.update_cases(fmt)[name]
    sp, st0 = c.spec, c.state0
    frames = [int(v) for v in st0.hdr[:, 0]]
    planes = [[[int(v) for v in r] for r in st0.plane[s]] for s in range(c.nstreams)]
    cells = [[[int(v) for v in r] for r in st0.cells[s]] for s in range(c.nstreams)]
    arena = c.start
    for t, s in enumerate(c.streams):
        d = c.desc[t]
        if s < 0 or d is None:
            assert c.rows[t].tolist() == [0] * 16
            continue
        if fmt == "bgr":
            off, w, h, pitch = d
            pix = [[tuple(int(v) for v in arena[off + y * pitch + 3 * x:off + y * pitch + 3 * x + 3]) for x in range(w)] for y in range(h)]
        else:
            off, _, w, h, pitch, _ = d
            pix = [[int(arena[off + y * pitch + x]) for x in range(w)] for y in range(h)]
        row, frames[s] = naive_update(frames[s], planes[s], cells[s], pix, sp)
        assert c.rows[t].tolist() == row, (t, c.rows[t].tolist(), row)
    for s in range(c.nstreams):
        assert int(c.state.hdr[s, 0]) == frames[s] and c.state.plane[s].tolist() == planes[s] and c.state.cells[s].tolist() == cells[s], s
    assert c.state.raw[:, 4:16].tobytes() == st0.raw[:, 4:16].tobytes()                # the reserved words stay


@pytest.mark.parametrize("name", fuzzcases.GATE_NAMES)
def test_motionref_gate_equals_the_naive_one(name):
    c = fuzzcases.gate_cases()[name]
    sp, S = c.spec, c.stride
    for t, s in enumerate(c.streams):
        if s < 0:
            assert not c.words[t].any() and (c.out_recs is None or not np.frombuffer(c.out_recs[t].tobytes(), np.uint8).any())
            continue
        r = c.recs[t]
        if c.flat is None:
            boxes = r["box"][:max(0, min(int(r["count"]), S))]
        else:
            f0 = c.first[t] if c.first is not None else t * S
            boxes = c.flat[f0:f0 + max(0, min(int(r["nfull"]), S))]
        head, per, sel = naive_gate(boxes, int(c.state.hdr[s, 0]), [[int(v) for v in row] for row in c.state.cells[s]], sp)
        assert c.words[t, :8].tolist() == head, (t, c.words[t, :8].tolist(), head)
        for i in range(S):
            assert tuple(c.words[t, 8 + 2 * i:10 + 2 * i].tolist()) == per.get(i, (0, 0)), (t, i)
        if c.out_recs is not None:
            o = c.out_recs[t]
            assert (int(o["count"]), int(o["ncand"]), int(o["overflow"]), int(o["nfull"])) == (min(len(sel), 128), int(r["ncand"]), (int(r["overflow"]) & 1) | (4 if len(sel) > 128 else 0), len(sel))
            assert o["box"][:min(len(sel), 128)].tobytes() == boxes[sel[:128]].tobytes() and not np.frombuffer(o["box"][min(len(sel), 128):].tobytes(), np.uint8).any()
        if c.out_lists is not None:
            assert c.out_lists[t, :len(sel)].tobytes() == boxes[sel].tobytes() and not np.frombuffer(c.out_lists[t, len(sel):].tobytes(), np.uint8).any()


# ------------------------------------------------------------------------------------------------- properties by name
def test_the_model_reaches_the_frame_exactly():
    """rounding up: from any background, 17 frames of one picture at learn_shift 1 leave bg == cur everywhere; at 16 nothing moves; at 0 one frame does it"""
    rng = np.random.default_rng(8500)
    luma = rng.integers(0, 256, (6, 9))
    for k, n, reached in ((1, 17, True), (0, 1, True), (16, 5, False), (15, 3, False)):
        sp = motionref.Spec(9, 6, 2, 255, k, k)
        st = motionref.State(1, 9, 6, 2)
        st.plane[0][:] = rng.integers(0, 65536, (6, 9))
        st.hdr[0, 0] = 1
        before = st.plane[0].copy()
        for _ in range(n):
            motionref.update_frame(luma, sp, st.hdr[0], st.plane[0], st.cells[0])
        assert (st.plane[0].astype(np.int64) == luma << 8).all() == reached, k
        if k == 16:
            assert st.plane[0].tobytes() == before.tobytes()


def test_threshold_is_exclusive():
    c = fuzzcases.update_cases("nv12")["threshold edge"]
    assert c.trace["at_threshold"] == 168 and c.trace["one_above"] == 48 == c.trace["changed"] and int(c.rows[0, 1]) == 48


# ------------------------------------------------------------------------------------------------- the fuzz is not vacuous
@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_update_cases_are_not_vacuous(fmt):
    cases = fuzzcases.update_cases(fmt)
    assert tuple(cases) == fuzzcases.UPDATE_NAMES
    for name, c in cases.items():
        t = c.trace
        assert c.want.tobytes() != c.start.tobytes(), name
        assert t.get("changed", 0) >= 1 and t.get("unchanged", 0) >= 1, (name, t)
        if c.spec.gw * c.spec.gh >= 2:
            assert t.get("active_cells", 0) >= 1 and t.get("inactive_cells", 0) >= 1, (name, t)
    assert sorted({c.spec.cell_log2 for c in cases.values()}) == [2, 3, 4, 5, 6]
    assert {(c.spec.w, c.spec.h) for c in cases.values()} >= {(1, 1), (7, 5), (17, 9), (67, 35), (63, 65), (64, 64), (65, 63)}
    assert cases["67x35 odd"].desc[0][0] % 2 == 1 and cases["learn 1 converges"].trace["reached_cur"] >= 100 and cases["freeze changed"].trace["frozen_changed"] >= 100
    assert cases["threshold edge"].trace["at_threshold"] >= 10 and cases["threshold edge"].trace["one_above"] >= 10
    assert cases["learn 1 converges"].n == 18 and (cases["learn 1 converges"].state.plane[0].astype(np.int64) == cases["learn 1 converges"].lumas[0] << 8).all()
    assert int(cases["wrap"].rows[0, 0]) == -1 and int(cases["wrap"].rows[1, 0]) == 0 and int(cases["wrap"].rows[1, 1]) == 0 and int(cases["wrap"].rows[0, 7]) == 0
    assert cases["targets 65"].n == 65 and cases["targets 130"].n == 130 and -1 in cases["skipped"].streams and None in cases["skipped"].desc


def test_gate_cases_are_not_vacuous():
    cases = fuzzcases.gate_cases()
    assert tuple(cases) == fuzzcases.GATE_NAMES
    moving = still = 0
    for name, c in cases.items():
        t = c.trace
        moving, still = moving + t.get("moving", 0), still + t.get("still", 0)
        assert c.want.tobytes() != c.start.tobytes(), name
        if name != "nan min_score":                                                    # (nothing qualifies there: that is the case)
            assert t.get("selected", 0) >= 1 and t.get("rejected", 0) >= 1, (name, t)
    assert not cases["nan min_score"].words[:, :4].any() and not cases["nan min_score"].words[:, 6:].any()
    assert moving >= (moving + still) / 10 and still >= (moving + still) / 10, (moving, still)
    t = cases["corners"].trace
    assert t["inverted"] >= 2 and t["beyond"] >= 2 and t["ends_on_boundary"] >= 1 and t["one_past_boundary"] >= 1
    assert int(cases["dropped"].words[0, 0]) == 128 and int(cases["dropped"].words[0, 1]) == 2 and int(cases["dropped"].out_recs[0]["nfull"]) > 0
    w = cases["warmth"].words
    assert w[:3, 4].tolist() == [0, 0, 1] and w[:3, 5].tolist() == [0, 6, 7] and (w[:2, 3] == w[:2, 0]).all() and int(w[2, 3]) < int(w[2, 0])
    assert cases["no outputs"].recs_off is None and cases["records only"].lists_off is None and cases["list_first"].first is not None and cases["own boxes"].flat is None
    assert cases["records 65"].n == 65 and cases["records 130"].n == 130 and int(cases["wide grid"].words[0, 8]) > 64
