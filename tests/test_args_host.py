"""ffcnn_amd/csrc/ffgpu_args.hpp -- the frame descriptors' checks and defaults, and where a post-pass finds its boxes (DetSource, its operator
and executor builders) -- on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C ffcnn_amd/csrc args`).  The driver
(san/args_driver.cc) runs a fixed table of cases and prints one line per case: id, return value, message, and for an accepted case what it resolved
to.  Every line is compared with a literal here.  The message formats below are the strings of the entry points as they stood before the checks were
gathered in one header (ffgpu_exec.hip, ffgpu_draw.inc, ffgpu_crop.inc, ffgpu_track.inc, ffgpu_feature.inc of that commit), copied: a call with one
bad argument reports what it always did, byte for byte.  A sanitizer report aborts the child: the test fails with it."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
BIN = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_args_san")

# the C format strings, `what` = "op"; NOUN is "frame" in the forward's messages and "target" in the draw's and the crop's
NULL_BGR = "op: frame %d: NULL bgr"
NULL_Y = "op: frame %d: NULL y"
BAD_SIZE = "op: NOUN %d: bad size %d x %d"
RESERVED = "op: NOUN %d: reserved must be 0"
PITCH = "op: NOUN %d: pitch %d is below 3 w = %d"
MATRIX = "op: NOUN %d: matrix %d is none of FFGPU_YUV_* (0..3)"
PITCH_Y = "op: NOUN %d: pitch_y %d is below w = %d"
PITCH_UV = "op: NOUN %d: pitch_uv %d is odd or below 2 ((w + 1) / 2) = %d"
UV_ODD = "op: NOUN %d: the uv plane's address %s is odd (U V pairs are VERB as aligned 16-bit values)"
NULL_RECORDS = "op: NULL records"
BAD_STRIDE = "op: bad list_stride %d"
NEG_START = "op: target %d: negative list start %d"
WHICH = "op: which = %d is neither FFGPU_%s_ENTRIES nor FFGPU_%s_MERGED"
NO_MERGE = "op: no ffgpu_exec_merge_tiles has run on this executor"
COUNT_MERGED = "op: %d targets for a merge of %d pictures"
COUNT_ENTRIES = "op: %d targets for an executor of batch %d"

B = 0x10000000                                                   # the driver's made-up base address


def _ok(p0, p1, w, h, pitch, pitch_uv, fmt):
    return "0 p0=%x p1=%x w=%d h=%d pitch=%d pitch_uv=%d fmt=%d" % (p0, p1, w, h, pitch, pitch_uv, fmt)


def _frames(role):
    fwd = role == "fwd"
    noun, verb = ("frame", "read") if fwd else ("target", "written")

    def no(fmt, *a):
        return "-1 " + (fmt % a).replace("NOUN", noun).replace("VERB", verb)
    bgr = [
        ("null", no(NULL_BGR, 0) if fwd else _ok(0, 0, 64, 48, 192, 0, 0)),            # an error for the forward, a skipped target for the draw
        ("null_badsize", no(NULL_BGR, 1) if fwd else no(BAD_SIZE, 1, 0, 48)),          # the forward asks for the address first
        ("w0", no(BAD_SIZE, 2, 0, 48)),
        ("hneg", no(BAD_SIZE, 3, 64, -1)),
        ("reserved", no(RESERVED, 4)),
        ("pitch_default", _ok(B, 0, 63, 48, 192, 0, 0)),                               # ALIGN(3 w, 4)
        ("pitch_3w", _ok(B, 0, 63, 48, 189, 0, 0)),
        ("pitch_3w_less_1", no(PITCH, 7, 188, 189)),
        ("pitch_negative", no(PITCH, 8, -4, 189)),
        ("w_max", _ok(B, 0, 0x2aaaaaaa, 1, 0x7ffffffe, 0, 0)),                         # 3 w = 2^31 - 2
        ("w_max_plus_1", no(BAD_SIZE, 10, 0x2aaaaaab, 1)),
        ("w_max_pitch_default", no(PITCH, 10, 0, 0x7ffffffe)),                         # ALIGN(3 w, 4) = 2^31 is no int
        ("h_3fffffff", _ok(B, 0, 1, 0x3fffffff, 4, 0, 0)),
        ("h_40000000", _ok(B, 0, 1, 0x40000000, 4, 0, 0) if fwd else no(BAD_SIZE, 12, 1, 0x40000000)),   # the forward's table has no bound on a BGR height
        ("h_7fffffff", _ok(B, 0, 1, 0x7fffffff, 4, 0, 0) if fwd else no(BAD_SIZE, 13, 1, 0x7fffffff)),
    ]
    nv12 = [
        ("null", no(NULL_Y, 0) if fwd else _ok(0, 0, 64, 48, 64, 64, 1)),
        ("null_badmatrix", no(NULL_Y, 1) if fwd else no(MATRIX, 1, 4)),                # a skip only after every other field has passed
        ("w0", no(BAD_SIZE, 2, 0, 48)),
        ("w_40000000", no(BAD_SIZE, 3, 0x40000000, 2)),
        ("h_40000000", no(BAD_SIZE, 4, 2, 0x40000000)),
        ("reserved", no(RESERVED, 5)),
        ("matrix_neg", no(MATRIX, 6, -1)),
        ("matrix_4", no(MATRIX, 7, 4)),
        ("pitch_y_low", no(PITCH_Y, 8, 63, 64)),
        ("pitch_uv_low", no(PITCH_UV, 9, 62, 64)),
        ("pitch_uv_odd", no(PITCH_UV, 10, 65, 64)),
        ("pitch_uv_even", _ok(B, B + 63 * 48, 63, 48, 63, 66, 4)),
        ("defaults", _ok(B, B + 63 * 48, 63, 48, 63, 64, 3)),                          # pitch_y = w, pitch_uv = 2 ((w + 1) / 2), uv = y + pitch_y h
        ("pitches_given", _ok(B, B + 80 * 48, 64, 48, 80, 96, 2)),
        ("uv_given", _ok(B, 3 * B, 64, 48, 64, 64, 1)),
        ("uv_odd", no(UV_ODD, 15, "0x10001001")),
        ("uv_default_odd", no(UV_ODD, 16, "0x%x" % (B + 65 * 47))),
        ("w_3fffffff", _ok(B, B, 0x3fffffff, 1, 0x3fffffff, 0x40000000, 1)),           # odd w: min_uv = 2^30
    ]
    return ["%s.bgr.%s %s" % (role, n, v) for n, v in bgr] + ["%s.nv12.%s %s" % (role, n, v) for n, v in nv12]


def _src(lists, stride, longest, first):
    return "0 lists=%d stride=%d longest=%d first=%s" % (lists, stride, longest, ",".join(str(x) for x in first))


WANT = _frames("fwd") + _frames("draw") + [
    "dev.null_records -1 " + NULL_RECORDS,
    "dev.first_null " + _src(1, 100, 100, (0, 100, 200, 300)),                         # t x stride
    "dev.first_given " + _src(1, 100, 100, (7, 0, 300, 12)),
    "dev.first_negative -1 " + NEG_START % (2, -5),                                    # the first of two negative entries
    "dev.no_lists " + _src(0, 128, 128, (0, 0, 0, 0)),                                 # FFGPU_MAX_DET; list_first is not looked at
    "dev.stride_0 -1 " + BAD_STRIDE % 0,
    "dev.stride_2p24 " + _src(1, 1 << 24, 1 << 24, (0, 1 << 24)),
    "dev.stride_2p24_plus_1 -1 " + BAD_STRIDE % ((1 << 24) + 1),
    "stride.no_lists 128 ",
    "stride.lists 1500 ",
    "stride.bad -1 " + BAD_STRIDE % -3,
    "exec.entries " + _src(0, 0, 1500, (0, 1500, 3000)),
    "exec.merged " + _src(0, 0, 3 * 1500, (0, 2 * 1500, 2 * 1500)),                    # offsets { 0, 2, 2, 5 }: a picture with no tile in between
] + ["exec.which_2.%s -1 " % f + WHICH % (2, f, f) for f in ("DRAW", "CROP", "TRACK", "RELABEL")] + [
    "exec.which_neg -1 " + WHICH % (-1, "TRACK", "TRACK"),
    "exec.merged_no_merge -1 " + NO_MERGE,
    "exec.merged_empty -1 " + NO_MERGE,
    "exec.count_entries -1 " + COUNT_ENTRIES % (4, 3),
    "exec.count_merged -1 " + COUNT_MERGED % (5, 3),
    "exec.past_2p31 " + _src(0, 0, 2 * 0x7fffffff, (0, 0x7fffffff)),                   # cand_cap x tiles as a long long, UBSan silent
]


@pytest.fixture(scope="module")
def lines():
    subprocess.check_call(["make", "-s", "-C", CSRC, "args"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    return r.stdout.decode().split("\n")[:-1]


def test_every_case_line_for_line(lines):
    assert len(lines) == len(WANT) == 2 * 33 + 23
    for got, want in zip(lines, WANT):
        assert got == want


def test_the_roles_differ_only_where_they_did(lines):
    """forward and draw: the same line but for the noun and the verb, except the four differences the roles carry: a NULL address (error / skip),
    which of a NULL address and another bad field is reported, and the BGR height bound"""
    fwd = {s.split(" ", 1)[0][4:]: s.split(" ", 1)[1] for s in lines if s.startswith("fwd.")}
    draw = {s.split(" ", 1)[0][5:]: s.split(" ", 1)[1] for s in lines if s.startswith("draw.")}
    assert fwd.keys() == draw.keys() and len(fwd) == 33
    differ = {k for k in fwd if fwd[k].replace(" frame ", " target ").replace(" read ", " written ") != draw[k]}
    assert differ == {"bgr.null", "bgr.null_badsize", "nv12.null", "nv12.null_badmatrix", "bgr.h_40000000", "bgr.h_7fffffff"}
