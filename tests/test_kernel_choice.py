"""Census of the convolution dispatcher's choices, without a GPU: for about 1 300 geometries the kernel AUTO takes, what each explicit
FFGPU_K_* id answers for the shape ("unsupported" included, which pins every *_ok), and what AUTO takes under each environment switch that
removes a kernel from its list.  ffgpu_groupconv_kernel_name is pure host code.  The expected answers are tests/golden/kernel_choice.json,
recorded once (`python tests/test_kernel_choice.py --write`) from the commit named in the file's "recorded_at"; a refactor of the dispatcher
must leave every one of them as it is, so the file is not regenerated with the code under test.

Fixture layout: "names" is the name table, "columns" the 20 questions asked per geometry, "cases" one row per geometry:
N, W, H, ic, groups, pad, stride, fs, oc, and a 20-character string whose i-th character is the base-36 index into "names" of column i's answer."""
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_choice.json")
AUTO_NAMES = ["conv_generic", "dw3_stream", "dw_lds", "pw_mfma", "pw_gemm", "pw_x3t", "pw_x3s", "conv_x3", "conv_dense8", "conv_igemm", "conv_thin"]
NAMES = AUTO_NAMES + ["pw_x3", "pw_bf16", "unsupported"]
EXPLICIT = [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13]            # the twelve FFGPU_K_* ids (include/ffcnn_hip.h; 6 was never assigned)
SWITCHES = [{"FFGPU_IG_X3": "0"}, {"FFGPU_PW_X3T": "0"}, {"FFGPU_PW_X3S": "0"}, {"FFGPU_PW_X3T": "0", "FFGPU_PW_X3S": "0"},
            {"FFGPU_NO_PW_GEMM": "1"}, {"FFGPU_NO_IGEMM": "1"}, {"FFGPU_NO_GROUP_THIN": "1"}]
COLUMNS = ["auto"] + ["k%d" % k for k in EXPLICIT] + [",".join("%s=%s" % kv for kv in sorted(sw.items())) for sw in SWITCHES]
FLOOR = 10
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"


def geometries():
    """(N, W, H, ic, groups, pad, stride, fs, oc), seeded; stratified so that every AUTO name has its share: a uniform grid gives pw_gemm and pw_x3t once each"""
    r = random.Random(20)
    out = []

    def add(N, W, H, ic, g, pad, stride, fs, oc):
        if ic % g or oc % g or W + 2 * pad < fs or H + 2 * pad < fs:
            return
        t = (N, W, H, ic, g, pad, stride, fs, oc)
        if t not in out:
            out.append(t)

    # the shapes the packed-image test of tests/test_gpu_kernels.py runs
    for t in [(1, 8, 8, 8, 1, 0, 1, 1, 16), (2, 10, 10, 12, 1, 0, 1, 1, 40), (1, 128, 128, 64, 1, 0, 1, 1, 128), (1, 256, 256, 128, 1, 0, 1, 1, 192),
              (1, 64, 128, 96, 1, 0, 1, 1, 64), (2, 104, 104, 16, 1, 1, 1, 3, 64), (4, 208, 208, 16, 1, 1, 2, 3, 64), (1, 13, 13, 256, 1, 1, 1, 3, 512),
              (2, 16, 16, 32, 2, 1, 1, 3, 32)]:
        add(*t)
    # anything: odd planes, every filter size, grouped, strided
    for _ in range(420):
        fs = r.choice([1, 1, 2, 3, 3, 5, 7])
        ic = r.choice([1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 120])
        g = r.choice([1, 1, 1, 2, 4, ic])
        oc = r.choice([1, 2, 3, 4, 8, 16, 24, 40, 64, 96, 128, 255]) if g == 1 else g * r.choice([1, 2, 3, 8])
        add(r.choice([1, 2, 3, 4, 8]), r.randint(1, 70), r.randint(1, 70), ic, g, r.choice([0, fs // 2]), r.choice([1, 1, 2]), fs, oc)
    # pointwise layers around the thresholds of pw_gemm, pw_x3s, pw_x3t and pw_x3: ic near 64 / 96 / 128 / 192, oc near 64 / 128 / 192 / 256, P near 16 384 / 65 536
    for _ in range(420):
        ic = r.choice([56, 63, 64, 65, 72, 88, 95, 96, 97, 104, 120, 127, 128, 129, 136, 184, 191, 192, 193, 200, 256])
        oc = r.choice([48, 63, 64, 65, 120, 127, 128, 129, 191, 192, 193, 247, 248, 255, 256, 257, 512])
        N, W, H = r.choice([(1, 64, 64), (1, 128, 127), (1, 128, 128), (1, 129, 128), (2, 128, 64), (1, 256, 255), (1, 256, 256), (1, 257, 256), (4, 128, 128),
                            (3, 127, 43), (1, 20, 20), (64, 20, 20), (256, 20, 20), (2, 256, 256)])
        add(N, W, H, ic, 1, 0, 1, 1, oc)
    for _ in range(40):                     # ... pw_x3's own corner (what is left to it once pw_x3t and pw_x3s are switched off)
        add(*r.choice([(1, 256, 255), (1, 256, 256), (4, 128, 128), (2, 256, 256)]), r.choice([184, 191, 192, 193, 200, 256]), 1, 0, 1, 1, r.choice([248, 255, 256, 257, 512]))
    # depthwise: the streaming kernel's width window (40 .. 512, whole quads), the LDS kernel's 3x3 / 5x5 at both strides, 7x7 for the generic one
    for _ in range(130):
        fs = r.choice([3, 3, 3, 5, 5, 7])
        c = r.choice([2, 8, 24, 96, 120])
        add(r.choice([1, 2, 4]), r.choice([6, 10, 20, 36, 39, 40, 42, 44, 64, 160, 512, 516, 1030]), r.choice([1, 2, 10, 20, 40, 64]), c, c, r.choice([0, fs // 2]),
            r.choice([1, 1, 2]), fs, c)
    for _ in range(70):                     # ... the streaming kernel's own form (3x3, stride 1, pad 1) on both sides of each of its limits
        c = r.choice([1, 8, 24, 96])
        add(r.choice([1, 2, 64]), r.choice([36, 38, 40, 41, 44, 64, 80, 160, 320, 508, 512, 516]), r.choice([1, 2, 3, 20, 64]), c, c, 1, 1, 3, c)
    # dense 3x3 / 5x5: the first-layer kernel (<= 8 channels), conv_x3 against conv_igemm (whole blocks of 8 channels, enough workgroups), stride 2
    for _ in range(220):
        fs = r.choice([3, 3, 3, 5])
        add(r.choice([1, 2, 4, 16]), *r.choice([(13, 13), (26, 26), (52, 52), (104, 104), (208, 208), (50, 38), (3, 3)]), r.choice([3, 8, 9, 12, 16, 24, 32, 64, 256]), 1,
            r.choice([0, fs // 2, fs // 2]), r.choice([1, 1, 2]), fs, r.choice([8, 16, 32, 64, 100, 128, 512]))
    # groups: 2 .. 7 channels per group for the thin kernel, 8 and more for the implicit GEMM (up to 16 groups), one per group and 32 groups for the generic one
    for _ in range(160):
        g = r.choice([2, 3, 4, 8, 16, 17, 32])
        fs = r.choice([1, 3, 3, 5, 11, 12])
        add(r.choice([1, 2]), r.randint(4, 40), r.randint(4, 40), g * r.choice([1, 2, 3, 4, 7, 8, 9, 16]), g, r.choice([0, fs // 2]), r.choice([1, 2]), fs, g * r.choice([1, 2, 5, 8, 70]))
    return out


def census(capi, geoms, setenv, delenv):
    """one string of len(COLUMNS) name indices per geometry"""
    for k in capi.knobs():                  # every variable the library reads (its own table): a developer's shell must not change the census
        delenv(k["name"])
    cols = [[capi.kernel_name(*t)for t in geoms]]
    for k in EXPLICIT:
        cols.append([capi.kernel_name(*t, variant=k) for t in geoms])
    for sw in SWITCHES:
        for kv in sw.items():
            setenv(*kv)
        cols.append([capi.kernel_name(*t) for t in geoms])
        for v in sw:
            delenv(v)
    return ["".join(DIGITS[NAMES.index(c[i])] for c in cols) for i in range(len(geoms))]


def write(recorded_at):
    from ffcnn_amd import capi
    capi.build_library()
    geoms = geometries()
    rows = census(capi, geoms, os.environ.__setitem__, lambda v: os.environ.pop(v, None))
    with open(FIXTURE, "w") as f:
        f.write('{"recorded_at": %s,\n "names": %s,\n "columns": %s,\n "cases": [\n' % (json.dumps(recorded_at), json.dumps(NAMES), json.dumps(COLUMNS)))
        f.write(",\n".join(json.dumps(list(t) + [row], separators=(",", ":")) for t, row in zip(geoms, rows)))
        f.write("\n]}\n")
    print("%d geometries, %d bytes" % (len(geoms), os.path.getsize(FIXTURE)))
    for n in AUTO_NAMES:
        print("%-13s %d" % (n, sum(row[0] == DIGITS[NAMES.index(n)] for row in rows)))


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_auto_kernel(golden):
    assert golden["names"] == NAMES and golden["columns"] == COLUMNS
    assert os.path.getsize(FIXTURE) < 100 * 1024
    auto = [golden["names"][DIGITS.index(c[9][0])] for c in golden["cases"]]
    for n in AUTO_NAMES:
        assert auto.count(n) >= FLOOR, (n, auto.count(n))
    under_both = [golden["names"][DIGITS.index(c[9][COLUMNS.index("FFGPU_PW_X3S=0,FFGPU_PW_X3T=0")])] for c in golden["cases"]]
    assert under_both.count("pw_x3") >= FLOOR


def test_kernel_choice_matches_fixture(capi, golden, monkeypatch):
    geoms = [tuple(c[:9]) for c in golden["cases"]]
    got = census(capi, geoms, monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    bad = [(t, [(COLUMNS[i], NAMES[DIGITS.index(w)], NAMES[DIGITS.index(g)]) for i, (w, g) in enumerate(zip(c[9], row)) if w != g])
           for t, c, row in zip(geoms, golden["cases"], got) if c[9] != row]
    assert not bad, "%d of %d geometries differ; the first: %s" % (len(bad), len(geoms), bad[:3])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if len(sys.argv) >= 2 and sys.argv[1] == "--write":         # (the commit the library is built from: HEAD unless named)
        import subprocess
        write(sys.argv[2] if len(sys.argv) > 2 else subprocess.check_output(["git", "-C", HERE, "rev-parse", "--short", "HEAD"], text=True).strip())
    else:
        sys.exit("usage: test_kernel_choice.py --write [commit]")
