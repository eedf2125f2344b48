"""Census of the fused-block planner, without a GPU: for about 400 blocks the line ffgpu_irb_plan_text writes -- family and instantiation, every scalar
of the parameter block the launch would pass, LDS bytes, grid, block, `half`, `pack_floats`, or "unsupported" -- by default, with FFGPU_CONCURRENT, and
under each of nine planner switches on its own.  The probe is pure host code.  The expected answers are tests/golden/irb_choice.json, recorded once
from a build of the commit its "recorded_at" names: the parent of the refactor that introduced IrbPlan, whose planner re-picked at every call.  The
refactor must leave every cell as it is, so the file is never regenerated with the code under test.

The parent had no probe.  The recorder was this patch on a scratch copy of it (not committed as code): a dry-run hook immediately in front of the kernel
dispatch of launch_irb_thin, launch_irbw and ffgpu_launch_irb, which formats what the parent's untouched arithmetic had just computed.

    ffgpu_conv_kernels.inc
      + char *g_irb_probe = nullptr; size_t g_irb_probe_cap = 0, g_irb_probe_pack = 0;
      launch_irb_thin, in front of `if (d.ic == 8 && d.oc == 4) return irb_thin_launch<8, 8, 4>(p, s);`
      + if (g_irb_probe) { snprintf(g_irb_probe, g_irb_probe_cap, "thin<%d,8,%d> W=%d H=%d N=%d band=%d nbands=%d act=%g,%g,%g,%g ntasks=%ld lds=0 grid=%u block=256 half=0 pack=%zu",
      +       d.ic, d.oc, p.W, p.H, p.N, p.band, p.nbands, p.act1, p.actd, p.act2, p.res_act, p.ntasks, (unsigned)((p.ntasks + 3) / 4), g_irb_probe_pack); return 0; }
      launch_irbw, in front of `if (c.NSO == 2) {`
      + if (g_irb_probe) { char key[48];
      +     if (c.NSO == 2) snprintf(key, sizeof key, "irbw2<%d,3%s>", c.KS1, c.x3 ? ",x3" : "");
      +     else snprintf(key, sizeof key, "irbw<%d,%d,%d,%d%s%s%s>", c.KS1, c.OT, d.stride, c.NSI, c.big ? ",big" : "", c.x3 ? ",x3" : "", c.xl ? ",xl" : "");
      +     snprintf(g_irb_probe, g_irb_probe_cap, "%s N=%d H=%d W=%d OH=%d OW=%d ic=%d ec=%d oc=%d act=%g,%g,%g,%g tile=%d,%d,%d,%d tiles=%d,%d,%ld ngroups=%d G=%d WPB=%d o_w2=%d o_cs=%d cs_floats=%d "
      +         "xl_off=%d red_cap=%d in_elems=%u vec=%d half_last=%d m=%u,%u,%u,%u xcd=%d lds=%zu grid=%ld block=%d half=%d pack=%zu",
      +         key, p.N, p.H, p.W, p.OH, p.OW, p.ic, p.ec, p.oc, p.act1, p.actd, p.act2, p.res_act, p.TWq, p.TH, p.EW, p.EH, p.tiles_x, p.tiles_y, p.ntiles, p.ngroups, p.G, p.WPB,
      +         p.o_w2, p.o_cs, p.cs_floats, p.xl_off, p.red_cap, p.in_elems, p.vec, p.half_last, p.m_ew, p.m_tx, p.m_ty, p.m_twq, p.xcd, lds, nblocks, waves * 64, p.half_last, g_irb_probe_pack);
      +     return 0; }
      ffgpu_launch_irb, in front of `#define IRB_CASE`
      + if (g_irb_probe) { snprintf(g_irb_probe, g_irb_probe_cap, "irb<%d,%d,%d,%d,%d> N=%d H=%d W=%d OH=%d OW=%d ic=%d ec=%d oc=%d stride=%d act=%g,%g,%g,%g tile=%d,%d,%d,%d,%d,%d NPin=%d NPout=%d tiles=%d,%d,%d "
      +         "k4=%d nchunks=%d ECH=%d CH=%d KS=%d red_off=%d vec_store=%d resident=%d inv_nsi=%d lds=%zu grid=%ld block=%d half=0 pack=%zu",
      +         MT, OT, d.stride, NW == 8 ? 1 : 2, NW, p.N, p.H, p.W, p.OH, p.OW, p.ic, p.ec, p.oc, p.stride, p.act1, p.actd, p.act2, p.res_act, p.TH, p.TW, p.TWq, p.NF, p.EH, p.EW,
      +         p.NPin, p.NPout, p.tiles_x, p.tiles_y, p.ntiles, p.k4, p.nchunks, p.ECH, p.CH, p.KS, p.red_off, p.vec_store, p.resident, p.inv_nsi, lds, nblocks, NW * 64, g_irb_probe_pack);
      +     return 0; }
    ffgpu_exec.hip
      + extern char *g_irb_probe; extern size_t g_irb_probe_cap, g_irb_probe_pack;
      + extern "C" int ffgpu_irb_plan_text(int batch, int iw, int ih, int ic, int ec, int oc, int stride, int act1, int actd, int act2, int res_act, int flags, char *buf, int cap)
      + {
      +     IrbDesc d{};                                      // filled as ffgpu_irb_dev fills it, plus d.flags = flags & FFGPU_CONCURRENT
      +     ...
      +     if (!ffgpu_irb_supported(d)) return snprintf(buf, cap, "unsupported");
      +     d.pk = reinterpret_cast<const float *>(16);       // never read on the host
      +     g_irb_probe = buf; g_irb_probe_cap = cap; g_irb_probe_pack = ffgpu_irb_pack_floats(d);
      +     buf[0] = 0;
      +     const int rc = ffgpu_launch_irb(d, nullptr);      // the hooks return in front of the dispatch
      +     g_irb_probe = nullptr;
      +     return rc ? snprintf(buf, cap, "launch-error") : (int)strlen(buf);
      + }

("launch-error" -- a block the parent's planner claimed and its launch then refused -- was recorded for no cell.)

Fixture layout: "keys" is the table of instantiation keys, "columns" the 11 questions, "cases" one row per block: N, W, H, ic, ec, oc, stride, act1, actd,
act2, res_act, then a string of two base-36 digits per column (the index into "keys" of that column's answer) and a string of eight hex digits per column
(the CRC-32 of the full line)."""
import ctypes
import json
import os
import random
import sys
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "irb_choice.json")
CONCURRENT = 64                                                # FFGPU_CONCURRENT (include/ffcnn_hip.h)
SWITCHES = [("FFGPU_NO_IRBW", "1"), ("FFGPU_NO_THIN", "1"), ("FFGPU_IRBW_X3", "0"), ("FFGPU_IRBW_NSO", "1"), ("FFGPU_IRBW_HALF", "0"), ("FFGPU_IRBW_G", "1"),
            ("FFGPU_IRBW_S2_NSI4", "1"), ("FFGPU_IRBW_S2_633", "0"), ("FFGPU_IRB_ECH", "32")]
COLUMNS = ["default", "flags=FFGPU_CONCURRENT"] + ["%s=%s" % kv for kv in SWITCHES]
FLOOR = 10
# The instantiations a switch-free or single-switch run can reach (of 4 thin, 33 wave and 24 workgroup ones):
#  - k_irbw, fp32 expand: `big` follows from the shape (registers = 4 NSI KS1 + 16 OT + 2 (KS1 + 4 OT) + 76 > 124) unless FFGPU_IRBW_BIG forces it, so one of
#    each shape's two register budgets; <6,2,1,2,big> and <4,2,2,4,big> only with FFGPU_IRBW_X3=0, the two <.,1,2,4> only with FFGPU_IRBW_S2_NSI4=1
#  - the three split-bf16 ones and three of the four two-strip ones (fp32 expand: FFGPU_IRBW_X3=0; <2,3,x3> needs bit 0 of FFGPU_IRBW_X3, which the default 30 has not)
#  - k_irb with eight waves (four: FFGPU_IRB_NW, not a column): MT 1 / 2 x OT 1 / 2 / 3 x both strides
REACHABLE = (["thin<%d,8,%d>" % t for t in ((8, 4), (4, 4), (8, 8), (4, 8))] +
             ["irbw<1,1,1,2>", "irbw<2,1,1,2>", "irbw<4,1,1,2,big>", "irbw<2,2,1,2,big>", "irbw<4,2,1,2,big>", "irbw<6,2,1,2,big>", "irbw<12,3,1,2,big>",
              "irbw<1,1,2,3>", "irbw<2,1,2,3,big>", "irbw<4,2,2,4,big>", "irbw<6,3,2,3,big>", "irbw<1,1,2,4>", "irbw<2,1,2,4,big>",
              "irbw<6,2,1,2,big,x3>", "irbw<4,2,2,4,big,x3>", "irbw<12,3,1,2,big,x3,xl>", "irbw2<2,3>", "irbw2<4,3>", "irbw2<4,3,x3>"] +
             ["irb<%d,%d,%d,1,8>" % (mt, ot, s) for mt in (1, 2) for ot in (1, 2, 3) for s in (1, 2)])


def family(key):
    if key == "unsupported":
        return key
    if key.startswith("thin<"):
        return "thin"
    if key.startswith("irbw2<"):
        return "two-strip"
    if key.startswith("irb<"):
        return "workgroup"
    return "XL" if ",xl" in key else ("wave X3" if ",x3" in key else "wave fp32")


FAMILIES = ["thin", "wave fp32", "wave X3", "XL", "two-strip", "workgroup", "unsupported"]


def geometries():
    """(N, W, H, ic, ec, oc, stride, act1, actd, act2, res_act), seeded"""
    r = random.Random(21)
    out = []

    def add(N, W, H, ic, ec, oc, stride, acts=(2, 2, 0, 0)):
        t = (N, W, H, ic, ec, oc, stride) + tuple(acts)
        if t not in out:
            out.append(t)

    # the fused blocks of yolo-fastest (distinct shapes) at batches 1, 4, 64 and 256
    for N in (1, 4, 64, 256):
        for ic, ec, oc, stride, P in [(8, 8, 4, 1, 160), (4, 8, 4, 1, 160), (4, 24, 8, 2, 160), (8, 32, 8, 1, 80), (8, 32, 8, 2, 80), (8, 48, 8, 1, 40), (8, 48, 16, 1, 40),
                                      (16, 96, 16, 1, 40), (16, 96, 24, 2, 40), (24, 136, 24, 1, 20), (24, 136, 48, 2, 20), (48, 224, 48, 1, 10)]:
            add(N, P, P, ic, ec, oc, stride)
    # IRB_SHAPES and the shapes of the other test_irb_* tests (tests/test_gpu_kernels.py), the split-expand and Inf tests of rounds 4 and 5: (ic, ec, oc, stride, N, H, W)
    for ic, ec, oc, stride, N, H, W in [(8, 32, 8, 1, 2, 80, 80), (4, 24, 8, 2, 2, 160, 160), (8, 48, 16, 1, 3, 40, 40), (16, 96, 16, 1, 2, 40, 40), (16, 96, 24, 2, 2, 40, 40),
                                        (24, 136, 24, 1, 3, 20, 20), (24, 136, 48, 2, 2, 20, 20), (48, 224, 48, 1, 3, 10, 10), (8, 8, 4, 1, 1, 32, 48), (4, 8, 4, 1, 2, 16, 16),
                                        (12, 40, 20, 1, 1, 12, 20), (6, 30, 10, 2, 2, 16, 12), (8, 32, 8, 1, 2, 13, 11), (16, 50, 30, 1, 1, 9, 22), (3, 20, 5, 2, 3, 21, 17),
                                        (8, 64, 16, 2, 1, 30, 26), (8, 8, 4, 1, 2, 37, 160), (4, 8, 4, 1, 3, 21, 48), (8, 8, 8, 1, 1, 16, 256), (4, 8, 8, 1, 2, 9, 4),
                                        (4, 8, 4, 1, 1, 1, 8), (8, 8, 4, 1, 2, 2, 12), (5, 20, 7, 1, 1, 23, 30), (8, 32, 8, 1, 7, 80, 80), (16, 96, 16, 1, 5, 40, 40),
                                        (24, 136, 24, 1, 11, 20, 20), (48, 224, 48, 1, 13, 10, 10), (4, 24, 8, 2, 3, 160, 160), (16, 96, 24, 2, 9, 40, 40),
                                        (48, 224, 48, 1, 2, 10, 10), (8, 48, 16, 1, 2, 40, 40), (4, 24, 8, 2, 2, 48, 32), (24, 136, 24, 1, 2, 20, 20),
                                        (16, 96, 16, 1, 24, 40, 40), (24, 136, 24, 1, 24, 20, 20), (48, 224, 48, 1, 24, 10, 10), (8, 48, 8, 1, 24, 40, 40), (8, 32, 8, 1, 8, 80, 80)]:
        add(N, W, H, ic, ec, oc, stride)
    # every (input-channel quads, output tiles, stride) the wave kernels are instantiated for, on planes of whole quads and others, at small and large batches
    for ks1, ot, stride in [(1, 1, 1), (2, 1, 1), (4, 1, 1), (2, 2, 1), (4, 2, 1), (6, 2, 1), (12, 3, 1), (1, 1, 2), (2, 1, 2), (4, 2, 2), (6, 3, 2)]:
        for _ in range(9):
            W, H = r.choice([(10, 10), (20, 20), (40, 40), (80, 80), (160, 160), (19, 23), (41, 37), (7, 5)])
            add(r.choice([1, 2, 4, 64, 256]), W, H, r.randint(4 * ks1 - 3, 4 * ks1), r.randint(8, 256), r.randint(16 * ot - 15, 16 * ot), stride)
    # the thin blocks' four channel pairs, widths of whole quads up to 256, any height
    for _ in range(24):
        add(r.choice([1, 2, 4, 64, 256]), 4 * r.randint(1, 40), r.randint(1, 160), r.choice([4, 8]), 8, r.choice([4, 8]), 1)
    # anything: planes 1..160 including odd sizes and sizes that are not whole quads, a few with the activation no fused kernel has (3) or a ReLU (1)
    for _ in range(185):
        acts = (2, 2, 0, 0) if r.random() < 0.85 else (r.choice([0, 1, 2, 3]), r.choice([1, 2]), r.choice([0, 2]), r.choice([0, 0, 1, 3]))
        add(r.choice([1, 2, 3, 4, 8, 64, 256]), r.randint(1, 160), r.randint(1, 160), r.randint(3, 64), r.randint(8, 256), r.randint(4, 48), r.choice([1, 2]), acts)
    # k_irb's 16-channel chunks under three output tiles: stride 1, planes 32..63 wide, at most 48 expanded channels
    for _ in range(8):
        P = r.choice([32, 40, 48, 60])
        add(r.choice([1, 4, 64]), P, P, r.randint(3, 64), r.randint(17, 48), r.randint(33, 48), 1)
    return out


def probe_of(L):
    L.ffgpu_irb_plan_text.argtypes = [ctypes.c_int] * 12 + [ctypes.c_char_p, ctypes.c_int]
    buf = ctypes.create_string_buffer(1024)

    def probe(t, flags=0):
        L.ffgpu_irb_plan_text(*t, flags, buf, len(buf))
        return buf.value.decode()
    return probe


def knob_names():
    """every variable the library reads, from its own table: a developer's shell must not change the census"""
    from ffcnn_amd import capi
    return [k["name"] for k in capi.knobs()]


def census(probe, geoms, setenv, delenv):
    """per geometry, the full line of every column"""
    for v in knob_names():
        delenv(v)
    cols = [[probe(t) for t in geoms], [probe(t, CONCURRENT) for t in geoms]]
    for k, v in SWITCHES:
        setenv(k, v)
        cols.append([probe(t) for t in geoms])
        delenv(k)
    return [[c[i] for c in cols] for i in range(len(geoms))]


def key_of(line):
    return line.split(" ")[0]


def write(lib_path, recorded_at):
    probe = probe_of(ctypes.CDLL(lib_path))
    geoms = geometries()
    rows = census(probe, geoms, os.environ.__setitem__, lambda v: os.environ.pop(v, None))
    keys = sorted({key_of(x) for row in rows for x in row})
    assert "launch-error" not in keys
    with open(FIXTURE, "w") as f:
        f.write('{"recorded_at": %s,\n "keys": %s,\n "columns": %s,\n "cases": [\n' % (json.dumps(recorded_at), json.dumps(keys), json.dumps(COLUMNS)))
        f.write(",\n".join(json.dumps(list(t) + ["".join(b36(keys.index(key_of(x))) for x in row), "".join("%08x" % zlib.crc32(x.encode()) for x in row)], separators=(",", ":"))
                           for t, row in zip(geoms, rows)))
        f.write("\n]}\n")
    print("%d geometries, %d keys, %d bytes" % (len(geoms), len(keys), os.path.getsize(FIXTURE)))
    for c in range(len(COLUMNS)):
        fam = [family(key_of(row[c])) for row in rows]
        print("%-24s %s" % (COLUMNS[c], " ".join("%s %d" % (n, fam.count(n)) for n in FAMILIES)))
    print("reachable but absent:", sorted(set(REACHABLE) - set(keys)), " present but not listed:", sorted(set(keys) - set(REACHABLE) - {"unsupported"}))


def b36(i):
    d = "0123456789abcdefghijklmnopqrstuvwxyz"
    return d[i // 36] + d[i % 36]


@pytest.fixture(scope="module")
def probe():
    from ffcnn_amd import capi
    capi.build_library()
    return capi.irb_plan_text


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def golden_keys(golden, c):
    return [golden["keys"][int(row[11][2 * c:2 * c + 2], 36)] for row in golden["cases"]]


def test_fixture_covers_every_family_and_reachable_instantiation(golden):
    assert golden["columns"] == COLUMNS and os.path.getsize(FIXTURE) < 100 * 1024
    assert [tuple(row[:11]) for row in golden["cases"]] == geometries()
    cols = [golden_keys(golden, c) for c in range(len(COLUMNS))]
    for n in FAMILIES:
        best = max([family(k) for k in col].count(n) for col in cols)
        assert best >= FLOOR, (n, best)
    seen = {k for col in cols for k in col}
    assert seen == set(REACHABLE) | {"unsupported"}, seen ^ (set(REACHABLE) | {"unsupported"})


def test_irb_plan_matches_fixture(probe, golden, monkeypatch):
    geoms = [tuple(row[:11]) for row in golden["cases"]]
    got = census(probe, geoms, monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    bad = []
    for t, row, lines in zip(geoms, golden["cases"], got):
        for c, line in enumerate(lines):
            want_key, want_crc = golden["keys"][int(row[11][2 * c:2 * c + 2], 36)], row[12][8 * c:8 * c + 8]
            if key_of(line) != want_key or "%08x" % zlib.crc32(line.encode()) != want_crc:
                bad.append((t, COLUMNS[c], "recorded: %s (crc %s)" % (want_key, want_crc), "now: %s" % line))
    assert not bad, "%d of %d cells differ; the first: %s" % (len(bad), len(geoms) * len(COLUMNS), bad[:3])


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--write":         # --write <library built from the recorder patch> <commit>
        write(sys.argv[2], sys.argv[3])
    else:
        sys.exit("usage: test_irb_choice.py --write LIBRARY COMMIT")
