"""Zones and lines, without a GPU: the exported symbols, the layout of the scene, spec and slot structs in the ctypes mirror and the constants in the
header, the pure host functions (ffgpu_zones_state_bytes, ffgpu_scene_check) on good and hostile arguments, the host glue under ASan + UBSan
(san/zones_driver.cc, run as a child process), tests/zones/zoneref.py (the numpy restatement of the contract the GPU tests compare with) pinned to a
literal scalar loop on seeded sequences and to the contract's properties, the seeded cases of the GPU fuzz held to the conditions that keep it from
passing vacuously, and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from zones import fuzzcases, zoneref

SYMBOLS = ["ffgpu_zones_state_bytes", "ffgpu_scene_check", "ffgpu_zones_reset_dev", "ffgpu_zones_boxes_dev", "ffgpu_exec_zones"]
NAN, INF = float("nan"), float("inf")
F32 = np.float32
S = zoneref.Spec
BOX = zoneref.BOX_DTYPE
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_zones_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_zones_struct_layout(capi):
    Z, Ln, Sc, P, Q = capi.Zone, capi.Line, capi.Scene, capi.ZonesSpec, capi.ZoneSlot
    assert [C.sizeof(t) for t in (Z, Ln, Sc, P, Q)] == [96, 32, 1040, 32, 64]
    assert [getattr(Z, f).offset for f in ("x", "y", "nverts", "dwell_frames", "classes", "reserved")] == [0, 32, 64, 68, 72, 88]
    assert [getattr(Ln, f).offset for f in ("ax", "ay", "bx", "by", "classes")] == [0, 4, 8, 12, 16]
    assert [getattr(Sc, f).offset for f in ("zone", "line", "nzones", "nlines", "anchor", "reserved")] == [0, 768, 1024, 1028, 1032, 1036]
    assert [getattr(P, f).offset for f in ("capacity", "max_missed", "identity", "flags", "min_score", "gate_zone", "gate_line", "reserved")] == list(range(0, 32, 4))
    assert [getattr(Q, f).offset for f in ("id", "px", "py", "inside", "last", "reserved", "since")] == [0, 4, 8, 12, 16, 20, 32]
    for dt, ct in ((zoneref.ZONE_DTYPE, Z), (zoneref.LINE_DTYPE, Ln), (zoneref.SCENE_DTYPE, Sc), (zoneref.SLOT_DTYPE, Q)):
        assert dt.itemsize == C.sizeof(ct) and [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]
    assert capi.ZONE_SLOT_DTYPE == zoneref.SLOT_DTYPE and zoneref.BOX_DTYPE == capi.BOX_DTYPE
    assert (capi.SCENE_ZONES, capi.SCENE_LINES, capi.ZONE_VERTS, capi.ZONES_DETS, capi.ZONES_ROW) == (8, 8, 8, 128, 64) == (8, 8, 8, zoneref.DETS, zoneref.ROW)
    assert (capi.ZONES_NONE, capi.ZONES_TYPE, capi.ZONES_IDS, capi.ZONES_GATE_INVERT, capi.ZONES_ENTRIES, capi.ZONES_MERGED) == (0, 1, 2, 1, 0, 1)
    assert (zoneref.NONE, zoneref.TYPE, zoneref.IDS) == (0, 1, 2) and capi.ZONES_EVENTS_HEADER == zoneref.HEADER and capi.ZONES_STATE_HEADER == zoneref.STATE_HEADER == 144
    sp = capi.zones_spec(5, max_missed=2, identity=capi.ZONES_TYPE, min_score=0.125, gate_zone=0xff00, gate_line=3, invert=True)
    assert (sp.capacity, sp.max_missed, sp.identity, sp.flags, sp.min_score, sp.gate_zone, sp.gate_line, sp.reserved) == (5, 2, 1, 1, 0.125, 0xff00, 3, 0)
    zones_ = [([(0, 0), (8, 0), (8, 8)], 3, [1, 33, 127]), ([(1, 1), (2, 1), (2, 2), (1, 2)],)]
    lines_ = [((0, 4), (9, 4), [2]), ((3, 0), (3, 9))]
    assert capi.scenes_bytes([capi.scene(zones_, lines_, anchor=1)]) == zoneref.make_scene(zones_, lines_, anchor=1).tobytes()
    assert capi.class_mask([1, 33, 127]) == [2, 2, 0, 1 << 31] == zoneref.class_mask([1, 33, 127]) and capi.class_mask() == [0, 0, 0, 0]
    hdr, slots = capi.zones_state(np.zeros(3 * (144 + 64 * 5), np.uint8), 3, 5)
    assert len(hdr) == 3 and hdr[0]["frames"] == 0 and hdr[2]["total_back"] == [0] * 8 and slots.shape == (3, 5)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    for phrase in ("} ffgpu_zone;", "} ffgpu_line;", "} ffgpu_scene;", "} ffgpu_zones_spec;", "} ffgpu_zone_slot;", "1040 bytes", "144-byte header",
                   "px = (x1 + x2) * 0.5f", "py = anchor ? y2 : (y1 + y2) * 0.5f", "d = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)", "yj > yi ? d > 0 : d < 0",
                   "side(P) = ((bx - ax) * (Py - ay) - (by - ay) * (Px - ax)) > 0", "entered = inside & ~slot.inside", "left = slot.inside & ~inside",
                   "frame - since[z] >= dwell_frames", "frame - last > max_missed", "GATED RECORD",
                   "(((word0 & gate_zone) | (word1 & gate_line)) != 0) != (flags & FFGPU_ZONES_GATE_INVERT)", "tests/zones/zoneref.py",
                   "A rejected call leaves the state as it was", "Works on FFGPU_SPLIT2 executors"):
        assert phrase in hdr, phrase
    for name, val in (("FFGPU_SCENE_ZONES", 8), ("FFGPU_SCENE_LINES", 8), ("FFGPU_ZONE_VERTS", 8), ("FFGPU_ZONES_DETS", 128), ("FFGPU_ZONES_ROW", 64),
                      ("FFGPU_ZONES_NONE", 0), ("FFGPU_ZONES_TYPE", 1), ("FFGPU_ZONES_IDS", 2), ("FFGPU_ZONES_GATE_INVERT", 1), ("FFGPU_ZONES_ENTRIES", 0),
                      ("FFGPU_ZONES_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_zones.inc"' in inc and inc.index('#include "ffgpu_track.inc"') < inc.index('#include "ffgpu_zones.inc"')
    host = open(os.path.join(CSRC, "ffgpu_zones_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP


# ------------------------------------------------------------------------------------------------- pure host functions
def test_state_bytes_is_pure_host_code(capi):
    assert [capi.zones_state_bytes(*a) for a in ((1, 1), (1, 128), (3, 5), (65536, 128))] == [208, 144 + 64 * 128, 3 * (144 + 320), 65536 * (144 + 64 * 128)]
    assert [capi.zones_state_bytes(*a) for a in ((0, 1), (-1, 1), (65537, 1), (1, 0), (1, -3), (1, 129), (0, 0))] == [0] * 7
    for ns, cap in ((1, 1), (3, 5), (65, 128)):
        assert capi.zones_state_bytes(ns, cap) == zoneref.state_nbytes(ns, cap) == len(zoneref.State(ns, cap).tobytes())


def test_scene_check_on_good_and_hostile_scenes(capi):
    def good():
        return capi.scene([([(0, 0), (10, 0), (10, 10), (0, 10)], 5), ([(20, 0), (30, 0), (25, 9)],)], [((0, 5), (30, 5))])
    capi.scene_check([good(), capi.scene(), good()])
    junk = good()
    junk.zone[5].nverts, junk.zone[5].x[0], junk.line[3].ax, junk.zone[7].dwell_frames = -7, NAN, INF, -1       # behind nzones / nlines: not looked at
    capi.scene_check([junk])

    def bad(change, msg):
        sc = good()
        change(sc)
        with pytest.raises(RuntimeError, match=msg):
            capi.scene_check([good(), sc])
    bad(lambda s: setattr(s, "nzones", 9), "scene 1: nzones 9")
    bad(lambda s: setattr(s, "nzones", -1), "scene 1: nzones -1")
    bad(lambda s: setattr(s, "nlines", 9), "scene 1: nlines 9")
    bad(lambda s: setattr(s, "nlines", -2 ** 31), "nlines")
    bad(lambda s: setattr(s.zone[1], "nverts", 2), "zone 1: nverts 2")
    bad(lambda s: setattr(s.zone[0], "nverts", 9), "zone 0: nverts 9")
    bad(lambda s: s.zone[1].y.__setitem__(2, NAN), "zone 1: vertex 2 is not finite")
    bad(lambda s: s.zone[0].x.__setitem__(3, -INF), "zone 0: vertex 3 is not finite")
    bad(lambda s: setattr(s.zone[1], "dwell_frames", -3), "negative dwell_frames -3")
    bad(lambda s: s.zone[0].reserved.__setitem__(1, 4), "zone 0: reserved")
    bad(lambda s: setattr(s.line[0], "by", NAN), "line 0 is not finite")
    bad(lambda s: (setattr(s.line[0], "bx", 0.0), setattr(s.line[0], "by", 5.0)), "line 0: A equals B")
    bad(lambda s: setattr(s, "anchor", 2), "anchor 2")
    bad(lambda s: setattr(s, "reserved", 1), "scene 1: reserved")
    assert capi.lib().ffgpu_scene_check(None, 1) < 0 and "NULL scenes" in capi.last_error()
    assert capi.lib().ffgpu_scene_check((capi.Scene * 1)(good()), 0) < 0 and "0 scenes" in capi.last_error()


def test_zones_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_zones_boxes_dev(None, None, 0, None, None, 1, None, None, None, 1, None, None, None, None, None),
                 lambda: L.ffgpu_zones_reset_dev(None, 1, 1, -1, None),
                 lambda: L.ffgpu_exec_zones(None, 0, None, 1, None, None, None, 1, None, None, None, None, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


def test_host_glue_under_the_sanitizers():
    """san/zones_driver.cc: the scene check, the spec and argument checks and the grouping by stream of ffgpu_zones_host.hpp on the CPU under
    ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "zones"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_zones_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"zones_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) >= 70, out[-1]
    assert not any("WRONG" in ln for ln in out)
    assert "args.stream_high -1 op: target 1: stream 2 is outside -1 .. 1" in out and "scene.line_a_is_b -1 scene_check: scene 1: line 0: A equals B" in out
    assert "group.all_distinct groups=128" in out


# ------------------------------------------------------------------------------------------------- zoneref against a literal scalar loop
def f32(v):
    return F32(v)


def literal_admits(mask, cls, known):
    if not any(int(m) for m in mask):
        return True
    return bool(known and 0 <= cls < 128 and (int(mask[cls >> 5]) >> (cls & 31)) & 1)


def literal_inside(zone, px, py):
    nv = int(zone["nverts"])
    if nv < 3 or nv > 8:
        return False
    xs, ys = [f32(v) for v in zone["x"][:nv]], [f32(v) for v in zone["y"][:nv]]
    if any(v != v for v in xs + ys):
        return False
    inside = False
    with np.errstate(all="ignore"):
        for i in range(nv):
            j = (i + 1) % nv
            xi, yi, xj, yj = xs[i], ys[i], xs[j], ys[j]
            if bool(yi > py) != bool(yj > py):
                d = f32(f32(f32(xj - xi) * f32(py - yi)) - f32(f32(px - xi) * f32(yj - yi)))
                if (d > 0) if yj > yi else (d < 0):
                    inside = not inside
    return inside


def literal_side(ax, ay, bx, by, px, py):
    with np.errstate(all="ignore"):
        return bool(f32(f32(f32(bx - ax) * f32(py - ay)) - f32(f32(by - ay) * f32(px - ax))) > 0)


def literal_frame(hdr, slots, scene, boxes, idrow, spec, stride):
    """the contract word for word on Python lists of dicts, one box at a time; the owners are walked in list order, not sorted"""
    fr = hdr["frames"]
    nz, nl = max(0, min(int(scene["nzones"]), 8)), max(0, min(int(scene["nlines"]), 8))
    cons, dropped = [], 0
    for k, b in enumerate(boxes):
        if b["score"] >= spec.min_score:
            if len(cons) < 128:
                cons.append(k)
            else:
                dropped += 1
    row = [0] * (64 + 2 * stride)
    known_cls = spec.identity != zoneref.TYPE
    info, seen_ids = [], set()
    for k in cons:
        b = boxes[k]
        with np.errstate(all="ignore"):
            px = f32(f32(f32(b["x1"]) + f32(b["x2"])) * f32(0.5))
            py = f32(b["y2"]) if int(scene["anchor"]) != 0 else f32(f32(f32(b["y1"]) + f32(b["y2"])) * f32(0.5))
        ident = 0 if spec.identity == zoneref.NONE else int(b["type"]) if spec.identity == zoneref.TYPE else int(idrow[8 + k])
        ins = 0
        for z in range(nz):
            if literal_admits(scene["zone"][z]["classes"], int(b["type"]), known_cls) and literal_inside(scene["zone"][z], px, py):
                ins |= 1 << z
        kind = "anonymous" if ident <= 0 else "duplicate" if ident in seen_ids else "owner"
        if kind == "owner":
            seen_ids.add(ident)
        info.append(dict(k=k, px=px, py=py, ident=ident, ins=ins, kind=kind, cls=int(b["type"]), w0=ins, w1=0))
    ev, ln = [[0] * 4 for _ in range(8)], [[0] * 2 for _ in range(8)]
    named = set()
    for o in info:
        for z in range(8):
            ev[z][0] += (o["ins"] >> z) & 1
        if o["kind"] == "anonymous":
            o["w1"] |= 1 << 20
        if o["kind"] == "duplicate":
            o["w1"] |= 1 << 19
        if o["kind"] != "owner":
            continue
        hit = [s for s, q in enumerate(slots) if q["id"] == o["ident"]]
        if not hit:
            o["kind"] = "unknown"
            continue
        q = slots[hit[0]]
        named.add(hit[0])
        was = q["inside"] & 0xff
        entered, left, loit = o["ins"] & ~was, was & ~o["ins"], 0
        for z in range(8):
            if (entered >> z) & 1:
                q["since"][z] = fr
        for l in range(nl):
            L = scene["line"][l]
            if not literal_admits(L["classes"], o["cls"], known_cls):
                continue
            a, b_ = (f32(L["ax"]), f32(L["ay"])), (f32(L["bx"]), f32(L["by"]))
            p0, p1 = (f32(q["px"]), f32(q["py"])), (o["px"], o["py"])
            s0, s1 = literal_side(*a, *b_, *p0), literal_side(*a, *b_, *p1)
            if s0 != s1 and literal_side(*p0, *p1, *a) != literal_side(*p0, *p1, *b_):
                o["w1"] |= 1 << (l if s1 else 8 + l)
                ln[l][0 if s1 else 1] += 1
        for z in range(nz):
            dwell = int(scene["zone"][z]["dwell_frames"])
            if (o["ins"] >> z) & 1 and dwell > 0 and zoneref.sdiff(fr, q["since"][z]) >= dwell:
                loit |= 1 << z
        q.update(px=o["px"], py=o["py"], inside=o["ins"], last=fr)
        o["w0"] |= entered << 8 | left << 16 | loit << 24
        o["w1"] |= 1 << 16
        for z in range(8):
            ev[z][1] += (entered >> z) & 1
            ev[z][2] += (left >> z) & 1
            ev[z][3] += (loit >> z) & 1
    freed = 0
    for s, q in enumerate(slots):
        if q["id"] != 0 and s not in named and zoneref.sdiff(fr, q["last"]) > spec.max_missed:
            for z in range(8):
                ev[z][2] += (q["inside"] >> z) & 1
            slots[s] = dict(id=0, px=f32(0), py=f32(0), inside=0, last=0, since=[0] * 8)
            freed += 1
    fresh = refused = 0
    for o in info:
        if o["kind"] != "unknown":
            continue
        free = [s for s, q in enumerate(slots) if q["id"] == 0]
        if not free:
            o["w1"] |= 1 << 18
            refused += 1
            continue
        slots[free[0]] = dict(id=o["ident"], px=o["px"], py=o["py"], inside=o["ins"], last=fr, since=[fr if (o["ins"] >> z) & 1 else 0 for z in range(8)])
        o["w0"] |= o["ins"] << 8
        o["w1"] |= 1 << 17
        fresh += 1
        for z in range(8):
            ev[z][1] += (o["ins"] >> z) & 1
    hdr["frames"] = fr + 1
    hdr["live"] = sum(q["id"] != 0 for q in slots)
    for k in range(8):
        hdr["entered"][k] += ev[k][1]
        hdr["left"][k] += ev[k][2]
        hdr["fwd"][k] += ln[k][0]
        hdr["back"][k] += ln[k][1]
    row[:10] = [len(cons), sum(o["w1"] >> 16 & 1 for o in info), fresh, refused, sum(o["kind"] == "duplicate" for o in info),
                sum(o["kind"] == "anonymous" for o in info), dropped, freed, hdr["live"], fr]
    for z in range(8):
        row[16 + 4 * z:20 + 4 * z] = ev[z]
        row[48 + 2 * z:50 + 2 * z] = ln[z]
    gated = []
    for o in info:
        row[64 + 2 * o["k"]], row[65 + 2 * o["k"]] = o["w0"], o["w1"]
        if (((o["w0"] & spec.gate_zone) | (o["w1"] & spec.gate_line)) != 0) != spec.invert:
            gated.append(o["k"])
    return row, gated


def same_bits(a, b):
    return np.asarray(a, F32).tobytes() == np.asarray(b, F32).tobytes()


def test_zoneref_is_the_literal_loop():
    rng = np.random.default_rng(5500)
    seen = dict.fromkeys(("known", "fresh", "refused", "duplicate", "anonymous", "freed", "entered", "left", "loitering", "fwd", "back", "gated"), 0)
    for case in range(40):
        cap = int(rng.choice([1, 2, 3, 7, 16]))
        ident = int(rng.choice([zoneref.NONE, zoneref.TYPE, zoneref.IDS, zoneref.IDS]))
        spec = S(cap, max_missed=int(rng.integers(0, 3)), identity=ident, min_score=float(rng.choice([0.0, 0.25])),
                 gate_zone=int(rng.choice([0, 0xff, 0xff00, 0xffffffff])), gate_line=int(rng.choice([0, 0xffff, 1 << 17])), invert=bool(rng.integers(0, 2)))
        scene = fuzzcases.rand_scene(rng, case)
        st = zoneref.State(1, cap)
        hdr = dict(frames=0, live=0, entered=[0] * 8, left=[0] * 8, fwd=[0] * 8, back=[0] * 8)
        slots = [dict(id=0, px=f32(0), py=f32(0), inside=0, last=0, since=[0] * 8) for _ in range(cap)]
        lists, idents = fuzzcases.video(rng, 6, [int(rng.integers(0, 12)) for _ in range(3)], type_is_id=ident == zoneref.TYPE, weird=0.04)
        for f, (b, ids) in enumerate(zip(lists, idents)):
            stride = len(b) + 2
            idrow = np.concatenate([rng.integers(-3, 3, 8), ids, rng.integers(-3, 3, 2)]).astype("<i4")
            row, gb = zoneref.frame(st.hdr[0], st.slots[0], scene, b, idrow if ident == zoneref.IDS else None, spec, stride)
            lrow, lgated = literal_frame(hdr, slots, scene, [dict(zip(b.dtype.names, (x[c] for c in b.dtype.names))) for x in b], idrow, spec, stride)
            assert [int(v) for v in row.view("<u4")] == lrow, (case, f)
            assert gb.tobytes() == b[lgated].tobytes(), (case, f)
            assert [int(v) for v in st.hdr[0][:2]] == [hdr["frames"], hdr["live"]]
            assert [int(v) for v in st.hdr[0][4:36]] == hdr["entered"] + hdr["left"] + hdr["fwd"] + hdr["back"]
            for s in range(cap):
                q, lq = st.slots[0][s], slots[s]
                assert (int(q["id"]), int(q["inside"]), int(q["last"]), [int(v) for v in q["since"]]) == (lq["id"], lq["inside"], lq["last"], lq["since"]), (case, f, s)
                assert (same_bits(q["px"], lq["px"]) or (np.isnan(q["px"]) and np.isnan(lq["px"]))) and (same_bits(q["py"], lq["py"]) or (np.isnan(q["py"]) and np.isnan(lq["py"])))
            for i, name in ((1, "known"), (2, "fresh"), (3, "refused"), (4, "duplicate"), (5, "anonymous"), (7, "freed")):
                seen[name] += int(row[i])
            for i, name in enumerate(("entered", "left", "loitering")):
                seen[name] += int(row[17 + i:48:4].sum())
            seen["fwd"] += int(row[48:64:2].sum())
            seen["back"] += int(row[49:64:2].sum())
            seen["gated"] += len(gb)
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------- properties
def boxes_at(points, types=None, score=0.5):
    """boxes whose centre anchor is exactly the given point (coordinates on a grid of eighths: +-2 is exact)"""
    b = np.zeros(len(points), BOX)
    for k, (x, y) in enumerate(points):
        b[k] = (types[k] if types else 0, score, x - 2, y - 2, x + 2, y + 2)
    return b


def run(frames, spec, scene, ids=None, state=None):
    """one stream, its frames one after the other: ([event row per frame], [gated boxes per frame], the state)"""
    st = state or zoneref.State(1, spec.capacity)
    rows, outs = [], []
    for f, b in enumerate(frames):
        n = max(1, len(b))
        idrow = None if ids is None else np.concatenate([np.zeros(8, "<i4"), np.asarray(ids[f], "<i4"), np.zeros(n - len(b), "<i4")])
        row, gb = zoneref.frame(st.hdr[0], st.slots[0], scene, b, idrow, spec, n)
        rows.append(row)
        outs.append(gb)
    return rows, outs, st


@pytest.mark.parametrize("step", [1.0, 0.125])
def test_a_fan_of_triangles_partitions_its_polygon(step):
    """integer grid (and a grid of eighths): the products are exact, so every point of the polygon -- the points on the spokes shared by two triangles
    included -- is in exactly one triangle of the fan round an interior point, and every point outside is in none"""
    rng = np.random.default_rng(5501)
    checked = shared = 0
    for trial in range(12):
        nv = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
        hub = rng.integers(-3, 4, 2) * step
        poly = [(float(np.round((hub[0] + r * np.cos(a)) / step) * step), float(np.round((hub[1] + r * np.sin(a)) / step) * step))
                for a, r in zip(ang, rng.integers(6, 14, nv) * step)]
        hubp = (float(hub[0]), float(hub[1]))
        if nv == 3 or np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]])).max() >= np.pi:
            continue                                                                    # (the hub must be strictly inside: a star-shaped polygon round it)
        whole = zoneref.make_scene([(poly,)])["zone"][0]
        fans = [zoneref.make_scene([([hubp, poly[i], poly[(i + 1) % nv]],)])["zone"][0] for i in range(nv)]
        g = np.arange(-16, 17) * step
        px, py = (v.reshape(-1).astype(F32) for v in np.meshgrid(g, g))
        inw = zoneref.inside(whole, px, py)
        count = sum(zoneref.inside(t, px, py).astype(int) for t in fans)
        assert (count == inw.astype(int)).all(), (trial, poly, hubp)
        # the spokes hub -> vertex: their grid points strictly between are shared edges of two triangles
        for vx, vy in poly:
            for k in range(1, 8):
                sx, sy = hubp[0] + (vx - hubp[0]) * k / 8, hubp[1] + (vy - hubp[1]) * k / 8
                p = (np.array([sx], F32), np.array([sy], F32))                      # (a multiple of step / 8, below 32: the products keep under 24 bits)
                assert float(p[0][0]) == sx and float(p[1][0]) == sy
                assert sum(int(zoneref.inside(t, *p)[0]) for t in fans) == int(zoneref.inside(whole, *p)[0]) == 1
                shared += 1
        checked += len(px)
    assert checked > 5000 and shared > 50


def test_a_point_walking_over_a_line_counts_alternately_and_beyond_its_end_nothing():
    scene = zoneref.make_scene([], [((0, 10), (20, 10))])
    spec = S(4, max_missed=0, identity=zoneref.IDS)
    path = [(5, 8), (5, 12), (6, 8), (6, 12), (7, 9), (7, 9), (7, 11)]
    rows, _, st = run([boxes_at([p]) for p in path], spec, scene, ids=[[9]] * len(path))
    side = zoneref.side(0, 10, 20, 10, 5, 12)
    got = [(int(r[48]), int(r[49])) for r in rows]
    fwd, back = ((1, 0), (0, 1)) if side else ((0, 1), (1, 0))
    assert got == [(0, 0), fwd, back, fwd, back, (0, 0), fwd]
    assert [int(v) for v in st.hdr[0][20:22]] + [int(v) for v in st.hdr[0][28:30]] == [3 if side else 2, 0, 2 if side else 3, 0]
    assert int(rows[1][64 + 1]) & 0xffff == (1 if side else 1 << 8)
    # beyond the segment's end: the same walk at x = 25 crosses the line's extension, not the line
    rows, _, st = run([boxes_at([(25, y)]) for y in (8, 12, 8, 12)], spec, scene, ids=[[9]] * 4)
    assert not any(r[48:64].any() for r in rows) and not st.hdr[0][20:36].any()
    # an anonymous walker and one refused for want of a slot cause no events
    rows, _, _ = run([boxes_at([p]) for p in path], spec, scene, ids=[[0]] * len(path))
    assert not any(r[48:64].any() for r in rows) and all(int(r[5]) == 1 for r in rows)
    rows, _, _ = run([boxes_at([(50, 50), p]) for p in path], S(1, identity=zoneref.IDS), scene, ids=[[1, 9]] * len(path))
    assert not any(r[48:64].any() for r in rows) and all(int(r[3]) == 1 for r in rows)


def seeded(seed, ident=zoneref.IDS, cap=6, nframes=8):
    rng = np.random.default_rng(seed)
    scene = fuzzcases.rand_scene(rng, 0)
    lists, idents = fuzzcases.video(rng, nframes, [7, 3, 9], type_is_id=ident == zoneref.TYPE)
    return scene, lists, idents


def test_a_sequence_cut_into_calls_leaves_the_same_bytes():
    scene, lists, idents = seeded(5502)
    recs = np.zeros(len(lists), zoneref.DETS_DTYPE)
    stride = 12
    flat, ids = np.zeros(len(lists) * stride, BOX), np.zeros((len(lists), 8 + stride), "<i4")
    for t, b in enumerate(lists):
        recs[t]["nfull"] = len(b)
        flat[t * stride:t * stride + len(b)] = b
        ids[t, 8:8 + len(b)] = idents[t]
    spec, scenes = S(4, max_missed=1, gate_zone=0xff), np.array([scene], zoneref.SCENE_DTYPE)
    st = zoneref.State(1, 4)
    whole = zoneref.zones(recs, flat, stride, None, [0] * len(lists), spec, scenes, st, ids)
    for cuts in ([3], [1, 2, 5], list(range(1, len(lists)))):
        st2, parts = zoneref.State(1, 4), []
        for a, b in zip([0] + cuts, cuts + [len(lists)]):
            parts.append(zoneref.zones(recs[a:b], flat[a * stride:], stride, None, [0] * (b - a), spec, scenes, st2, ids[a:b]))
        assert st2.tobytes() == st.tobytes()
        for k in range(3):
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes()
    assert whole[0][:, 17:48:4].sum() > 0 and st.hdr[0][0] == len(lists)


def test_identical_frames_produce_no_events_after_the_first():
    scene, lists, idents = seeded(5505)
    rows, _, st = run([lists[0]] * 5, S(16, max_missed=0), scene, ids=[idents[0]] * 5)
    assert rows[0][17:48:4].sum() > 0                                                  # the first frame: everybody inside something enters
    for r in rows[1:]:
        assert not r[17:48:4].any() and not r[18:48:4].any() and not r[48:64].any() and int(r[2]) == 0 and int(r[7]) == 0
        assert (r[16:48:4] == rows[0][16:48:4]).all() and (r[64::2] & 0xffff00 == 0).all() and (r[65::2] & 0xffff == 0).all()
    assert sum(int(r[19:48:4].sum()) for r in rows) > 0                                # but they loiter


def test_frees_count_as_left():
    scene = zoneref.make_scene([([(0, 0), (20, 0), (20, 20), (0, 20)],), ([(0, 0), (10, 0), (10, 10), (0, 10)],)])
    spec = S(4, max_missed=1, identity=zoneref.IDS)
    frames, ids = [boxes_at([(5, 5), (15, 15)]), np.zeros(0, BOX), np.zeros(0, BOX), np.zeros(0, BOX)], [[1, 2], [], [], []]
    rows, _, st = run(frames, spec, scene, ids=ids)
    assert [int(v) for v in rows[0][16:24]] == [2, 2, 0, 0, 1, 1, 0, 0] and int(rows[0][8]) == 2
    assert not rows[1][16:64].any() and int(rows[1][7]) == 0 and int(rows[1][8]) == 2  # frame - last = 1: not yet
    assert [int(v) for v in rows[2][16:24]] == [0, 0, 2, 0, 0, 0, 1, 0] and int(rows[2][7]) == 2 and int(rows[2][8]) == 0
    assert not rows[3][16:64].any() and not st.slots.view(np.uint8).any()
    assert [int(v) for v in st.hdr[0][4:6]] == [2, 1] == [int(v) for v in st.hdr[0][12:14]] and [int(v) for v in st.hdr[0][:2]] == [4, 0]


def test_a_nan_box_or_vertex_is_never_inside():
    sq = [(0, 0), (20, 0), (20, 20), (0, 20)]
    scene = zoneref.make_scene([(sq,)])
    b = boxes_at([(10, 10)] * 6)
    b["x1"][1], b["y2"][2], b["x2"][3], b["y1"][4] = NAN, NAN, INF, -INF
    rows, _, _ = run([b], S(8, identity=zoneref.NONE), scene)
    assert [int(v) & 1 for v in rows[0][64::2]] == [1, 0, 0, 0, 0, 1]
    px, py = np.array([10, 1, 19, 5], F32), np.array([10, 1, 19, 15], F32)
    for k in range(4):
        for c in ("x", "y"):
            sc = zoneref.make_scene([(sq,)])
            sc["zone"][0][c][k] = NAN
            assert not zoneref.inside(sc["zone"][0], px, py).any()
            rows, _, _ = run([boxes_at([(10, 10)])], S(8, identity=zoneref.NONE), sc)
            assert int(rows[0][64]) == 0 and int(rows[0][16]) == 0
    sc = zoneref.make_scene([(sq,)])
    sc["zone"][0]["x"][5] = NAN                                                         # behind nverts: not a vertex
    assert zoneref.inside(sc["zone"][0], px, py).all()
    for nv in (-1, 0, 2, 9, 2 ** 31 - 1):
        sc["zone"][0]["nverts"] = nv
        assert not zoneref.inside(sc["zone"][0], px, py).any()


def test_gate_invert_gives_the_complement_among_the_considered():
    scene, lists, idents = seeded(5504)
    for gz, gl in ((0xff, 0), (0, 0xffff), (0xff00, zoneref.FRESH), (0, 0), (0xffffffff, 0xffffffff)):
        a = run(lists, S(6, max_missed=1, min_score=0.25, gate_zone=gz, gate_line=gl), scene, ids=idents)
        b = run(lists, S(6, max_missed=1, min_score=0.25, gate_zone=gz, gate_line=gl, invert=True), scene, ids=idents)
        assert a[2].tobytes() == b[2].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))     # the gate changes no state and no event
        for f, boxes in enumerate(lists):
            with np.errstate(invalid="ignore"):
                cons = boxes[boxes["score"] >= F32(0.25)]
            w0, w1 = a[0][f][64::2].view("<u4").astype(np.int64), a[0][f][65::2].view("<u4").astype(np.int64)
            with np.errstate(invalid="ignore"):
                considered = np.nonzero(boxes["score"] >= F32(0.25))[0]
            sel = ((w0[considered] & gz) | (w1[considered] & gl)) != 0
            assert len(cons) == int(a[0][f][0]) and a[1][f].tobytes() == cons[sel].tobytes() and b[1][f].tobytes() == cons[~sel].tobytes()
    assert any(len(x) for x in a[1]) and not any(len(x) for x in b[1])                  # (all bits set: everybody; inverted: nobody)


# ------------------------------------------------------------------------------------------------- the GPU fuzz's seeds
@pytest.mark.parametrize("cap", fuzzcases.CAPACITIES)
def test_fuzz_seeds_meet_the_conditions_on_the_reference_alone(cap):
    """the seeded cases of the GPU fuzz (tests/zones/fuzzcases.py) through zoneref, no device: every parametrisation shows entered, left, fwd, back,
    loitering, fresh, refused, duplicate, anonymous, freed, dropped, a non-empty and a non-full gated record -- a condition on the inputs"""
    cs = fuzzcases.fuzz_cases(cap)
    total = fuzzcases.check_stats(cs)
    print(cap, total)
    assert sorted(cs) == sorted(fuzzcases.NAMES)
    fr = cs["frames"]
    assert [len(fr.flat[t * fr.stride:][:int(fr.recs[t]["nfull"])]) for t in range(9)] == [0, 1, 127, 128, 129, 255, 256, 257, 6]
    assert len(cs["records 131"].streams) == 131 and cs["records 131"].streams.count(-1) == 6
    assert {int(s["nzones"]) for c in cs.values() for s in c.scenes} >= {0, 8, 11} and {int(s["nlines"]) for c in cs.values() for s in c.scenes} >= {0, 8, 12}
    assert {int(z["nverts"]) for c in cs.values() for s in c.scenes for z in s["zone"]} >= {0, 2, 3, 8, 9}
    assert {c.spec.identity for c in cs.values()} == {zoneref.NONE, zoneref.TYPE, zoneref.IDS}
    assert any((c.ids[:, 8:] < 0).any() for c in cs.values() if c.ids is not None)
    assert any(np.isnan(c.scenes["zone"]["x"]).any() or np.isnan(c.scenes["zone"]["y"]).any() for c in cs.values())
    assert any(c.first is not None for c in cs.values()) and any(c.flat is None for c in cs.values())
    assert any(c.rec_off is None for c in cs.values()) and any(c.list_off is None and c.rec_off is not None for c in cs.values())
