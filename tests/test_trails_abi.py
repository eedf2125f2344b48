"""Track trails, without a GPU: the exported symbols, the layout of the point, slot and spec structs in the ctypes mirror and the constants in the
header, the phrases of the contract, the host glue under ASan + UBSan (san/trails_driver.cc, run as a child process: every rejection with its
message), tests/trails/trailref.py (the numpy restatement of the contract the GPU tests compare with) pinned to a deliberately naive second
implementation -- Python lists of points per identity, no ring -- the seeded cases of the GPU fuzz held to the conditions that keep it from passing
vacuously, and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from trails import fuzzcases, trailref

SYMBOLS = ["ffgpu_trails_state_bytes", "ffgpu_trails_spec_check", "ffgpu_trails_reset_dev", "ffgpu_trails_boxes_dev", "ffgpu_exec_trails"]
CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")
F32 = np.float32
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


@pytest.fixture(scope="module", autouse=True)
def feature(capi):
    """every test of this file is a test of the feature, those that pin trailref and the fuzz's seeds too: a reference is worth what the library it
    restates carries, so each of them needs the built library to export the family and its slot layout to be trailref's"""
    missing = [s for s in SYMBOLS if s not in capi.EXPORTS or not hasattr(capi.lib(), s)]
    assert not missing, "libffcnn_hip.so lacks %s" % missing
    assert capi.TRAIL_SLOT_DTYPE == trailref.SLOT_DTYPE and C.sizeof(capi.TrailSlot) == trailref.SLOT_DTYPE.itemsize


# ------------------------------------------------------------------------------------------------- symbols, layout, header
def test_trails_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_trails_struct_layout(capi):
    Pt, Sl, Sp = capi.TrailPoint, capi.TrailSlot, capi.TrailsSpec
    assert (C.sizeof(Pt), C.sizeof(Sl), C.sizeof(Sp)) == (12, 416, 64)
    assert [getattr(Pt, f).offset for f in ("x", "y", "frame")] == [0, 4, 8]
    assert [getattr(Sl, f).offset for f in ("id", "last", "n", "head", "cx", "cy", "reserved", "ring")] == [0, 4, 8, 12, 16, 20, 24, 32]
    assert [getattr(Sp, f).offset for f in ("capacity", "max_missed", "identity", "flags", "min_score", "anchor", "points", "min_move", "thickness", "coast_dash", "color",
                                            "reserved0", "palette", "npalette", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 60]
    D = capi.TRAIL_SLOT_DTYPE
    assert D == trailref.SLOT_DTYPE and D.itemsize == 416 and [D.fields[f[0]][1] for f in Sl._fields_] == [getattr(Sl, f[0]).offset for f in Sl._fields_]
    assert capi.SEG_ITEM_DTYPE == trailref.ITEM_DTYPE
    assert (capi.TRAIL_POINTS, capi.TRAILS_DETS, capi.TRAILS_ROW, capi.TRAILS_COAST, capi.TRAILS_TAPER, capi.TRAILS_ENTRIES, capi.TRAILS_MERGED, capi.TRAILS_STATE_HEADER) == \
        (32, 128, 16, 1, 2, 0, 1, 16) == (trailref.POINTS, trailref.DETS, trailref.ROW, trailref.COAST, trailref.TAPER, 0, 1, trailref.STATE_HEADER)
    assert capi.TRAILS_ROW_HEADER == trailref.HEADER and (capi.ZONES_TYPE, capi.ZONES_IDS) == (trailref.TYPE, trailref.IDS)
    sp = capi.trails_spec(7, 3, capi.ZONES_TYPE, 0.5, 1, 9, 4, 5, coast=True, taper=True, coast_dash=2, color=(4, 5, 6), palette=[(7, 8, 9), (10, 11, 12)])
    assert (sp.capacity, sp.max_missed, sp.identity, sp.flags, sp.min_score, sp.anchor, sp.points, sp.min_move, sp.thickness, sp.coast_dash, list(sp.color), sp.reserved0,
            sp.npalette, sp.reserved) == (7, 3, 1, 3, 0.5, 1, 9, 4, 5, 2, [4, 5, 6, 0], 0, 2, 0)
    assert bytes((C.c_ubyte * 8).from_address(sp.palette)) == bytes([7, 8, 9, 0, 10, 11, 12, 0])
    capi.trails_spec_check(sp)
    sp.points = 33
    with pytest.raises(Exception, match="points 33 is outside 2..32"):
        capi.trails_spec_check(sp)
    assert capi.trails_state_bytes(3, 5) == 3 * (16 + 416 * 5) == trailref.state_nbytes(3, 5) and capi.trails_state_bytes(65536, 128) == 65536 * (16 + 416 * 128)
    assert [capi.trails_state_bytes(*a) for a in ((0, 1), (65537, 1), (1, 0), (1, 129), (-1, -1))] == [0] * 5
    st = trailref.State(2, 3)
    st.hdr[1] = (5, 1, 0, 0)
    st.slots[1, 2]["id"], st.slots[1, 2]["ring"][31] = 9, (1, 2, 3)
    hdr, slots = capi.trails_state(np.frombuffer(st.tobytes(), np.uint8), 2, 3)
    assert hdr.tolist() == [[0, 0, 0, 0], [5, 1, 0, 0]] and slots.tobytes() == st.slots.tobytes() and tuple(slots[1, 2]["ring"][31]) == (1, 2, 3)


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    text = re.sub(r"\s*\n \*\s*", " ", hdr)                                             # (a phrase may run over a line of the comment)
    for phrase in ("} ffgpu_trail_point;", "} ffgpu_trail_slot;", "} ffgpu_trails_spec;", "tests/trails/trailref.py",
                   "416 bytes: id 0, last 4, n 8, head 12, cx 16, cy 20, reserved 24, ring 32",
                   "64 bytes: capacity 0, max_missed 4, identity 8, flags 12, min_score 16, anchor 20, points 24, min_move 28,",
                   "thickness 32, coast_dash 36, color 40, reserved0 44, palette 48, npalette 56, reserved 60",
                   "a free slot is all zero, all 416 bytes", "per stream a 16-byte header { int frames, live, reserved[2]; }", "all-zero is the valid empty state",
                   "n is clamped to 0..points and head is taken modulo 32", "a known owner's slot gets the clamped values back",
                   "px = (x1 + x2) * 0.5f; py = anchor ? y2 : (y1 + y2) * 0.5f", "toward zero, saturating, NaN -> 0",
                   "max(|A.x - N.x|, |A.y - N.y|) >= min_move, in 64-bit integers (min_move 0: always)", "and also when the slot has no live point (n == 0)",
                   "Append with n == points: head = (head + 1) % 32; otherwise n += 1", "ring[(head + n - 1) % 32] = { A.x, A.y, frame }",
                   "cx, cy = A and last = frame are set whether or not a point was appended", "with frame - last > max_missed, is zeroed, all 416 bytes",
                   "n = 1, head = 0, ring[0] = { A.x, A.y, frame }, cx, cy = A; every other byte of the slot is zero", "An owner that finds no free slot is REFUSED",
                   "refused, duplicate, anonymous, dropped, freed, live, frame, appended, drawn, clipped, 0, 0, 0 }", "the MOTION ROW { n, dx, dy, df }",
                   "64 bits and saturated to int; df = frame - O.frame, modulo 2^32 as signed", "may be NULL: then items_stride, first_item and nitems must be 0",
                   "every byte of those slots and no other byte", "THE ROW SHOWS THE STATE RIGHT AFTER RECORD t",
                   "a slot is DRAWN when id != 0, n >= 1 and (last == frame or FFGPU_TRAILS_COAST is set)", "while (k + 1) P <= nitems",
                   "with NULL items every drawn slot is clipped", "when j + 1 < n, otherwise 32 zero bytes", "the TIP: the segment from the newest live point to (cx, cy)",
                   "dash = coast_dash when last != frame, otherwise 0", "1 + ((T - 1) * (j + 1)) / n", "Redact, then draw, then outline, then trails, then caption",
                   "64 records per launch", "A rejected call leaves the state as it was", "_NONE is rejected: there is nobody to remember"):
        assert phrase in text, phrase
    assert hdr.index("---- outlines:") < hdr.index("---- track trails:") and "Redact, then draw, then outline, then caption: the tags lie on top" in hdr
    for name, val in (("FFGPU_TRAIL_POINTS", 32), ("FFGPU_TRAILS_DETS", 128), ("FFGPU_TRAILS_ROW", 16), ("FFGPU_TRAILS_COAST", 1), ("FFGPU_TRAILS_TAPER", 2),
                      ("FFGPU_TRAILS_ENTRIES", 0), ("FFGPU_TRAILS_MERGED", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val
    inc = open(os.path.join(CSRC, "ffgpu_kernels.hip")).read()
    assert '#include "ffgpu_trails.inc"' in inc and inc.index('#include "ffgpu_lines.inc"') < inc.index('#include "ffgpu_trails.inc"')
    host = open(os.path.join(CSRC, "ffgpu_trails_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer driver compiles it with no HIP
    kern = open(os.path.join(CSRC, "ffgpu_trails.inc")).read()
    assert "atomic" not in kern.replace("no atomic", "") and "printf" not in kern and "asm" not in kern and "__threadfence" not in kern
    assert "block_consider(" in kern and "ident_duplicate(" in kern and "slot_lowest(" in kern and "block_take_free(" in kern      # k_zones' primitives, not copies
    zones = open(os.path.join(CSRC, "ffgpu_zones.inc")).read()
    assert "block_consider(" in zones and "block_take_free(" in zones


# ------------------------------------------------------------------------------------------------- trailref against a naive second implementation
def naive_f2i(v):
    v = float(F32(v))
    if v != v:
        return 0
    return IMAX if v >= 2.0 ** 31 else IMIN if v <= -2.0 ** 31 else int(v)


def wrap(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


class NaiveStream:
    """one stream from the empty state: a list of capacity objects or None, every object a dict with a plain Python list of (x, y, frame) points that
    is cut at the front when it grows beyond `points`.  No ring, no head, no numpy but for the fp32 anchor."""

    def __init__(self, spec, frames=0):
        self.spec, self.frames, self.slots = spec, wrap(frames), [None] * spec.capacity

    def frame(self, boxes, idents, stride, nitems):
        sp, fr = self.spec, self.frames
        row = [0] * (trailref.ROW + 4 * stride)
        cons = [k for k in range(len(boxes)) if float(boxes[k]["score"]) >= float(sp.min_score)]
        dropped, cons = max(0, len(cons) - 128), cons[:128]
        seen, named, fresh_boxes, motion = set(), set(), [], {}
        known = dup = anon = appended = 0
        for k in cons:
            b = boxes[k]
            with np.errstate(all="ignore"):
                ax = naive_f2i((F32(b["x1"]) + F32(b["x2"])) * F32(0.5))
                ay = naive_f2i(F32(b["y2"]) if sp.anchor else (F32(b["y1"]) + F32(b["y2"])) * F32(0.5))
            id_ = int(idents[k])
            if id_ <= 0:
                anon += 1
                continue
            if id_ in seen:
                dup += 1
                continue
            seen.add(id_)
            at = [s for s, o in enumerate(self.slots) if o is not None and o["id"] == id_]
            if not at:
                fresh_boxes.append((k, id_, ax, ay))
                continue
            o = self.slots[at[0]]
            named.add(at[0])
            known += 1
            nx, ny, _ = o["pts"][-1]
            if max(abs(ax - nx), abs(ay - ny)) >= sp.min_move:
                o["pts"] = (o["pts"] + [(ax, ay, fr)])[-sp.points:]
                appended += 1
            o["c"], o["last"] = (ax, ay), fr
            motion[k] = o
        freed = 0
        for s, o in enumerate(self.slots):
            if o is not None and s not in named and wrap(fr - o["last"]) > sp.max_missed:
                self.slots[s] = None
                freed += 1
        fresh = refused = 0
        for k, id_, ax, ay in fresh_boxes:
            if None not in self.slots:
                refused += 1
                continue
            o = self.slots[self.slots.index(None)] = dict(id=id_, pts=[(ax, ay, fr)], c=(ax, ay), last=fr)
            motion[k] = o
            fresh += 1
        for k, o in motion.items():
            ox, oy, of = o["pts"][0]
            row[trailref.ROW + 4 * k:trailref.ROW + 4 * k + 4] = [len(o["pts"]), max(IMIN, min(IMAX, o["c"][0] - ox)), max(IMIN, min(IMAX, o["c"][1] - oy)), wrap(fr - of)]
        items, drawn, clipped, P = [], 0, 0, sp.points
        for o in self.slots:
            if o is None or not (o["last"] == fr or sp.coast):
                continue
            if len(items) + P > nitems:
                clipped += 1
                continue
            drawn += 1
            n, col, dash = len(o["pts"]), sp.colour(o["id"]), sp.coast_dash if o["last"] != fr else 0
            reg = [None] * P
            for j in range(n - 1):
                reg[j] = (o["pts"][j][:2] + o["pts"][j + 1][:2], col, 1 + ((sp.thickness - 1) * (j + 1)) // n if sp.taper else sp.thickness, dash)
            reg[P - 1] = (o["pts"][-1][:2] + o["c"], col, sp.thickness, dash)
            items += reg
        items += [None] * (nitems - len(items))
        live = sum(o is not None for o in self.slots)
        row[:13] = [len(cons), known, fresh, refused, dup, anon, dropped, freed, live, fr, appended, drawn, clipped]
        self.frames = wrap(fr + 1)
        return row, items


def naive_items(items):
    out = np.zeros(len(items), trailref.ITEM_DTYPE)
    for k, it in enumerate(items):
        if it is not None:
            (out[k]["x0"], out[k]["y0"], out[k]["x1"], out[k]["y1"]), out[k]["color"], out[k]["thickness"], out[k]["dash"] = it[0], it[1], it[2], it[3]
    return out


@pytest.mark.parametrize("cap", fuzzcases.CAPACITIES)
def test_trailref_equals_the_naive_lists(cap):
    """every seeded case that starts from an empty state (the junk state has no meaning the lists could hold): rows and items of every record"""
    for name, c in fuzzcases.fuzz_cases(cap).items():
        if name == "junk state":
            continue
        streams = [NaiveStream(c.spec, int(c.state0.hdr[s, 0])) for s in range(c.nstreams)]
        for t in range(c.n):
            if c.streams[t] < 0:
                assert not c.rows[t].any() and not c.items[t].view(np.uint8).any()
                continue
            f0 = t * c.stride if c.first is None else c.first[t]
            nb = max(0, min(int(c.recs[t]["nfull"]), c.stride))
            boxes = c.flat[f0:f0 + nb]
            idents = boxes["type"] if c.spec.identity == trailref.TYPE else c.ids[t, 8:8 + nb]
            row, items = streams[c.streams[t]].frame(boxes, idents, c.stride, c.nitems)
            assert row == c.rows[t].tolist(), (name, t)
            assert naive_items(items).tobytes() == c.items[t].tobytes(), (name, t)
        for s, ns in enumerate(streams):                                                 # and the state the ring holds is the lists'
            assert int(c.state.hdr[s, 0]) == ns.frames and int(c.state.hdr[s, 1]) == sum(o is not None for o in ns.slots)
            for q, o in zip(c.state.slots[s], ns.slots):
                assert (int(q["id"]) == 0) == (o is None)
                if o is None:
                    assert not np.frombuffer(q.tobytes(), np.uint8).any()
                    continue
                live = [tuple(int(v) for v in q["ring"][(int(q["head"]) + j) % 32]) for j in range(int(q["n"]))]
                assert live == o["pts"] and (int(q["cx"]), int(q["cy"]), int(q["last"]), int(q["id"])) == (o["c"][0], o["c"][1], o["last"], o["id"])


def test_trailref_on_named_cases():
    """by hand: a ring of two, min_move, a coasting slot, the taper, the clip, the clamp of a junk slot"""
    S = trailref.Spec
    sp = S(2, max_missed=1, identity=trailref.TYPE, points=2, min_move=3, thickness=5, coast=True, taper=True, coast_dash=4, palette=[(1, 1, 1), (2, 2, 2), (3, 3, 3)])
    st = trailref.State(1, 2)

    def rec(*boxes):
        r = np.zeros(1, trailref.DETS_DTYPE)
        r[0]["count"] = len(boxes)
        for k, (id_, x, y) in enumerate(boxes):
            r[0]["box"][k] = (id_, 1.0, x - 1, y - 1, x + 1, y + 1)
        return r

    def step(*boxes, nitems=4):
        rows, items = trailref.trails(rec(*boxes), None, 0, None, [0], sp, st, None, nitems)
        return rows[0], items[0]
    row, items = step((7, 10, 10), (4, 50, 50), (9, 1, 1), (7, 3, 3), (0, 2, 2))
    assert row[:13].tolist() == [5, 0, 2, 1, 1, 1, 0, 0, 2, 0, 0, 2, 0] and row[16:24].tolist() == [1, 0, 0, 0, 1, 0, 0, 0] and not row[24:36].any()
    assert [tuple(int(v) for v in (i["x0"], i["y0"], i["x1"], i["y1"], i["thickness"], i["dash"])) for i in items] == \
        [(0, 0, 0, 0, 0, 0), (10, 10, 10, 10, 5, 0), (0, 0, 0, 0, 0, 0), (50, 50, 50, 50, 5, 0)]
    assert items[1]["color"].tolist() == [2, 2, 2, 0] and items[3]["color"].tolist() == [2, 2, 2, 0]       # 7 % 3 == 4 % 3 == 1
    row, items = step((7, 12, 12))                                                      # moved 2 < min_move: not appended, the tip follows; 4 coasts dashed
    assert row[:13].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 2, 1, 0, 2, 0] and row[16:20].tolist() == [1, 2, 2, 1]
    assert [tuple(int(v) for v in (i["x0"], i["y0"], i["x1"], i["y1"], i["thickness"], i["dash"])) for i in items] == \
        [(0, 0, 0, 0, 0, 0), (10, 10, 12, 12, 5, 0), (0, 0, 0, 0, 0, 0), (50, 50, 50, 50, 5, 4)]
    row, items = step((7, 20, 5), nitems=3)                                             # appended; 4 is freed (missed 2 > 1); one region fits three slots
    assert row[:13].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 1, 2, 1, 1, 0] and row[16:20].tolist() == [2, 10, -5, 2]
    assert [tuple(int(v) for v in (i["x0"], i["y0"], i["x1"], i["y1"], i["thickness"], i["dash"])) for i in items] == \
        [(10, 10, 20, 5, 3, 0), (20, 5, 20, 5, 5, 0), (0, 0, 0, 0, 0, 0)]               # taper: 1 + (4 * 1) / 2 = 3
    row, items = step((7, 30, 5), nitems=1)                                             # the ring of two wraps: head 1; no room for a region: clipped
    assert row[:13].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1, 3, 1, 0, 1] and row[16:20].tolist() == [2, 10, 0, 1] and not items.view(np.uint8).any()
    q = st.slots[0, 0]
    assert (int(q["n"]), int(q["head"])) == (2, 1) and [tuple(int(v) for v in p) for p in q["ring"][:4]] == [(10, 10, 0), (20, 5, 2), (30, 5, 3), (0, 0, 0)]
    assert not np.frombuffer(st.slots[0, 1].tobytes(), np.uint8).any() and st.hdr[0].tolist() == [4, 1, 0, 0]
    # a junk slot: n above points reads as points, head modulo 32 (the non-negative remainder), and a known owner writes the clamped values back
    q["n"], q["head"] = 77, -31
    row, _ = step((7, 30, 5), nitems=0)
    assert (int(q["n"]), int(q["head"])) == (2, 1) and row[:13].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1, 4, 0, 0, 1]
    # a saturated anchor and a frame counter at the wrap
    st2 = trailref.State(1, 1)
    st2.hdr[0, 0] = -1
    sp2 = S(1, identity=trailref.TYPE, points=2)
    r = rec((3, 0, 0))
    r[0]["box"][0]["x2"], r[0]["box"][0]["y1"] = 1e30, np.nan
    rows, _ = trailref.trails(r, None, 0, None, [0], sp2, st2, None, 0)
    assert (int(st2.slots[0, 0]["cx"]), int(st2.slots[0, 0]["cy"]), int(st2.slots[0, 0]["last"])) == (IMAX, 0, -1) and st2.hdr[0].tolist() == [0, 1, 0, 0]
    r = rec((3, 0, 0))
    r[0]["box"][0]["x1"] = -1e30
    rows, _ = trailref.trails(r, None, 0, None, [0], sp2, st2, None, 0)
    assert rows[0, 16:20].tolist() == [2, IMIN, 0, 1]                                    # IMIN - IMAX saturates; the frame span crosses the wrap


# ------------------------------------------------------------------------------------------------- the seeds of the GPU fuzz
@pytest.mark.parametrize("cap", fuzzcases.CAPACITIES)
def test_fuzz_seeds_meet_the_conditions_on_the_reference_alone(cap):
    """the seeded cases of the GPU fuzz (tests/trails/fuzzcases.py) through trailref, no device: together they show a ring that wrapped, a point that
    min_move kept out, clipped, refused, duplicate, anonymous and dropped boxes, frees with max_missed 0 and above, a coasting slot drawn dashed, a
    taper of T = 8 with at least three thicknesses, a saturated coordinate and a frame counter that wraps through 2^32"""
    cases = fuzzcases.fuzz_cases(cap)
    total = fuzzcases.check_stats(cases)
    assert all(total[k] > 0 for k in ("wrapped", "not_appended", "clipped", "refused", "duplicate", "anonymous", "dropped", "freed", "dashed", "saturated"))
    ring, long_, junk = cases["ring"], cases["long lists"], cases["junk state"]
    assert ring.n == 40 and ring.spec.points == 32 and int(ring.state.slots[0, 0]["n"]) == 32 and int(ring.state.slots[0, 0]["head"]) == 8
    assert ring.first_item > 0 and ring.nitems == int(ring.rows[-1, 11]) * 32 and ring.items_stride > ring.first_item + ring.nitems
    assert cases["records 65"].n == 65 and cases["records 65"].items_off is None and len(set(cases["records 65"].streams[60:65])) >= 2
    assert max(int(r["nfull"]) for r in long_.recs) > 256 and long_.nitems < long_.spec.points and int(long_.state0.hdr[0, 0]) == -2
    assert cases["streams"].nitems % cases["streams"].spec.points != 0 and -1 in cases["streams"].streams and cases["streams"].nstreams == 6
    assert {c.spec.identity for c in cases.values()} == {trailref.TYPE, trailref.IDS} and {c.spec.points for c in cases.values()} == {2, 32}
    js = junk.state0.slots
    assert (js["n"] > 32).any() and (js["n"] < 0).any() and (js["head"] < 0).any() and (js["head"] > 31).any()      # what the clamps are for
    nonfinite = sum(int((~np.isfinite(c.flat[k])).sum()) for c in cases.values() for k in ("x1", "y1", "x2", "y2"))
    assert nonfinite > 0 and any((c.flat["x2"] == F32(1e30)).any() for c in cases.values())
    # the arena: every region word-aligned, the state 16-byte aligned, guards between
    for c in cases.values():
        assert c.state_off % 16 == 0 and all(lo % 4 == 0 and nb % 4 == 0 for _, lo, nb in c.regions())
        assert (c.want != c.start).any() and c.want[:GUARD_LO(c)].tobytes() == c.start[:GUARD_LO(c)].tobytes()


def GUARD_LO(c):
    return min(lo for _, lo, _ in c.regions())


# ------------------------------------------------------------------------------------------------- without a device; the host glue
def test_trails_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    errs = []
    for call in (lambda: L.ffgpu_trails_reset_dev(None, 1, 1, -1, None),
                 lambda: L.ffgpu_trails_boxes_dev(None, None, 0, None, None, 1, None, None, 1, None, None, None, 0, 0, 0, None),
                 lambda: L.ffgpu_exec_trails(None, 0, None, 1, None, None, 1, None, None, None, 0, 0, 0, None)):
        assert call() < 0
        errs.append(capi.last_error())
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    assert all(want in e for e in errs), errs


def test_host_glue_under_the_sanitizers():
    """san/trails_driver.cc: the state's size, the trails spec's plan and every argument check of ffgpu_trails_host.hpp on the CPU under ASan + UBSan, as
    a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "trails"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_trails_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"trails_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 60, out[-1]
