"""The detections cut out of the frames on the device: ffgpu_crop_boxes_bgr_dev / _nv12_dev and ffgpu_crops_to_source_dev (the operators, on synthetic
records and lists), ffgpu_exec_crop_bgr / _nv12 (behind a forward or a merge of the real net) and the cascade they exist for, against
tests/crops/cropref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  Every comparison is byte for byte over the WHOLE allocation:
sources, output slots and table lie in one arena of seeded random bytes with 64 guard bytes around each, so a byte that should have stayed and did
not is a failure like a wrong pixel.  The seeded cases are built on the CPU (Case), where their statistics are checked too.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the net_input fuzz tests.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from crops import cropref
from test_gpu_round2 import F, boxes_match, net  # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu
BOX = cropref.BOX_DTYPE
GUARD = 64
COUNTS = (0, 1, 2, 127, 128, 129, 300)
SIZES = ((1, 1), (7, 5), (64, 48), (333, 257))
OUTS = ((1, 1), (5, 7), (32, 32), (96, 64))
MARGINS = ((0, 1), (1, 8), (4, 1))
SETTING = ((104.0, 117.0, 123.0), (0.017, 0.0175, 0.0171))
NEEDED = ("down", "up", "same_dword", "same_bytes", "clip_l", "clip_r", "clip_t", "clip_b", "empty", "cut_per_target", "cut_capacity")


class Arena:
    """one host buffer of seeded random bytes, the regions carved out of it with GUARD bytes around each; the same bytes on the device"""

    def __init__(self, rng):
        self.rng, self.size, self.start, self.dev = rng, 0, None, None

    def alloc(self, nbytes, parity=None, align=1):
        """offset of a region of nbytes behind a guard; parity 0 / 1: an even / odd offset; align: a multiple of it (the device base is 256-byte aligned)"""
        off = -(-(self.size + GUARD) // align) * align
        if parity is not None and (off & 1) != parity:
            off += 1
        self.size = off + nbytes
        return off

    def fill(self):
        self.size += GUARD
        self.start = self.rng.integers(0, 256, self.size, dtype=np.uint8)

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.start.copy()).cuda()
        assert self.dev.data_ptr() % 256 == 0
        return self.dev.data_ptr()

    def download(self):
        import torch
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def rand_boxes(rng, n, w, h, ow, oh):
    """n boxes around a w x h source: inside, across an edge, outside or inverted, of exactly the slot's size (not resized), tiny (resized up)"""
    b = np.zeros(n, BOX)
    b["type"] = rng.integers(-2, 7, n)
    b["score"] = rng.uniform(0, 1, n)
    for k in range(n):
        a, c = sorted(int(v) for v in rng.integers(0, w, 2))
        t, d = sorted(int(v) for v in rng.integers(0, h, 2))
        kind = rng.random()
        if kind < 0.25 and ow <= w and oh <= h:                                      # the slot's own size: s1 == s2
            a, t = int(rng.integers(0, w - ow + 1)), int(rng.integers(0, h - oh + 1))
            c, d = a + ow - 1, t + oh - 1
        elif kind < 0.35:                                                            # tiny
            c, d = min(a + int(rng.integers(0, 3)), w - 1), min(t + int(rng.integers(0, 3)), h - 1)
        x1, y1, x2, y2 = a + rng.uniform(0, 0.99), t + rng.uniform(0, 0.99), c + rng.uniform(0, 0.99), d + rng.uniform(0, 0.99)
        if 0.35 <= kind < 0.55:                                                      # one or two corners pushed out
            side = int(rng.integers(0, 6))
            if side in (0, 4):
                x1 = -rng.uniform(1, w + 2)
            if side in (1, 5):
                y1 = -rng.uniform(1, h + 2)
            if side in (2, 5):
                x2 = w + rng.uniform(0, w + 2)
            if side in (3, 4):
                y2 = h + rng.uniform(0, h + 2)
        elif 0.55 <= kind < 0.65:                                                    # moved out as a whole, or inverted
            if rng.random() < 0.5:
                x1, x2 = x2 + 1, x1
            else:
                dx, dy = ((w + rng.uniform(0, 40), 0), (-(w + rng.uniform(1, 40)), 0), (0, h + rng.uniform(0, 40)), (0, -(h + rng.uniform(1, 40))))[int(rng.integers(0, 4))]
                x1, x2, y1, y2 = x1 + dx, x2 + dx, y1 + dy, y2 + dy
        b[k]["x1"], b[k]["y1"], b[k]["x2"], b[k]["y2"] = x1, y1, x2, y2
    return b


def fixed_boxes(w, h):
    """+-1e30, NaN, inverted and zero-size boxes, NaN and negative scores, a box equal to the source, boxes on the last row and column"""
    nan, big = float("nan"), 1e30
    rows = [(-big, h // 3, big, big), (-big, -big, big, big), (big, big, big, big), (nan, nan, w // 2, h // 2), (w // 2, nan, nan, h - 1),
            (w - 2, 1, 2, h - 2), (2, h - 2, w - 2, 1), (w // 2, h // 2, w // 2, h // 2), (0, 0, w - 1, h - 1), (w - 1, h - 1, w - 1, h - 1),
            (0, h - 1, w - 1, h - 1), (w - 1, 0, w - 1, h - 1), (0, 0, w, h), (-0.99, -0.99, w - 0.01, h - 0.01), (3e9, 1, -3e9, h - 2), (-3e9, 0, 3e9, 0)]
    b = np.zeros(len(rows) + 2, BOX)
    for k, r in enumerate(rows):
        b[k] = (k % 5 - 1, 0.5 + 0.01 * k, r[0], r[1], r[2], r[3])
    b[-2] = (0, nan, 0, 0, w - 1, h - 1)
    b[-1] = (0, -1.0, 0, 0, w - 1, h - 1)
    return b


def records_of(F, lists):
    """the records k_nms would leave beside these full lists"""
    r = np.zeros(len(lists), F.DETS_DTYPE)
    for t, b in enumerate(lists):
        n = len(b)
        r[t]["count"], r[t]["nfull"], r[t]["ncand"] = min(n, 128), n, n
        r[t]["box"][:min(n, 128)] = b[:128]
    return r


def flat_lists(lists, stride):
    flat = np.zeros((len(lists), stride), BOX)
    flat.view(np.uint8)[:] = 0x3C                                               # (slots behind a list hold junk: never read)
    for t, b in enumerate(lists):
        flat[t, :len(b)] = b
    return flat.reshape(-1)


def explain(got, want, regions, what):
    """which region (guards included) differs first"""
    if got.tobytes() == want.tobytes():
        return
    bad = np.nonzero(got != want)[0]
    for name, lo, hi in regions:
        hit = bad[(bad >= lo - GUARD) & (bad < hi + GUARD)]
        if len(hit):
            pytest.fail("%s: %s: %d bytes differ, first at region offset %d (region of %d bytes): got %d, want %d"
                        % (what, name, len(hit), int(hit[0]) - lo, hi - lo, got[hit[0]], want[hit[0]]), pytrace=False)
    pytest.fail("%s: %d bytes differ outside every region, first at %d" % (what, len(bad), int(bad[0])), pytrace=False)


def bgr_bytes(w, h, pitch):
    return pitch * (h - 1) + 3 * w


def view(buf, off, shape, strides):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=shape, strides=strides, writeable=False)


class Case:
    """one call of an operator, built on the CPU: the arena's bytes, the sources, the lists, the spec, and what cropref makes of them"""

    def __init__(self, rng, nv12, specs, lists, spec, capacity, use_records=False, first_given=False, what="", patch=None):
        self.nv12, self.specs, self.lists, self.spec, self.use_records, self.what = nv12, specs, lists, spec, use_records, what
        ar = self.ar = Arena(rng)
        self.offs = []
        for s in specs:
            if s is None:
                self.offs.append(None)
            elif not nv12:                                                        # (w, h, pitch): odd base addresses
                self.offs.append(ar.alloc(bgr_bytes(*s), parity=1))
            else:                                                                 # (w, h, pitch_y, pitch_uv, separate uv plane, matrix)
                w, h, py, puv, sep, _ = s
                uv_bytes = puv * ((h + 1) // 2 - 1) + 2 * ((w + 1) // 2)
                if sep:
                    self.offs.append((ar.alloc(py * (h - 1) + w, parity=int(rng.integers(0, 2))), ar.alloc(uv_bytes, parity=0)))
                else:                                                             # one surface: uv = y + pitch_y h, which must come out even
                    oy = ar.alloc(py * h + uv_bytes, parity=(py * h) & 1)
                    self.offs.append((oy, oy + py * h))
        if patch:
            patch(self)
        self.stride = max(1, max(len(b) for b in lists)) + 3
        order = list(rng.permutation(len(lists))) if first_given else list(range(len(lists)))   # list t lies in slot order[t]
        self.slots_of_lists = [None] * len(lists)
        for t, s in enumerate(order):
            self.slots_of_lists[s] = lists[t]
        self.first = [int(s) * self.stride for s in order] if first_given else None
        read = [b[:128] if use_records else b for b in lists]
        srcs = []
        for s, o in zip(specs, self.offs):
            if s is None:
                srcs.append(None)
            elif nv12:
                srcs.append({"w": s[0], "h": s[1], "nv12": True, "addr": o[0], "pitch": s[2]})
            else:
                srcs.append({"w": s[0], "h": s[1], "nv12": False, "addr": o, "pitch": s[2]})
        total = cropref.select(srcs, read, spec, 1)[0][0]
        self.capacity = max(1, {"below": total - 2, "at": total, "above": total + 3}[capacity]) if isinstance(capacity, str) else capacity
        self.out_off = ar.alloc(self.capacity * cropref.slot_nbytes(spec), align=16)
        self.tab_off = ar.alloc(16 + 48 * self.capacity, align=16)
        ar.fill()
        self.stats = {}
        self.header, self.entries = cropref.select(srcs, read, spec, self.capacity, self.stats)
        pics = []
        for s, o in zip(specs, self.offs):
            if s is None:
                pics.append(None)
            elif nv12:
                w, h, py, puv = s[:4]
                pics.append(cropref.nv12_picture(view(ar.start, o[0], (h, w), (py, 1)), view(ar.start, o[1], ((h + 1) // 2, 2 * ((w + 1) // 2)), (puv, 1)), w, h, s[5]))
            else:
                pics.append(view(ar.start, o, (s[1], s[0], 3), (s[2], 3, 1)))
        self.want = ar.start.copy()
        out = cropref.slots(pics, self.header, self.entries, spec)
        self.want[self.out_off:self.out_off + len(out)] = out
        self.want[self.tab_off:self.tab_off + 16 + 48 * self.capacity] = cropref.table_bytes(self.header, self.entries)

    def run(self, F):
        base = self.ar.upload()
        if self.nv12:
            frames = [None if s is None else (base + o[0], base + o[1] if s[4] else 0, s[0], s[1], s[2], s[3], s[5]) for s, o in zip(self.specs, self.offs)]
        else:
            frames = [None if s is None else (base + o, s[0], s[1], s[2]) for s, o in zip(self.specs, self.offs)]
        sp = self.spec
        cs = F.crop_spec(sp.out_w, sp.out_h, sp.form, sp.per_target, sp.min_score, sp.classes, (sp.num, sp.den), sp.mean, sp.norm)
        d_recs = to_dev(records_of(F, self.lists))
        d_lists = None if self.use_records else to_dev(flat_lists(self.slots_of_lists, self.stride))
        fn = F.crop_boxes_nv12_dev if self.nv12 else F.crop_boxes_bgr_dev
        fn(d_recs.data_ptr(), None if self.use_records else d_lists.data_ptr(), 0 if self.use_records else self.stride, frames, cs,
           base + self.out_off, base + self.tab_off, self.capacity, list_first=self.first)
        got = self.ar.download()
        regions = [("table (%s)" % (self.header,), self.tab_off, self.tab_off + 16 + 48 * self.capacity)]
        n = cropref.slot_nbytes(sp)
        regions += [("slot %d %s" % (k, self.entries[k] if k < self.header[1] else "(none)"), self.out_off + k * n, self.out_off + (k + 1) * n) for k in range(self.capacity)]
        explain(got, self.want, regions, self.what)
        return got


def bgr_cases():
    """every source size x pitch (3 w, ALIGN(3 w, 4), 3 w + 5) as one target each per call; out size, form, list lengths, per_target, capacity and
    margin rotate from call to call"""
    rng = np.random.default_rng(5400)
    specs = [(w, h, p) for w, h in SIZES for p in (3 * w, (3 * w + 3) & ~3, 3 * w + 5)]
    out = []
    for call in range(12):
        ow, oh = OUTS[call % 4]
        form = (call // 4 + call) % 2
        spec = cropref.Spec(ow, oh, form, per_target=(1, 3, 128)[call % 3], min_score=0.2, classes=(None, [1, 1, 0, 1, 1, 1, 1, 0, 1])[call % 2],
                            margin=MARGINS[(call // 2) % 3], mean=SETTING[0] if call % 2 else (0.0,) * 3, norm=SETTING[1] if call % 2 else (1 / 255.0,) * 3)
        lists = [rand_boxes(rng, COUNTS[(k + call) % 7], s[0], s[1], ow, oh) for k, s in enumerate(specs)]

        def patch(case, ow=ow, oh=oh, spec=spec):                                    # the first box of a list: the slot's own size, starting on a dword
            for s, o, b in zip(case.specs, case.offs, case.lists):
                if len(b) and spec.num == 0 and s[2] % 4 == 0 and 4 <= ow <= s[0] - 3 and oh <= s[1] - 3:
                    x = [x for x in range(4) if (o + 3 * x) % 4 == 0][0]
                    b[0] = (0, 0.9, x, x, x + ow - 1 + 0.5, x + oh - 1 + 0.5)
        out.append(Case(rng, False, specs, lists, spec, ("below", "at", "above")[call % 3], patch=patch, use_records=call % 4 == 3, first_given=call % 4 == 1,
                        what="bgr call %d: out %d x %d form %d" % (call, ow, oh, form)))
    return out


def nv12_cases():
    """odd and even sizes, separate and contiguous UV planes, padded pitches, all four matrices"""
    rng = np.random.default_rng(5410)
    specs = []
    for k, (w, h) in enumerate(((1, 1), (7, 5), (63, 47), (64, 48), (333, 257))):
        mu = 2 * ((w + 1) // 2)
        specs += [(w, h, w, mu, False, k % 4), (w, h, (w + 3) & ~3, mu + 6, True, (k + 1) % 4), (w, h, w + 5, mu + 2, False, (k + 2) % 4), (w, h, (w + 11) & ~3, mu, True, (k + 3) % 4)]
    out = []
    for call in range(8):
        ow, oh = OUTS[call % 4]
        form = (call // 4 + call) % 2
        spec = cropref.Spec(ow, oh, form, per_target=(3, 128, 1)[call % 3], min_score=0.1, margin=MARGINS[call % 3], mean=SETTING[0], norm=SETTING[1])
        lists = [rand_boxes(rng, COUNTS[(k + call) % 7], s[0], s[1], ow, oh) for k, s in enumerate(specs)]
        out.append(Case(rng, True, specs, lists, spec, ("above", "below", "at")[call % 3], first_given=call % 4 == 2, what="nv12 call %d: out %d x %d form %d" % (call, ow, oh, form)))
    return out


def many_target_cases():
    """ntargets 1, 64, 65, 130 (a launch's arguments hold 64), some skipped"""
    rng = np.random.default_rng(5420)
    out = []
    for k, nt in enumerate((1, 64, 65, 130)):
        specs = [None if (t % 7 == 3 and nt > 1) else (16 + t % 5, 12 + t % 3, 3 * (16 + t % 5) + (t % 4)) for t in range(nt)]
        lists = [rand_boxes(rng, int(rng.integers(0, 6)), 16, 12, 8, 8) for _ in range(nt)]
        spec = cropref.Spec(8, 8, k % 2, per_target=2, min_score=0.1, margin=(1, 8))
        out.append(Case(rng, False, specs, lists, spec, ("above", "below", "at", "below")[k], first_given=nt == 130, what="%d targets" % nt))
    return out


_CASES = {}


def cases(name):
    if name not in _CASES:
        _CASES[name] = {"bgr": bgr_cases, "nv12": nv12_cases, "many": many_target_cases}[name]()
    return _CASES[name]


def summed(cs):
    total = {}
    for c in cs:
        for k, v in c.stats.items():
            total[k] = total.get(k, 0) + v
    return total


# ---------------------------------------------------------------------------------------------------------------- 1. the operators against cropref
def test_seeded_set_covers_every_path():
    """the reference run of the seeded set (CPU only): every path and edge case the contract names occurs in it"""
    bgr, nv, many = summed(cases("bgr")), summed(cases("nv12")), summed(cases("many"))
    print("bgr %s\nnv12 %s\nmany %s" % (bgr, nv, many))
    for st in (bgr, nv):
        for key in NEEDED:
            assert st.get(key, 0) > 0, (key, st)
    assert nv.get("odd_x", 0) > 0 and nv.get("odd_y", 0) > 0, nv
    assert many.get("cut_capacity", 0) > 0 and many.get("cut_per_target", 0) > 0, many


@pytest.mark.parametrize("call", range(12))
def test_operator_bgr(F, call):
    cases("bgr")[call].run(F)


@pytest.mark.parametrize("call", range(8))
def test_operator_nv12(F, call):
    cases("nv12")[call].run(F)


@pytest.mark.parametrize("k", range(4))
def test_operator_many_targets(F, k):
    cases("many")[k].run(F)


@pytest.mark.parametrize("nv12", [False, True])
def test_operator_fixed_boxes(F, nv12):
    """NaN corners and scores, +-1e30, inverted and one-pixel boxes, with every margin; run twice into the same buffers: the same bytes"""
    rng = np.random.default_rng(5430)
    for m, margin in enumerate(MARGINS):
        specs = [(64, 48, 65, 66, True, 1), (7, 5, 7, 8, False, 2), (333, 257, 336, 340, True, 3)] if nv12 else [(64, 48, 3 * 64 + 5), (7, 5, 21), (333, 257, 1000)]
        lists = [fixed_boxes(s[0], s[1]) for s in specs]
        spec = cropref.Spec(32, 32, m % 2, per_target=128, min_score=0.0, margin=margin)
        c = Case(rng, nv12, specs, lists, spec, "at", what="fixed boxes, margin %d / %d" % margin)
        assert c.stats["empty"] >= 9 and c.header[0] >= 18, (c.stats, c.header)
        a = c.run(F)
        assert c.run(F).tobytes() == a.tobytes()


def test_operator_counts_are_clamped(F):
    """records whose count / nfull is negative or beyond the stride select from the clamped number and nothing is read behind it"""
    rng = np.random.default_rng(5440)
    w, h, pitch, stride = 64, 48, 200, 40
    for use_records in (False, True):
        cap = 128 if use_records else stride
        lists = [rand_boxes(rng, cap, w, h, 32, 32) for _ in range(4)]
        claimed = (-1, -2 ** 31, cap + 1, 2 ** 31 - 1)
        c = Case(rng, False, [(w, h, pitch)] * 4, [lists[t][:0] if claimed[t] < 0 else lists[t] for t in range(4)], cropref.Spec(32, 32, 1, per_target=128, min_score=0.5), "above",
                 use_records=use_records, what="clamped counts, records %s" % use_records)
        base = c.ar.upload()
        recs = records_of(F, lists)
        for t, v in enumerate(claimed):
            recs[t]["count" if use_records else "nfull"] = v
            recs[t]["nfull" if use_records else "count"] = 7                     # (the other field is not the one that is read)
        d_recs = to_dev(recs)
        d_lists = None if use_records else to_dev(flat_lists(lists, stride))
        F.crop_boxes_bgr_dev(d_recs.data_ptr(), None if use_records else d_lists.data_ptr(), 0 if use_records else stride, [(base + o, w, h, pitch) for o in c.offs],
                             F.crop_spec(32, 32, 1, 128, 0.5), base + c.out_off, base + c.tab_off, c.capacity)
        explain(c.ar.download(), c.want, [("table", c.tab_off, c.tab_off + 16 + 48 * c.capacity), ("slots", c.out_off, c.tab_off - GUARD)], c.what)
        assert d_recs.cpu().numpy().tobytes() == recs.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. against what exists
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


def test_f32_slot_is_the_staged_input_of_the_same_region(F, net, picture):
    """BGR sources: an F32 slot == read_layer(-1) of a FFGPU_KEEP_ALL executor given the same region as a host descriptor through
    forward_bgr_frames_dev, bit for bit (resized down, up, and the picture itself)"""
    import torch
    pitch = 3 * 640 + 4
    buf = np.zeros((424, pitch), np.uint8)
    buf[:, :1920] = picture.reshape(424, 1920)
    dev = torch.from_numpy(buf).cuda()
    boxes = np.zeros(4, BOX)
    for k, r in enumerate(((0, 0, 639, 423), (101, 37, 420, 356), (333, 100, 340, 111), (7, 200, 600, 260))):
        boxes[k] = (0, 0.9, r[0], r[1], r[2], r[3])
    d_recs = to_dev(records_of(F, [boxes]))
    frame = (dev.data_ptr(), 640, 424, pitch)
    for setting in (((0.0, 0.0, 0.0), (1 / 255.0,) * 3), SETTING):
        out = torch.full((4 * 3 * 320 * 320,), float("nan"), dtype=torch.float32, device="cuda")
        tab = torch.zeros(16 + 48 * 4, dtype=torch.uint8, device="cuda")
        F.crop_boxes_bgr_dev(d_recs.data_ptr(), None, 0, [frame], F.crop_spec(320, 320, F.CROP_F32, per_target=4, mean=setting[0], norm=setting[1]), out.data_ptr(), tab.data_ptr(), 4)
        torch.cuda.synchronize()
        hdr, ent = F.crop_table(tab.cpu().numpy())
        assert hdr == dict(total=4, taken=4, empty=0, capacity=4)
        got = out.cpu().numpy().reshape(4, 3, 320, 320)
        with net.executor(4, F.FFGPU.KEEP_ALL) as ex:
            ex.forward_bgr_frames_dev([(dev.data_ptr() + int(e["y0"]) * pitch + 3 * int(e["x0"]), int(e["w"]), int(e["h"]), pitch) for e in ent], *setting)
            for n in range(4):
                assert got[n].tobytes() == ex.read_layer(-1, n).tobytes(), (n, ent[n])


# ---------------------------------------------------------------------------------------------------------------- 3. map back
def test_map_back_against_cropref(F):
    """synthetic records and lists, NaN and +-1e30 coordinates, counts beyond their clamps; out of place and in place; slots >= taken zeroed"""
    import torch
    rng = np.random.default_rng(5450)
    cap, stride = 9, 140
    srcs = [{"w": 640, "h": 424}, {"w": 33, "h": 1000}]
    sel = [np.zeros(4, BOX), np.zeros(3, BOX)]
    for b in sel:
        for k in range(len(b)):
            b[k] = (1, 0.9, rng.uniform(0, 20), rng.uniform(0, 200), rng.uniform(20, 33), rng.uniform(200, 420))
    hdr, ent = cropref.select(srcs, sel, cropref.Spec(96, 64, per_target=4, margin=(1, 8)), cap)
    assert hdr[1] == 7
    lists = [rand_boxes(rng, n, 96, 64, 32, 32) for n in (0, 1, 127, 128, 129, 140, 5, 77, 140)]
    lists[2][3]["x1"], lists[2][4]["y2"], lists[2][5]["x2"], lists[2][6]["y1"] = np.nan, 1e30, -1e30, np.inf
    recs = records_of(F, lists)
    recs[3]["count"], recs[4]["nfull"], recs[5]["count"], recs[6]["nfull"] = 2 ** 31 - 1, 2 ** 31 - 1, -5, -2 ** 31
    flat = flat_lists(lists, stride)
    d_tab = to_dev(cropref.table_bytes(hdr, ent))
    junk = rng.integers(0, 256, flat.nbytes, dtype=np.uint8)

    def same(got, want, what):
        g, w = got.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)
        gf, wf = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
        ok = (g == w) | (np.isnan(gf) & np.isnan(wf))                             # (NaNs as NaN, not by payload)
        assert ok.all(), "%s: %d words differ, first at %d" % (what, (~ok).sum(), int(np.nonzero(~ok)[0][0]))
    for with_lists in (False, True):
        want_r, want_l = cropref.map_back(hdr, ent, recs, flat if with_lists else None, stride, junk.view(BOX) if with_lists else None)
        # out of place: guards around the outputs
        ar = Arena(rng)
        ro, lo = ar.alloc(recs.nbytes, align=16), ar.alloc(flat.nbytes, align=16)
        ar.fill()
        ar.start[lo:lo + flat.nbytes] = junk
        base = ar.upload()
        d_recs, d_lists = to_dev(recs), to_dev(flat)
        F.crops_to_source_dev(d_tab.data_ptr(), cap, d_recs.data_ptr(), d_lists.data_ptr() if with_lists else None, stride, base + ro, base + lo if with_lists else None)
        got = ar.download()
        same(got[ro:ro + recs.nbytes], want_r.view(np.uint8).reshape(-1), "records, lists %s" % with_lists)
        if with_lists:
            same(got[lo:lo + flat.nbytes], want_l.view(np.uint8).reshape(-1), "lists")
        keep = np.ones(len(got), bool)
        keep[ro:ro + recs.nbytes] = False
        if with_lists:
            keep[lo:lo + flat.nbytes] = False
        assert (got[keep] == ar.start[keep]).all()
        assert d_recs.cpu().numpy().tobytes() == recs.tobytes() and d_lists.cpu().numpy().tobytes() == flat.tobytes()
        assert not got[ro + 7 * recs.itemsize:ro + recs.nbytes].any()               # slots >= taken
        # in place
        want_r, want_l = cropref.map_back(hdr, ent, recs, flat if with_lists else None, stride, flat if with_lists else None)
        F.crops_to_source_dev(d_tab.data_ptr(), cap, d_recs.data_ptr(), d_lists.data_ptr() if with_lists else None, stride, d_recs.data_ptr(), d_lists.data_ptr() if with_lists else None)
        torch.cuda.synchronize()
        same(d_recs.cpu().numpy(), want_r.view(np.uint8).reshape(-1), "in place, records")
        if with_lists:
            same(d_lists.cpu().numpy(), want_l.view(np.uint8).reshape(-1), "in place, lists")


# ---------------------------------------------------------------------------------------------------------------- 4. executor forms and the cascade
def picture_on_device(picture, pad=4):
    import torch
    h, w = picture.shape[:2]
    buf = np.zeros((h, 3 * w + pad), np.uint8)
    buf[:, :3 * w] = picture.reshape(h, 3 * w)
    return torch.from_numpy(buf).cuda(), 3 * w + pad


def crop_buffers(spec, capacity):
    import torch
    out = torch.full((capacity * cropref.slot_nbytes(spec),), 0xA5, dtype=torch.uint8, device="cuda")
    tab = torch.full((16 + 48 * capacity,), 0xA5, dtype=torch.uint8, device="cuda")
    return out, tab


def check_against_cropref(out, tab, srcs, pics, lists, spec, capacity, what):
    import torch
    torch.cuda.synchronize()
    hdr, ent = cropref.select(srcs, lists, spec, capacity)
    assert tab.cpu().numpy().tobytes() == cropref.table_bytes(hdr, ent).tobytes(), what + ": table"
    assert out.cpu().numpy().tobytes() == cropref.slots(pics, hdr, ent, spec).tobytes(), what + ": slots"
    return hdr, ent


def as_image(pix):
    h, w = pix.shape[:2]
    rows = np.zeros((h, cropref.align4(3 * w)), np.uint8)
    rows[:, :3 * w] = pix.reshape(h, 3 * w)
    return rows


def test_cascade(F, net, orc, picture):
    """executor 1 on data/test.bmp -> ffgpu_exec_crop_bgr (F32, 320 x 320, margin 1 / 8, capacity 4) -> executor 2 (batch 4, forward_dev) ->
    ffgpu_crops_to_source_dev.  Against the host round trip (the same regions as host descriptors through forward_bgr_frames_dev on executor 2,
    translated on the host), byte for byte; against the oracle's run of each region, within 0.05 px / 1e-4; against cropref; then the U8 form
    through forward_bgr_dev"""
    import torch
    dev, pitch = picture_on_device(picture)
    frame = (dev.data_ptr(), 640, 424, pitch)
    spec = cropref.Spec(320, 320, cropref.F32, per_target=4, min_score=0.0, margin=(1, 8))
    with net.executor(1) as ex1, net.executor(4) as ex2:
        ex1.forward_bgr_frames_dev([frame])
        dets1, boxes1, caps = ex1.read_dets().tobytes(), ex1.read_boxes(0), ex1.graph_captures
        assert len(boxes1) == 3
        out, tab = crop_buffers(spec, 4)
        ex1.crop_bgr([frame], F.crop_spec(320, 320, F.CROP_F32, per_target=4, margin=(1, 8)), out.data_ptr(), tab.data_ptr(), 4)
        hdr, ent = check_against_cropref(out, tab, [{"w": 640, "h": 424}], [picture], [boxes1], spec, 4, "cascade F32")
        assert hdr == (3, 3, 0, 4)
        assert ex1.graph_captures == caps and ex1.read_dets().tobytes() == dets1 and ex1.read_boxes(0).tobytes() == boxes1.tobytes()
        # executor 2 on the slots, mapped back on the device
        ex2.forward_dev(out.data_ptr())
        recs2 = ex2.read_dets()
        lists2 = [ex2.read_boxes(n) for n in range(4)]
        d_recs, _ = ex2.dets_dev()
        mapped = torch.zeros(recs2.nbytes, dtype=torch.uint8, device="cuda")
        F.crops_to_source_dev(tab.data_ptr(), 4, d_recs, None, 0, mapped.data_ptr())
        torch.cuda.synchronize()
        mapped = mapped.cpu().numpy().view(F.DETS_DTYPE)
        want, _ = cropref.map_back(hdr, ent, recs2)
        assert mapped.tobytes() == want.tobytes()
        assert mapped[3].tobytes() == bytes(F.DETS_DTYPE.itemsize)
        assert sum(int(r["count"]) for r in mapped[:3]) >= 3
        # the host round trip: the same regions as host descriptors (slot 3: one black pixel, a zero frame), translated in fp32 on the host
        black = torch.zeros(4, dtype=torch.uint8, device="cuda")
        regions = [(dev.data_ptr() + int(e["y0"]) * pitch + 3 * int(e["x0"]), int(e["w"]), int(e["h"]), pitch) for e in ent[:3]] + [(black.data_ptr(), 1, 1, 4)]
        ex2.forward_bgr_frames_dev(regions)
        trip = ex2.read_dets()
        for n in range(3):
            assert trip[n]["count"] == mapped[n]["count"] and trip[n]["nfull"] == mapped[n]["nfull"] and trip[n]["ncand"] == mapped[n]["ncand"]
            moved = trip[n]["box"].copy()
            k = int(trip[n]["count"])
            for c, o in (("x1", "x0"), ("y1", "y0"), ("x2", "x0"), ("y2", "y0")):
                moved[c][:k] = trip[n]["box"][c][:k] + np.float32(int(ent[n][o]))
            assert moved.tobytes() == mapped[n]["box"].tobytes(), "slot %d: device crop and host round trip differ" % n
            assert ex2.read_boxes(n).tobytes() != b"" and len(lists2[n]) == int(mapped[n]["nfull"])
        # the oracle's run of each region, copied out as an image of its own
        o = orc.Oracle()
        try:
            for n in range(3):
                e = ent[n]
                x0, y0, w, h = (int(e[f]) for f in ("x0", "y0", "w", "h"))
                o.set_input_image(as_image(picture[y0:y0 + h, x0:x0 + w]), w, h)
                o.forward()
                ob = o.boxes
                for c, off in (("x1", x0), ("y1", y0), ("x2", x0), ("y2", y0)):
                    ob[c] += np.float32(off)
                boxes_match(mapped[n]["box"][:int(mapped[n]["count"])], ob, "slot %d against the oracle" % n)
        finally:
            o.close()
        # the U8 form (mean 0 keeps the letterbox remainder at zero) through forward_bgr_dev
        spec8 = cropref.Spec(320, 320, cropref.U8, per_target=4, min_score=0.0, margin=(1, 8))
        out8, tab8 = crop_buffers(spec8, 4)
        ex1.crop_bgr([frame], F.crop_spec(320, 320, F.CROP_U8, per_target=4, margin=(1, 8)), out8.data_ptr(), tab8.data_ptr(), 4)
        check_against_cropref(out8, tab8, [{"w": 640, "h": 424}], [picture], [boxes1], spec8, 4, "cascade U8")
        ex2.forward_bgr_dev(out8.data_ptr(), 320, 320)
        recs8 = ex2.read_dets()
        for n in range(4):
            boxes_match(recs8[n]["box"][:int(recs8[n]["count"])], recs2[n]["box"][:int(recs2[n]["count"])], "U8 slot %d" % n)


def four_frames(picture):
    rng = np.random.default_rng(5460)
    out = [picture]
    for _ in range(3):
        x0, y0 = int(rng.integers(0, 60)), int(rng.integers(0, 40))
        out.append(picture[y0:424 - int(rng.integers(0, 40)), x0:640 - int(rng.integers(0, 60))])
    return [np.ascontiguousarray(f) for f in out]


@pytest.mark.parametrize("flags", [0, 32])
def test_exec_crop_entries(F, net, picture, flags):
    """batch 4 (flags 32: FFGPU_SPLIT2): the array handed to the forward, one source skipped; the records, lists and the captured graph stay"""
    imgs = four_frames(picture)
    devs = [picture_on_device(im, pad=1 + k) for k, im in enumerate(imgs)]
    frames = [(d.data_ptr(), im.shape[1], im.shape[0], p) for (d, p), im in zip(devs, imgs)]
    spec = cropref.Spec(96, 64, cropref.U8, per_target=2, min_score=0.3, margin=(1, 8))
    with net.executor(4, flags) as ex:
        ex.forward_bgr_frames_dev(frames)
        dets, boxes, caps = ex.read_dets().tobytes(), [ex.read_boxes(t) for t in range(4)], ex.graph_captures
        assert all(len(b) > 0 for b in boxes)
        out, tab = crop_buffers(spec, 7)
        ex.crop_bgr(frames[:1] + [None] + frames[2:], F.crop_spec(96, 64, F.CROP_U8, per_target=2, min_score=0.3, margin=(1, 8)), out.data_ptr(), tab.data_ptr(), 7)
        srcs = [None if t == 1 else {"w": im.shape[1], "h": im.shape[0]} for t, im in enumerate(imgs)]
        hdr, _ = check_against_cropref(out, tab, srcs, imgs, boxes, spec, 7, "exec entries, flags %d" % flags)
        assert 3 <= hdr[1] <= 6
        assert ex.graph_captures == caps and ex.read_dets().tobytes() == dets and all(ex.read_boxes(t).tobytes() == boxes[t].tobytes() for t in range(4))


def test_exec_crop_nv12_and_merged(F, net, picture):
    """NV12 frames through ffgpu_exec_crop_nv12; FFGPU_CROP_MERGED behind a two-tile merge of a 1280 x 424 picture"""
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    Y, UV = bgr_to_nv12(picture[3:420, 5:636])
    dY, dUV = torch.from_numpy(Y).cuda(), torch.from_numpy(UV).cuda()
    h, w = Y.shape
    spec = cropref.Spec(32, 32, cropref.F32, per_target=8, min_score=0.0, margin=(1, 8), mean=SETTING[0], norm=SETTING[1])
    cs = F.crop_spec(32, 32, F.CROP_F32, per_target=8, margin=(1, 8), mean=SETTING[0], norm=SETTING[1])
    with net.executor(1) as ex:
        ex.forward_nv12_frames_dev([(dY, dUV)], matrix=2)
        boxes = ex.read_boxes(0)
        assert len(boxes) > 0
        out, tab = crop_buffers(spec, 4)
        ex.crop_nv12([(dY, dUV)], cs, out.data_ptr(), tab.data_ptr(), 4, matrix=2)
        check_against_cropref(out, tab, [{"w": w, "h": h}], [cropref.nv12_picture(Y, UV, w, h, 2)], [boxes], spec, 4, "exec nv12")
    wide = np.ascontiguousarray(np.concatenate([picture, picture[:, ::-1]], axis=1))
    dev, pitch = picture_on_device(wide, pad=7)
    plan = F.tile_plan(1280, 424, 640, 424, 0, 0, 1)
    assert len(plan) == 2
    frames = [(dev.data_ptr() + y0 * pitch + 3 * x0, tw, th, pitch) for x0, y0, tw, th in plan]
    whole = [(dev.data_ptr(), 1280, 424, pitch)]
    with net.executor(2) as ex:
        ex.forward_bgr_frames_dev(frames)
        out, tab = crop_buffers(spec, 8)
        with pytest.raises(RuntimeError, match="no ffgpu_exec_merge_tiles has run"):
            ex.crop_bgr(whole, cs, out.data_ptr(), tab.data_ptr(), 8, which=F.CROP_MERGED)
        ex.merge_tiles([(0, x0, y0) for x0, y0, _, _ in plan], 1)
        merged, lists = ex.read_merged(1).tobytes(), [ex.read_merged_boxes(0)]
        assert len(lists[0]) >= 4
        ex.crop_bgr(whole, cs, out.data_ptr(), tab.data_ptr(), 8, which=F.CROP_MERGED)
        hdr, _ = check_against_cropref(out, tab, [{"w": 1280, "h": 424}], [wide], lists, spec, 8, "exec merged")
        assert hdr[1] >= 4 and ex.read_merged(1).tobytes() == merged and ex.graph_captures == 1


def test_rejections(F, net, picture):
    """every rejected argument with its message, the target's index where there is one; nothing is written by a rejected call, and the next valid call
    on the same executor equals cropref"""
    import torch
    dev, pitch = picture_on_device(picture)
    frame = (dev.data_ptr(), 640, 424, pitch)
    L = F.lib()
    spec = cropref.Spec(32, 32, cropref.U8, per_target=4)
    out, tab = crop_buffers(spec, 4)
    o, t = out.data_ptr(), tab.data_ptr()
    cls = (C.c_ubyte * 4)(1, 1, 1, 1)

    def sp(**kw):
        s = F.crop_spec(32, 32, F.CROP_U8, per_target=4)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    good = sp()
    with net.executor(1) as ex:
        ex.forward_bgr_frames_dev([frame])
        boxes = ex.read_boxes(0)
        ftab = F.bgr_frame_table([frame])
        nv = F.nv12_frame_table([(dev.data_ptr(), 0, 64, 48)])
        d_recs, _ = ex.dets_dev()

        def both(frames, n, s, oo, tt, cap, msg, which=0, nv12_too=True):
            calls = [lambda: L.ffgpu_exec_crop_bgr(ex.h, which, frames, n, s, oo, tt, cap, None)]
            if which == 0:
                calls.append(lambda: L.ffgpu_crop_boxes_bgr_dev(d_recs, None, 0, None, frames, n, s, oo, tt, cap, None))
            if nv12_too:
                calls.append(lambda: L.ffgpu_exec_crop_nv12(ex.h, which, None if frames is None else nv, n, s, oo, tt, cap, None))
            for c in calls:
                assert c() < 0
                assert re.search(msg, F.last_error()), (msg, F.last_error())
        both(None, 1, good, o, t, 4, "NULL targets")
        both(ftab, 1, None, o, t, 4, "NULL spec")
        both(ftab, 1, good, None, t, 4, "NULL output")
        both(ftab, 1, good, o, None, 4, "NULL table")
        both(ftab, 1, good, o, t, 0, "capacity 0")
        both(ftab, 1, good, o + 4, t, 4, "16-byte aligned")
        both(ftab, 1, good, o, t + 8, 4, "16-byte aligned")
        for kw, msg in ((dict(out_w=0), "out size"), (dict(out_h=4097), "out size"), (dict(form=2), "form 2"), (dict(per_target=0), "per_target 0"),
                        (dict(per_target=2 ** 24 + 1), "per_target"), (dict(nclasses=3), "nclasses 3"), (dict(classes=C.addressof(cls), nclasses=0), "nclasses 0"),
                        (dict(classes=C.addressof(cls), nclasses=257), "nclasses 257"), (dict(margin_den=0), "margin"), (dict(margin_den=1025), "margin"),
                        (dict(margin_num=-1), "margin"), (dict(margin_num=5, margin_den=1), "margin"), (dict(reserved=1), "reserved")):
            both(ftab, 1, sp(**kw), o, t, 4, msg)
        both(ftab, 1, good, o, t, 4, "which = 2", which=2)
        both(ftab, 1, good, o, t, 4, "no ffgpu_exec_merge_tiles has run", which=1)
        assert L.ffgpu_exec_crop_bgr(ex.h, 0, ftab, 2, good, o, t, 4, None) < 0 and "2 targets for an executor of batch 1" in F.last_error()
        assert L.ffgpu_crop_boxes_bgr_dev(d_recs, None, 0, None, ftab, 0, good, o, t, 4, None) < 0 and "ntargets" in F.last_error()
        assert L.ffgpu_crop_boxes_bgr_dev(None, None, 0, None, ftab, 1, good, o, t, 4, None) < 0 and "NULL records" in F.last_error()
        assert L.ffgpu_crop_boxes_bgr_dev(d_recs, d_recs, 0, None, ftab, 1, good, o, t, 4, None) < 0 and "list_stride" in F.last_error()
        first = (C.c_int * 1)(-5)
        assert L.ffgpu_crop_boxes_bgr_dev(d_recs, d_recs, 8, first, ftab, 1, good, o, t, 4, None) < 0 and "target 0: negative list start" in F.last_error()
        st = torch.cuda.Stream()
        assert L.ffgpu_exec_crop_bgr(ex.h, 0, ftab, 1, good, o, t, 4, st.cuda_stream) < 0 and "stream of the forward" in F.last_error()
        for field, val, msg in (("w", 0, "bad size"), ("h", -3, "bad size"), ("w", 2 ** 31 - 1, "bad size"), ("h", 2 ** 31 - 1, "bad size"), ("reserved", 1, "reserved"), ("pitch", 5, "pitch")):
            bad = F.bgr_frame_table([frame])
            setattr(bad[0], field, val)
            both(bad, 1, good, o, t, 4, "target 0: .*%s" % msg, nv12_too=False)
        for field, val, msg in (("w", 0, "bad size"), ("h", 2 ** 31 - 1, "bad size"), ("matrix", 4, "matrix"), ("reserved", 1, "reserved"), ("pitch_y", 5, "pitch_y"),
                                ("pitch_uv", 63, "pitch_uv"), ("uv", dev.data_ptr() + 1, "odd")):
            bad = F.nv12_frame_table([(dev.data_ptr(), 0, 64, 48)])
            setattr(bad[0], field, val)
            assert L.ffgpu_exec_crop_nv12(ex.h, 0, bad, 1, good, o, t, 4, None) < 0 and re.search("target 0: .*%s" % msg, F.last_error()), F.last_error()
            assert L.ffgpu_crop_boxes_nv12_dev(d_recs, None, 0, None, bad, 1, good, o, t, 4, None) < 0 and re.search("target 0: .*%s" % msg, F.last_error()), F.last_error()
        for call, msg in ((lambda: L.ffgpu_crops_to_source_dev(None, 4, d_recs, None, 0, d_recs, None, None), "NULL table"),
                          (lambda: L.ffgpu_crops_to_source_dev(t, 4, None, None, 0, d_recs, None, None), "NULL records"),
                          (lambda: L.ffgpu_crops_to_source_dev(t, 4, d_recs, None, 0, None, None, None), "NULL records"),
                          (lambda: L.ffgpu_crops_to_source_dev(t, 0, d_recs, None, 0, d_recs, None, None), "capacity 0"),
                          (lambda: L.ffgpu_crops_to_source_dev(t + 4, 4, d_recs, None, 0, d_recs, None, None), "16-byte aligned"),
                          (lambda: L.ffgpu_crops_to_source_dev(t, 4, d_recs, d_recs, 0, d_recs, None, None), "list_stride")):
            assert call() < 0 and msg in F.last_error(), (msg, F.last_error())
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xA5).all() and (tab.cpu().numpy() == 0xA5).all()        # nothing was launched
        ex.crop_bgr([frame], good, o, t, 4)                                               # the executor is still usable
        check_against_cropref(out, tab, [{"w": 640, "h": 424}], [picture], [boxes], spec, 4, "after the rejections")
        assert ex.graph_captures == 1
