"""The outlines contract of include/ffcnn_hip.h restated in numpy: the segment primitive (segment items drawn serially in slot order into u8 BGR and
NV12 surfaces, the NV12 chroma rule) and the scene composer (the zones' edges, the lines' shafts and forward ticks, the anchors' crosses as items,
from tests/zones/zoneref.py's structures).  All geometry is Python / int64 integer arithmetic; `//` is the floor toward -infinity the contract names.
The GPU tests compare the device's bytes with this; tests/test_outlines_abi.py pins this to the per-pixel inequality, to the literal column loop and
to the stated properties."""
import numpy as np

from zones.zoneref import SCENE_DTYPE, SLOT_DTYPE, STATE_HEADER  # noqa: F401  (the scenes' and the state's layouts)
from captions.textref import f2i  # noqa: F401  (the draw contract's conversion)

SEG_ITEMS, SEG_LIMIT, FIXED = 512, 1 << 20, 80
ZONES, LINES, TICKS, MARKERS, ALARM = 1, 2, 4, 8, 16
ITEM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("color", "u1", (4,)), ("thickness", "u1"), ("dash", "u1"), ("flags", "u1"),
                       ("reserved", "u1"), ("reserved2", "<i4", (2,))])
assert ITEM_DTYPE.itemsize == 32
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


class Spec:
    """ffgpu_outline_spec: palette None or a sequence of colours"""

    def __init__(self, flags=ZONES | LINES, thickness=1, line_dash=0, marker=0, color=(0, 0, 0), alarm=(0, 0, 255), palette=None):
        self.flags, self.thickness, self.line_dash, self.marker = flags, thickness, line_dash, marker
        self.color, self.alarm = tuple(color[:3]), tuple(alarm[:3])
        self.palette = None if palette is None else [tuple(c[:3]) for c in palette]

    def paint(self, index):
        return self.color if self.palette is None else self.palette[index % len(self.palette)]


# ---------------------------------------------------------------------------------------------------------------- the primitive
def canon(item):
    """the item's set-up: None when it draws nothing, else (ymajor, Sm, Sn, D, g, T, d) -- S's major and minor coordinate, Python ints"""
    x0, y0, x1, y1 = (int(item[f]) for f in ("x0", "y0", "x1", "y1"))
    T, d = min(int(item["thickness"]), 8), min(int(item["dash"]), 6)
    if T == 0 or max(abs(x0), abs(y0), abs(x1), abs(y1)) > SEG_LIMIT:
        return None
    ym = abs(x1 - x0) < abs(y1 - y0)
    a, b = ((y0, x0), (y1, x1)) if ym else ((x0, y0), (x1, y1))
    if b[0] < a[0]:
        a, b = b, a
    return ym, a[0], a[1], b[0] - a[0], b[1] - a[1], T, d


def pixels(item, w, h):
    """(xs, ys): the item's pixels inside a w x h target, int64 arrays, every pixel once; by the column form: the major steps clipped to the target, the
    column S.y + floor((2 m g + D) / (2 D)) of each, lo pixels before and hi behind"""
    c = canon(item)
    none = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if c is None:
        return none
    ym, sm, sn, D, g, T, d = c
    wm, wn = (h, w) if ym else (w, h)
    mlo, mhi = max(0, -sm), min(D, wm - 1 - sm)
    if mlo > mhi:
        return none
    m = np.arange(mlo, mhi + 1, dtype=np.int64)
    if d:
        m = m[((m >> d) & 1) == 0]
    col = sn + ((2 * m * g + D) // (2 * D) if D else np.zeros(len(m), np.int64))
    lo, hi = (T - 1) // 2, T // 2
    M = np.repeat(sm + m, T)
    N = (col[:, None] + np.arange(-lo, hi + 1, dtype=np.int64)[None, :]).reshape(-1)
    keep = (N >= 0) & (N < wn)
    M, N = M[keep], N[keep]
    return (N, M) if ym else (M, N)


def draw_bgr(buf, off, w, h, pitch, items):
    """the items drawn serially in slot order into the BGR surface at byte `off` of the flat uint8 array `buf`, rows `pitch` bytes apart"""
    for it in items:
        xs, ys = pixels(it, w, h)
        at = off + ys * pitch + 3 * xs
        for c in range(3):
            buf[at + c] = it["color"][c]


def draw_nv12(buf, y_off, uv_off, w, h, pitch_y, pitch_uv, items):
    """the same into an NV12 surface: a written pixel sets its Y byte; a chroma pair any of whose luma pixels the item writes takes the item's (U, V).
    Serially in slot order: the last such item decides."""
    for it in items:
        xs, ys = pixels(it, w, h)
        buf[y_off + ys * pitch_y + xs] = it["color"][0]
        at = uv_off + (ys >> 1) * pitch_uv + 2 * (xs >> 1)
        buf[at] = it["color"][1]
        buf[at + 1] = it["color"][2]


# ---------------------------------------------------------------------------------------------------------------- the composer
def sat(v):
    return min(max(int(v), IMIN), IMAX)


def tdiv(a, b):
    """a / b toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def make_item(x0, y0, x1, y1, color, thickness, dash=0):
    it = np.zeros((), ITEM_DTYPE)
    it["x0"], it["y0"], it["x1"], it["y1"], it["thickness"], it["dash"] = sat(x0), sat(y0), sat(x1), sat(y1), thickness, dash
    it["color"][:3] = color
    return it


def zone_draws(zn):
    nv = int(zn["nverts"])
    return 3 <= nv <= 8 and not (np.isnan(zn["x"][:nv]).any() or np.isnan(zn["y"][:nv]).any())


def tick_ends(ax, ay, bx, by):
    """the forward tick of the line (ax, ay) -> (bx, by), converted integers: (mx, my, ex, ey), not yet saturated"""
    mx, my = (ax + bx) >> 1, (ay + by) >> 1
    return mx, my, mx + tdiv(-(by - ay), 8), my + tdiv(bx - ax, 8)


def seen_slots(hdr_frames, slots):
    """the slots of one stream's state that were seen in the frame before `frames`, in slot order"""
    want = (int(hdr_frames) - 1) % 2 ** 32
    return [q for q in range(len(slots)) if int(slots[q]["id"]) != 0 and int(slots[q]["last"]) % 2 ** 32 == want]


def outline_scene(scenes, state, nstreams, capacity, events, events_stride, streams, spec, items_stride):
    """ffgpu_outline_scene_dev: (ntargets, items_stride) items.  scenes: SCENE_DTYPE per stream; state: the zones state's bytes (uint8); events: the event
    rows as uint32, events_stride words apart"""
    raw = np.asarray(state, np.uint8).reshape(nstreams, STATE_HEADER + 64 * capacity)
    hdr = raw[:, :STATE_HEADER].copy().view("<u4")
    slots = np.ascontiguousarray(raw[:, STATE_HEADER:]).view(SLOT_DTYPE).reshape(nstreams, capacity)
    ev = np.asarray(events).view("<u4").reshape(-1, events_stride)
    out = np.zeros((len(streams), items_stride), ITEM_DTYPE)
    for t, s in enumerate(streams):
        if s < 0:
            continue
        sc = scenes[s]
        if spec.flags & ZONES:
            for z in range(max(0, min(int(sc["nzones"]), 8))):
                zn = sc["zone"][z]
                if not zone_draws(zn):
                    continue
                nv = int(zn["nverts"])
                col = spec.alarm if spec.flags & ALARM and int(ev[t, 16 + 4 * z + 3]) != 0 else spec.paint(z)
                for i in range(nv):
                    j = (i + 1) % nv
                    out[t, 8 * z + i] = make_item(f2i(zn["x"][i]), f2i(zn["y"][i]), f2i(zn["x"][j]), f2i(zn["y"][j]), col, spec.thickness)
        for l in range(max(0, min(int(sc["nlines"]), 8))):
            ln = sc["line"][l]
            ax, ay, bx, by = f2i(ln["ax"]), f2i(ln["ay"]), f2i(ln["bx"]), f2i(ln["by"])
            if spec.flags & LINES:
                out[t, 64 + 2 * l] = make_item(ax, ay, bx, by, spec.paint(8 + l), spec.thickness, spec.line_dash)
            if spec.flags & TICKS:
                out[t, 64 + 2 * l + 1] = make_item(*tick_ends(ax, ay, bx, by), spec.paint(8 + l), 1)
        if spec.flags & MARKERS:
            for k, q in enumerate(seen_slots(hdr[s, 0], slots[s])):
                if FIXED + 2 * k + 1 >= items_stride:
                    break
                sl = slots[s, q]
                cx, cy, r, col = f2i(sl["px"]), f2i(sl["py"]), spec.marker, spec.paint(int(sl["id"]))
                out[t, FIXED + 2 * k] = make_item(cx - r, cy, cx + r, cy, col, 1)
                out[t, FIXED + 2 * k + 1] = make_item(cx, cy - r, cx, cy + r, col, 1)
    return out
