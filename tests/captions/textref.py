"""The captions contract of include/ffcnn_hip.h restated in numpy: the rasteriser (text items drawn serially in slot order into u8 BGR and NV12
surfaces, the NV12 chroma rule), the box composer (which boxes are captioned, where the tag sits, the three text parts) and the scene composer (the
zones' occupancies and the lines' totals as items).  The font is an argument: a (256, 8) or flat 2 048-byte uint8 array.  The GPU tests compare the
device's bytes with this; tests/test_captions_abi.py pins this to a literal per-pixel scalar loop and to the formatting cases."""
import numpy as np

from zones.zoneref import BOX_DTYPE, DETS_DTYPE, SCENE_DTYPE, STATE_HEADER  # noqa: F401  (the records' and the scenes' layouts)

TEXT_MAX, TEXT_ITEMS, OPAQUE = 44, 256, 1
DETS = 128
NAME, SCORE, ID, CAPTION_OPAQUE = 1, 2, 4, 8
NONE, TYPE, IDS = 0, 1, 2
ZONES_ROW = 64
MAX_DET = DETS_DTYPE["box"].shape[0]
ITEM_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("fg", "u1", (4,)), ("bg", "u1", (4,)), ("scale", "u1"), ("flags", "u1"), ("len", "u1"), ("reserved", "u1"),
                       ("text", "u1", (TEXT_MAX,))])
assert ITEM_DTYPE.itemsize == 64
F32 = np.float32


class Spec:
    """ffgpu_caption_spec: names is None or an (n, 16) uint8 array (the rows d_names points to), palette None or a sequence of colours"""

    def __init__(self, flags=NAME | SCORE, min_score=0.0, identity=NONE, scale=1, fg=(255, 255, 255), color=(0, 0, 0), palette=None, names=None):
        self.flags, self.min_score, self.identity, self.scale = flags, F32(min_score), identity, scale
        self.fg, self.color, self.palette = tuple(fg[:3]), tuple(color[:3]), None if palette is None else [tuple(c[:3]) for c in palette]
        self.names = None if names is None else np.asarray(names, np.uint8).reshape(-1, 16)

    def paper(self, index):
        return self.color if self.palette is None else self.palette[index % len(self.palette)]


# ---------------------------------------------------------------------------------------------------------------- the rasteriser
def clamped(item):
    """(s, n): the scale and the length an item draws with"""
    return min(max(int(item["scale"]), 1), 4), min(int(item["len"]), TEXT_MAX)


def masks(item, font, w, h):
    """(x0, y0, written, ink): the item's rectangle clipped to the target as the slice [y0:y0 + rows, x0:x0 + cols], and, over it, the pixels the item
    writes and those of them that are ink; None when nothing of the rectangle lies inside"""
    font = np.asarray(font, np.uint8).reshape(256, 8)
    s, n = clamped(item)
    x, y = int(item["x"]), int(item["y"])
    x0, x1, y0, y1 = max(x, 0), min(x + 8 * s * n, w), max(y, 0), min(y + 8 * s, h)
    if x1 <= x0 or y1 <= y0:
        return None
    dx, dy = np.arange(x0, x1, dtype=np.int64) - x, np.arange(y0, y1, dtype=np.int64) - y
    glyph = item["text"][dx // (8 * s)].astype(np.int64)
    col, row = (dx // s) % 8, dy // s
    ink = ((font[glyph[None, :], row[:, None]] >> (7 - col[None, :])) & 1).astype(bool)
    written = ink | bool(int(item["flags"]) & OPAQUE)
    return x0, y0, written, ink


def draw_bgr(buf, off, w, h, pitch, items, font):
    """the items drawn serially in slot order into the BGR surface at byte `off` of the flat uint8 array `buf`, rows `pitch` bytes apart"""
    for it in items:
        m = masks(it, font, w, h)
        if m is None:
            continue
        x0, y0, written, ink = m
        ys, xs = np.nonzero(written)
        val = np.where(ink[ys, xs][:, None], it["fg"][None, :3], it["bg"][None, :3])
        at = off + (y0 + ys) * pitch + 3 * (x0 + xs)
        for c in range(3):
            buf[at + c] = val[:, c]


def draw_nv12(buf, y_off, uv_off, w, h, pitch_y, pitch_uv, items, font):
    """the same into an NV12 surface: a written pixel sets its Y byte; a chroma pair any of whose luma pixels the item writes takes the item's fg (U, V)
    if one of those written pixels is ink, else its bg (U, V).  Serially in slot order: the last such item decides."""
    for it in items:
        m = masks(it, font, w, h)
        if m is None:
            continue
        x0, y0, written, ink = m
        ys, xs = np.nonzero(written)
        buf[y_off + (y0 + ys) * pitch_y + x0 + xs] = np.where(ink[ys, xs], it["fg"][0], it["bg"][0])
        sy, sx = (y0 + ys) >> 1, (x0 + xs) >> 1
        key = sy.astype(np.int64) * ((w + 1) // 2) + sx
        samples, inv = np.unique(key, return_inverse=True)
        any_ink = np.zeros(len(samples), bool)
        np.logical_or.at(any_ink, inv, ink[ys, xs])
        at = uv_off + (samples // ((w + 1) // 2)) * pitch_uv + 2 * (samples % ((w + 1) // 2))
        buf[at] = np.where(any_ink, it["fg"][1], it["bg"][1])
        buf[at + 1] = np.where(any_ink, it["fg"][2], it["bg"][2])


# ---------------------------------------------------------------------------------------------------------------- the composers
def f2i(v):
    """(int)v of the draw contract: toward zero, saturating, NaN -> 0"""
    v = F32(v)
    if v != v:
        return 0
    if v >= F32(2147483648.0):
        return 2 ** 31 - 1
    if v <= F32(-2147483648.0):
        return -2 ** 31
    return int(v)


def score_percent(score):
    with np.errstate(all="ignore"):
        return min(max(f2i(F32(F32(score) * F32(100.0)) + F32(0.5)), 0), 999)


def caption_text(type_, score, v, spec):
    """the caption's bytes, cut to TEXT_MAX: the parts present, joined by one space.  v: the id (0: absent)"""
    parts = []
    if spec.flags & NAME and spec.identity != TYPE:
        if spec.names is not None and 0 <= type_ < len(spec.names):
            row = bytes(spec.names[type_])
            parts.append(row.split(b"\0")[0])
        else:
            parts.append(b"%d" % type_)
    if spec.flags & SCORE:
        parts.append(b"%d%%" % score_percent(score))
    if spec.flags & ID and v != 0:
        parts.append(b"#%d" % v if v > 0 else b"#%d?" % -v)
    return b" ".join(p for p in parts if p)[:TEXT_MAX]


def make_item(x, y, text, fg, bg, scale, opaque):
    it = np.zeros((), ITEM_DTYPE)
    it["x"], it["y"], it["scale"], it["flags"], it["len"] = x, y, scale, OPAQUE if opaque else 0, len(text)
    it["fg"][:3], it["bg"][:3] = fg, bg
    it["text"][:len(text)] = np.frombuffer(text, np.uint8)
    return it


def box_item(b, v, spec):
    a, top = f2i(b["x1"]), f2i(b["y1"])
    s8 = 8 * spec.scale
    return make_item(a, top - s8 if top >= s8 else top, caption_text(int(b["type"]), b["score"], v, spec), spec.fg, spec.paper(int(b["type"])), spec.scale,
                     bool(spec.flags & CAPTION_OPAQUE))


def caption_boxes(recs, flat, stride, first, spec, ids, items_stride):
    """ffgpu_caption_boxes_dev: (ntargets, items_stride) items.  flat None: the records' own boxes; first: the lists' starts (None: t * stride); ids: rows
    of 8 + S ints (S = stride, or MAX_DET without lists), read with identity IDS"""
    n = len(recs)
    out = np.zeros((n, items_stride), ITEM_DTYPE)
    S = stride if flat is not None else MAX_DET
    for t in range(n):
        if flat is None:
            boxes = recs[t]["box"][:max(0, min(int(recs[t]["count"]), MAX_DET))]
        else:
            lo = t * stride if first is None else int(first[t])
            boxes = flat[lo:lo + max(0, min(int(recs[t]["nfull"]), stride))]
        k = 0
        with np.errstate(invalid="ignore"):
            ok = boxes["score"] >= spec.min_score
        for j in np.nonzero(ok)[0]:
            if k >= min(DETS, items_stride):
                break
            b = boxes[j]
            v = 0 if spec.identity == NONE else int(b["type"]) if spec.identity == TYPE else int(np.asarray(ids).reshape(n, 8 + S)[t, 8 + j])
            out[t, k] = box_item(b, v, spec)
            k += 1
    return out


def caption_scene(scenes, state, nstreams, capacity, events, events_stride, streams, spec, items_stride):
    """ffgpu_caption_scene_dev: (ntargets, items_stride) items.  scenes: SCENE_DTYPE per stream; state: the zones state's bytes (uint8); events: the event
    rows as uint32, events_stride words apart"""
    hdr = np.asarray(state, np.uint8).reshape(nstreams, STATE_HEADER + 64 * capacity)[:, :STATE_HEADER].copy().view("<u4")
    ev = np.asarray(events).view("<u4").reshape(-1, events_stride)
    out = np.zeros((len(streams), items_stride), ITEM_DTYPE)
    opaque = bool(spec.flags & CAPTION_OPAQUE)
    for t, s in enumerate(streams):
        if s < 0:
            continue
        sc = scenes[s]
        for z in range(max(0, min(int(sc["nzones"]), 8))):
            zn = sc["zone"][z]
            if 3 <= int(zn["nverts"]) <= 8:
                out[t, z] = make_item(f2i(zn["x"][0]), f2i(zn["y"][0]), b"Z%d %d" % (z, int(ev[t, 16 + 4 * z])), spec.fg, spec.paper(z), spec.scale, opaque)
        for l in range(max(0, min(int(sc["nlines"]), 8))):
            ln = sc["line"][l]
            out[t, 8 + l] = make_item(f2i(ln["ax"]), f2i(ln["ay"]), b"L%d %d/%d" % (l, int(hdr[s, 20 + l]), int(hdr[s, 28 + l])), spec.fg, spec.paper(8 + l),
                                      spec.scale, opaque)
    return out
