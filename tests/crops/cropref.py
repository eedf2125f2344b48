"""numpy restatement of the crop contract of include/ffcnn_hip.h (ffgpu_crop_boxes_*_dev, ffgpu_exec_crop_*, ffgpu_crops_to_source_dev): which
boxes of which sources become crops and in what order (select), the table's bytes, the pixels of a slot in both forms for BGR and NV12 sources
(slot_pixels is the sliced form, slot_pixels_literal the per-pixel loop; tests/test_crops_abi.py holds the two against each other and the F32
slot against the reference's own net_input through the oracle), and the way back into source coordinates (map_back).  Python integers stand for
the contract's 64-bit integers, numpy float32 scalars for its fp32 arithmetic.  Nothing here knows how the device parallelises."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
CROP_DTYPE = np.dtype([("target", "<i4"), ("box", "<i4"), ("type", "<i4"), ("score", "<f4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"),
                       ("sw", "<i4"), ("sh", "<i4"), ("s1", "<i4"), ("s2", "<i4")])
MAX_DET = 128
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
F32, U8 = 0, 1
MATS = {0: (16, 298, 409, 100, 208, 516), 1: (0, 256, 359, 88, 183, 454), 2: (16, 298, 459, 55, 136, 541), 3: (0, 256, 403, 48, 120, 475)}


class Spec:
    """ffgpu_crop_spec: classes is None or a sequence of flags; margin = (num, den)"""

    def __init__(self, out_w, out_h, form=F32, per_target=1, min_score=0.0, classes=None, margin=(0, 1), mean=(0.0, 0.0, 0.0), norm=(1 / 255.0,) * 3):
        self.out_w, self.out_h, self.form, self.per_target, self.min_score, self.classes = out_w, out_h, form, per_target, min_score, classes
        self.num, self.den = margin
        self.mean, self.norm = tuple(mean), tuple(norm)


def align4(v):
    return (v + 3) & ~3


def f2i(v):
    """(int)v as the draw contract defines it: toward zero, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    if v >= 2.0 ** 31:
        return INT_MAX
    if v <= -2.0 ** 31:
        return INT_MIN
    return int(v)


def corners(box):
    return f2i(box["x1"]), f2i(box["y1"]), f2i(box["x2"]), f2i(box["y2"])


def letterbox(w, h, W, H):
    """net_input's (sw, sh, s1, s2) of a w x h image in a W x H plane (ffcnn.c:267-273)"""
    if w * H > h * W:
        return W, W * h // w, w, W
    return H * w // h, H, h, H


def qualifies(box, spec):
    if not (np.float32(box["score"]) >= np.float32(spec.min_score)):             # (False for a NaN score)
        return False
    if spec.classes is None:
        return True
    t = int(box["type"])
    return 0 <= t < len(spec.classes) and bool(spec.classes[t])


def region(box, w, h, num, den):
    """(X0, Y0, X1, Y1, edges clipped as a set of 'l' 't' 'r' 'b') of a qualifying box in a w x h source, or None: the box is empty"""
    a, b, c, d = corners(box)
    if a > c or b > d:
        return None
    mx, my = (c - a + 1) * num // den, (d - b + 1) * num // den
    X0, X1, Y0, Y1 = max(a - mx, 0), min(c + mx, w - 1), max(b - my, 0), min(d + my, h - 1)
    if X0 > X1 or Y0 > Y1:
        return None
    clipped = {k for k, hit in (("l", a - mx < 0), ("r", c + mx > w - 1), ("t", b - my < 0), ("b", d + my > h - 1)) if hit}
    return X0, Y0, X1, Y1, clipped


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + n


def select(sources, lists, spec, capacity, stats=None):
    """sources[t]: None (skipped) or a dict with w, h and, for the statistics, nv12 (bool), addr (device address of row 0 of the pixels / the Y
    plane) and pitch; lists[t]: the boxes the device reads for target t (the caller applies the clamps of the counts).  Returns (header, entries):
    header = (total, taken, empty, capacity), entries = a CROP_DTYPE array of `capacity`."""
    ent = np.zeros(capacity, CROP_DTYPE)
    ent["target"], ent["s1"], ent["s2"] = -1, 1, 1
    total = empty = 0
    for t, (src, boxes) in enumerate(zip(sources, lists)):
        if src is None:
            continue
        mine = 0
        for k, box in enumerate(boxes):
            if not qualifies(box, spec):
                continue
            r = region(box, src["w"], src["h"], spec.num, spec.den)
            if r is None:
                empty += 1
                _bump(stats, "empty")
                continue
            if mine >= spec.per_target:
                _bump(stats, "cut_per_target")
                continue
            mine += 1
            X0, Y0, X1, Y1, clipped = r
            w, h = X1 - X0 + 1, Y1 - Y0 + 1
            if total < capacity:
                sw, sh, s1, s2 = letterbox(w, h, spec.out_w, spec.out_h)
                ent[total] = (t, k, box["type"], box["score"], X0, Y0, w, h, sw, sh, s1, s2)
                for e in clipped:
                    _bump(stats, "clip_" + e)
                _bump(stats, "down" if s1 > s2 else ("up" if s1 < s2 else "same"))
                if s1 == s2 and sw >= 4 and "addr" in src:
                    first = src["addr"] + X0 if src.get("nv12") else src["addr"] + Y0 * src["pitch"] + 3 * X0
                    _bump(stats, "same_dword" if (first | src["pitch"]) & 3 == 0 else "same_bytes")
                if src.get("nv12"):
                    _bump(stats, "odd_x", X0 & 1)
                    _bump(stats, "odd_y", Y0 & 1)
            else:
                _bump(stats, "cut_capacity")
            total += 1
    return (total, min(total, capacity), empty, capacity), ent


def table_bytes(header, entries):
    return np.concatenate([np.asarray(header, "<i4").view(np.uint8), entries.view(np.uint8).reshape(-1)])


def nv12_picture(Y, UV, w, h, matrix):
    """the BGR picture (h, w, 3) an NV12 source stands for: the header's integer formula, nearest chroma (Y: (h, >= w), UV: ((h + 1) // 2, >= 2 ((w + 1) // 2)))"""
    yoff, cy, crv, cgu, cgv, cbu = MATS[matrix]
    yy, xx = np.mgrid[0:h, 0:w]
    c = Y[yy, xx].astype(np.int32) - yoff
    d = UV[yy >> 1, 2 * (xx >> 1)].astype(np.int32) - 128
    e = UV[yy >> 1, 2 * (xx >> 1) + 1].astype(np.int32) - 128
    r, g, b = (cy * c + crv * e + 128) >> 8, (cy * c - cgu * d - cgv * e + 128) >> 8, (cy * c + cbu * d + 128) >> 8
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def slot_pixels(img, e, out_w, out_h):
    """the B G R bytes (out_h, out_w, 3) of entry e's slot cut out of its source picture img (h, w, 3): pixel (x, y), x < sw, y < sh, is source
    pixel (x0 + x s1 / s2, y0 + y s1 / s2), zero elsewhere -- as index arrays"""
    out = np.zeros((out_h, out_w, 3), np.uint8)
    sw, sh, s1, s2 = int(e["sw"]), int(e["sh"]), int(e["s1"]), int(e["s2"])
    if sw > 0 and sh > 0:
        xs = int(e["x0"]) + np.arange(sw, dtype=np.int64) * s1 // s2
        ys = int(e["y0"]) + np.arange(sh, dtype=np.int64) * s1 // s2
        out[:sh, :sw] = img[ys][:, xs]
    return out


def slot_pixels_literal(img, e, out_w, out_h):
    """the same, pixel by pixel"""
    out = np.zeros((out_h, out_w, 3), np.uint8)
    for y in range(out_h):
        for x in range(out_w):
            if x < int(e["sw"]) and y < int(e["sh"]):
                out[y, x] = img[int(e["y0"]) + y * int(e["s1"]) // int(e["s2"]), int(e["x0"]) + x * int(e["s1"]) // int(e["s2"])]
    return out


def slot_f32(pix, e, mean, norm):
    """FFGPU_CROP_F32: planes R, G, B of ((float)byte - mean) * norm (two fp32 roundings) inside sw x sh, 0.0 elsewhere; (3, out_h, out_w) float32"""
    out = np.zeros((3,) + pix.shape[:2], np.float32)
    sw, sh = int(e["sw"]), int(e["sh"])
    for p in range(3):
        v = pix[:sh, :sw, 2 - p].astype(np.float32)
        out[p, :sh, :sw] = (v - np.float32(mean[p])) * np.float32(norm[p])
    return out


def slot_u8(pix):
    """FFGPU_CROP_U8: out_h rows of ALIGN(3 out_w, 4) bytes, padding zero"""
    h, w = pix.shape[:2]
    out = np.zeros((h, align4(3 * w)), np.uint8)
    out[:, :3 * w] = pix.reshape(h, 3 * w)
    return out


def slot_nbytes(spec):
    return 12 * spec.out_w * spec.out_h if spec.form == F32 else spec.out_h * align4(3 * spec.out_w)


def slots(pictures, header, entries, spec):
    """the bytes of all `capacity` slots; pictures[t]: the BGR picture (h, w, 3) of source t (None where it is skipped)"""
    n = slot_nbytes(spec)
    out = np.zeros((header[3], n), np.uint8)
    for k in range(header[1]):
        e = entries[k]
        pix = slot_pixels(pictures[int(e["target"])], e, spec.out_w, spec.out_h)
        out[k] = (slot_f32(pix, e, spec.mean, spec.norm) if spec.form == F32 else slot_u8(pix)).view(np.uint8).reshape(-1)
    return out.reshape(-1)


def _move(boxes, e):
    """x * (float)s1 / (float)s2 + (float)x0 in fp32: multiply, divide, add"""
    out = boxes.copy()
    s1, s2 = np.float32(int(e["s1"])), np.float32(int(e["s2"]))
    with np.errstate(all="ignore"):
        for c, o in (("x1", "x0"), ("y1", "y0"), ("x2", "x0"), ("y2", "y0")):
            out[c] = (boxes[c].astype(np.float32) * s1 / s2 + np.float32(int(e[o]))).astype(np.float32)
    return out


def map_back(header, entries, records, lists=None, stride=0, out_lists=None):
    """records: `capacity` ffgpu_frame_dets (a structured array with count, ncand, overflow, nfull, box); lists: (capacity, stride) boxes or
    None; out_lists: what the output lists hold before the call.  Returns (records, lists) after it."""
    out = np.zeros_like(records)
    outl = None if lists is None or out_lists is None else out_lists.copy().reshape(header[3], stride)
    for n in range(header[1]):
        e, r = entries[n], records[n]
        nb = max(0, min(int(r["count"]), MAX_DET))
        for f in ("count", "ncand", "overflow", "nfull"):
            out[n][f] = r[f]
        out[n]["box"][:nb] = _move(r["box"][:nb], e)
        if outl is not None:
            nl = max(0, min(int(r["nfull"]), stride))
            outl[n, :nl] = _move(lists.reshape(header[3], stride)[n, :nl], e)
    return out, outl
