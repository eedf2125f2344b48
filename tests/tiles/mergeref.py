"""Tiled detection: a float32 numpy restatement of the merge contract of include/ffcnn_hip.h (ffgpu_merge_tiles_dev).

    1. translate every survivor of every tile by the tile's origin: one fp32 addition per coordinate;
    2. order the union by score descending, then position of the tile in the caller's table ascending, then index in the tile's list ascending;
    3. greedy class-aware suppression (ffcnn.c:298-322): area = (x2 - x1) * (y2 - y1) in fp32, a later box of the same class goes when
       metric > thresh, metric = inter / min(area) or inter / union, a suppressed box never suppresses another;
    4. the survivors in that order, not rescaled.

GPU results are compared with THIS, byte for byte, not with oracle.orc.nms directly: the reference orders equal scores by qsort, which is
unspecified, and a tiled picture produces exact ties from identical pixels.  tests/test_tiles_abi.py pins this file to orc.nms on tie-free lists."""
import numpy as np

BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])


def merge(lists, origins, thresh=0.5, use_min=1, stats=None):
    """lists: one BOX_DTYPE array per tile, in the caller's table order; origins: one (x0, y0) per tile.  Returns the merged survivors.
    stats (a dict, optional) counts the same-class pairs the loop examined: stats["suppressed"], stats["kept"]."""
    parts, pos, idx = [], [], []
    for k, (b, (x0, y0)) in enumerate(zip(lists, origins)):
        b = np.array(b, BOX_DTYPE)
        fx, fy = np.float32(x0), np.float32(y0)
        for c, f in (("x1", fx), ("x2", fx), ("y1", fy), ("y2", fy)):
            b[c] = (b[c] + f).astype(np.float32)
        parts.append(b)
        pos.append(np.full(len(b), k))
        idx.append(np.arange(len(b)))
    if not parts or sum(len(p) for p in parts) == 0:
        return np.zeros(0, BOX_DTYPE)
    u, pos, idx = np.concatenate(parts), np.concatenate(pos), np.concatenate(idx)
    u = u[np.lexsort((idx, pos, -u["score"].astype(np.float64)))]
    x1, y1, x2, y2, ty = u["x1"], u["y1"], u["x2"], u["y2"], u["type"]
    area = ((x2 - x1) * (y2 - y1)).astype(np.float32)
    alive = np.ones(len(u), bool)
    thresh = np.float32(thresh)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(len(u)):
            if not alive[a]:
                continue
            j = np.nonzero(alive[a + 1:] & (ty[a + 1:] == ty[a]))[0] + a + 1
            if not len(j):
                continue
            xa, ya = np.maximum(x1[a], x1[j]), np.maximum(y1[a], y1[j])
            xb, yb = np.minimum(x2[a], x2[j]), np.minimum(y2[a], y2[j])
            inter = np.where((xa < xb) & (ya < yb), ((xb - xa).astype(np.float32) * (yb - ya).astype(np.float32)).astype(np.float32), np.float32(0))
            if use_min:
                metric = (inter / np.minimum(area[a], area[j])).astype(np.float32)
            else:
                metric = (inter / ((area[a] + area[j]).astype(np.float32) - inter).astype(np.float32)).astype(np.float32)
            gone = metric > thresh
            alive[j[gone]] = False
            if stats is not None:
                stats["suppressed"] = stats.get("suppressed", 0) + int(gone.sum())
                stats["kept"] = stats.get("kept", 0) + int((~gone).sum())
    return u[alive].copy()


def record(merged, tile_records):
    """the merged ffgpu_frame_dets of one picture from its merged survivors and its tiles' records"""
    r = np.zeros((), DETS_DTYPE)
    n = len(merged)
    r["count"], r["nfull"] = min(n, MAX_DET), n
    r["ncand"] = int(sum(int(t["ncand"]) for t in tile_records))
    r["overflow"] = (1 if any(int(t["overflow"]) & 1 for t in tile_records) else 0) | (4 if n > MAX_DET else 0)
    r["box"][:min(n, MAX_DET)] = merged[:MAX_DET]
    return r


def merge_table(records, lists, tiles, nimages, thresh=0.5, use_min=1):
    """the whole operator: records (DETS_DTYPE array, one per table entry), lists (one BOX_DTYPE array per entry, or None: the records' own
    box[0 .. count)), tiles (one (image, x0, y0) per entry).  Returns ([merged record per picture], [merged full list per picture])."""
    recs, fulls = [], []
    for g in range(nimages):
        sel = [t for t, e in enumerate(tiles) if e[0] == g]
        src = [lists[t] if lists is not None else records[t]["box"][:records[t]["count"]] for t in sel]
        m = merge(src, [(tiles[t][1], tiles[t][2]) for t in sel], thresh, use_min)
        recs.append(record(m, [records[t] for t in sel]))
        fulls.append(m)
    return recs, fulls
