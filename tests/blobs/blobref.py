"""Motion blobs: a numpy restatement of the contract of include/ffcnn_hip.h (ffgpu_blobs_dev), in the contract's own words, with a plain flood
fill.  GPU results are compared with THIS, byte for byte (tests/blobs/test_gpu_fuzz_input.py).  The state is the motion maps' (motionref.State)."""
import numpy as np

from motion.motionref import BOX_DTYPE, DETS_DTYPE, MAX_DET, State  # noqa: F401  (the record layout and the state)

WORDS, MAX_CELLS, COMPONENTS = 8, 32768, 2048


class Spec:
    def __init__(self, w, h, cell_log2, min_pixels=1, warmup=0, connect=8, min_cells=1, max_cells=0, max_boxes=MAX_DET, pad=0, type_=0):
        self.w, self.h, self.cell_log2, self.min_pixels, self.warmup, self.connect = w, h, cell_log2, min_pixels, warmup, connect
        self.min_cells, self.max_cells, self.max_boxes, self.pad, self.type = min_cells, max_cells, max_boxes, pad, type_
        self.c = 1 << cell_log2
        self.gw, self.gh = (w + self.c - 1) >> cell_log2, (h + self.c - 1) >> cell_log2


def components(active, connect):
    """the components of a boolean grid as lists of (y, x), in the order of their roots (the raster scan meets a component at its root)"""
    gh, gw = active.shape
    near = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connect == 8 else [])
    seen, out = np.zeros_like(active), []
    for y, x in zip(*np.nonzero(active)):
        if seen[y, x]:
            continue
        comp, todo, seen[y, x] = [], [(int(y), int(x))], True
        while todo:
            j, i = todo.pop()
            comp.append((j, i))
            for dj, di in near:
                q = (j + dj, i + di)
                if 0 <= q[0] < gh and 0 <= q[1] < gw and active[q] and not seen[q]:
                    seen[q] = True
                    todo.append(q)
        out.append(comp)
    return out


def target(sp, frames, cells):
    """(words, record, labels) of one stream: frames as an int, cells the gh x gw uint32 counts"""
    words, rec, labels = np.zeros(WORDS, "<i4"), np.zeros((), DETS_DTYPE), np.zeros((sp.gh, sp.gw), "<u2")
    words[6] = np.uint32(frames).astype("<i4")
    if int(frames) % 2 ** 32 <= sp.warmup:
        return words, rec, labels
    c, w, h = sp.c, sp.w, sp.h
    active = cells >= sp.min_pixels
    comps = components(active, sp.connect)
    table = []
    for comp in comps[:COMPONENTS]:
        area = [(min(c * (x + 1), w) - c * x) * (min(c * (y + 1), h) - c * y) for y, x in comp]
        ys, xs = [y for y, _ in comp], [x for _, x in comp]
        table.append(dict(root=min(y * sp.gw + x for y, x in comp), cells=len(comp), area=sum(area), pixels=sum(min(int(cells[q]), a) for q, a in zip(comp, area)),
                          i0=min(xs), i1=max(xs), j0=min(ys), j1=max(ys), comp=comp))
    kept = sorted((e for e in table if sp.min_cells <= e["cells"] and (sp.max_cells == 0 or e["cells"] <= sp.max_cells)),
                  key=lambda e: (-e["pixels"], -e["cells"], e["root"]))
    written, untabled = kept[:sp.max_boxes], len(comps) - len(table)
    labels[active] = 0xFFFF
    for r, e in enumerate(written):
        q = min(256, e["pixels"] * 256 // e["area"])
        rec["box"][r] = (sp.type, np.float32(q) / np.float32(256), max(c * e["i0"] - sp.pad, 0), max(c * e["j0"] - sp.pad, 0),
                         min(min(c * (e["i1"] + 1), w) - 1 + sp.pad, w - 1), min(min(c * (e["j1"] + 1), h) - 1 + sp.pad, h - 1))
        for p in e["comp"]:
            labels[p] = r + 1
    rec["count"] = rec["nfull"] = len(written)
    rec["ncand"], rec["overflow"] = len(kept), int(len(kept) > len(written) or untabled > 0)
    words[:6] = (int(active.sum()), len(comps), len(kept), len(written), untabled, 1)
    return words, rec, labels


def blobs(streams, sp, state):
    """(words n x 8, records, labels n x ALIGN(gw gh, 8) with the padding zero) of a call"""
    n, pitch = len(streams), (sp.gw * sp.gh + 7) & ~7
    words, recs, labels = np.zeros((n, WORDS), "<i4"), np.zeros(n, DETS_DTYPE), np.zeros((n, pitch), "<u2")
    for t, s in ((t, s) for t, s in enumerate(streams) if s >= 0):
        words[t], recs[t], lab = target(sp, state.hdr[s, 0], state.cells[s])
        labels[t, :sp.gw * sp.gh] = lab.reshape(-1)
    return words, recs, labels
