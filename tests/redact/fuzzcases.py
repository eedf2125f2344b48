"""The seeded cases of the redaction fuzz (tests/redact/test_gpu_fuzz_input.py) and the conditions that keep it from passing vacuously.  The cases are
made here, from their own generator and before any device call, so tests/test_redact_abi.py can hold the conditions against redactref alone."""
import numpy as np

from overlay.test_gpu_fuzz_input import fixed_boxes
from redact import redactref

BOX = redactref.BOX_DTYPE
Spec, FILL, MOSAIC = redactref.Spec, redactref.FILL, redactref.MOSAIC
# 150 x 140: a block boundary inside the frame with cell 6 (blocks of 60) and with cell 64 (partial cells at both edges); 65 x 33, 70 x 45: one past a
# block of 64; the rest: smaller than a block, odd, down to one pixel
SIZES = ((1, 1), (2, 3), (7, 5), (13, 9), (33, 17), (64, 48), (65, 33), (70, 45), (150, 140))
CELLS = {False: (2, 3, 5, 8, 64), True: (2, 4, 6, 64)}


def rand_boxes(rng, n, w, h):
    """n boxes around a w x h target: about half inside, a third across an edge, the rest wholly outside or inverted; classes -1 .. 4, scores 0 .. 1"""
    b = np.zeros(n, BOX)
    b["type"] = rng.integers(-1, 5, n)
    b["score"] = rng.uniform(0, 1, n)
    for k in range(n):
        a, c = sorted(float(v) for v in rng.uniform(0, w, 2))
        t, d = sorted(float(v) for v in rng.uniform(0, h, 2))
        kind = rng.random()
        if kind < 0.33:
            side = int(rng.integers(0, 4))
            a, t = (a - rng.uniform(1, w + 2) if side == 0 else a), (t - rng.uniform(1, h + 2) if side == 1 else t)
            c, d = (c + rng.uniform(1, w + 2) if side == 2 else c), (d + rng.uniform(1, h + 2) if side == 3 else d)
        elif kind < 0.43:
            a, c = a + w + 3, c + w + 3
        elif kind < 0.5:
            a, c = c + 1, a
        b[k]["x1"], b[k]["y1"], b[k]["x2"], b[k]["y2"] = a, t, c, d
    return b


def rand_spec(rng, mode, cell, outside):
    classes = None if rng.random() < 0.3 else [1, 1, 0, 1, 1][:int(rng.integers(3, 6))]
    margin = ((0, 1), (1, 8), (1, 4), (1, 2))[int(rng.integers(0, 4))]
    return Spec(mode, cell, outside, float(rng.uniform(0.05, 0.3)), classes, margin, tuple(int(v) for v in rng.integers(0, 256, 3)))


def targets_of(rng, nv12, sizes=SIZES):
    out = []
    for k, (w, h) in enumerate(sizes):
        if nv12:
            mu = 2 * ((w + 1) // 2)
            out.append(((w, h, w, mu, False), (w, h, w, mu, True), (w, h, w + 5, mu + 6, False), (w, h, w + 6, mu + 10, True))[k % 4])
        else:
            out.append((w, h, (3 * w, (3 * w + 3) & ~3, 3 * w + 13)[k % 3]))
    return out


# one generator seed per parametrisation (nv12, mode, outside): the first from 5220, 5230, .. on whose cases meet check_stats on redactref alone
SEEDS = {(False, 0, False): 5220, (False, 0, True): 5230, (False, 1, False): 5240, (False, 1, True): 5250, (True, 0, False): 5260, (True, 0, True): 5270, (True, 1, False): 5281, (True, 1, True): 5290}


def fuzz_cases(nv12, mode, outside, seed=None):
    """one parametrisation's calls: (cell, specs, lists, spec) per call"""
    rng = np.random.default_rng(SEEDS[(bool(nv12), mode, bool(outside))] if seed is None else seed)
    out = []
    for call, cell in enumerate(CELLS[nv12]):
        specs = targets_of(rng, nv12)
        lists = []
        for k, s in enumerate(specs):
            b = rand_boxes(rng, (k + call + 3) % 8, s[0], s[1])     # (the largest target, k = 8: 3 to 7 boxes)
            if (k + call) % 5 == 1:
                fb = fixed_boxes(s[0], s[1])
                fb["type"] = np.arange(len(fb)) % 4
                b = np.concatenate([b, fb[rng.permutation(len(fb))[:3]]])[:7]
            lists.append(b)
        out.append((cell, specs, lists, rand_spec(rng, mode, cell if mode == MOSAIC else 0, outside)))
    return out


def check_stats(total, nv12, mode):
    """redactref's statistics summed over one parametrisation's cases: an empty qualifying box, a box rejected by score and one by class, more than a
    quarter of the pixels covered and more than a quarter left alone; MOSAIC: a partly covered cell, a cell cut by the right and one by the bottom
    edge (FILL has no cells); NV12: a chroma sample with mixed coverage"""
    n = lambda key: total.get(key, 0)                                               # noqa: E731
    assert n("empty") > 0 and n("rejected_score") > 0 and n("rejected_class") > 0 and n("qualifying") > n("empty"), total
    assert 4 * n("covered") > n("pixels") and 4 * (n("pixels") - n("covered")) > n("pixels"), total
    if mode == MOSAIC:
        assert min(n("cells_partial"), n("cells_full"), n("cells_cut_right"), n("cells_cut_bottom")) > 0, total
    if nv12:
        assert n("chroma_mixed") > 0, total
