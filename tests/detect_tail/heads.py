"""Tiny darknet cfgs and crafted head tensors for the detection-tail tests (k_yolo, k_nms), and what the oracle expects of them.

The vehicle: channels = 3 * (5 + classes), layer 0 a [dropout], layer 1 an [upsample] stride=1 (held to bit equality by tests/layer_ops; it stages the
frame-major input to CNHW), then the [yolo] -- so the FRAMES are the head tensor.  Expected candidates are orc.yolo on the executor's own copy of each
head's input, concatenated in cfg order; expected boxes are orc.nms of the first bbox_max of them when their scores are pairwise distinct, and
nms_ordered (below: the same greedy loop behind a total order, pinned to orc.nms by tests/test_detect_tail_ref.py) when they are not.  No comparison
made with these has a tolerance.  Shared by tests/detect_tail/test_gpu_kernels.py and tests/test_detect_tail_ref.py; nothing here needs a GPU."""
import numpy as np

f32 = np.float32
BOX_DTYPE = np.dtype([("type", "<i4"), ("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4")])
MAX_DET = 128
DETS_DTYPE = np.dtype([("count", "<i4"), ("ncand", "<i4"), ("overflow", "<i4"), ("nfull", "<i4"), ("box", BOX_DTYPE, (MAX_DET,))])
NMS_LDS_CAP = 8192                                   # FFGPU_NMS_LDS_CAP: more candidate slots per frame than this and k_nms works in global scratch
ANCHORS = ((4, 6), (8, 12), (16, 14))


class Head:
    def __init__(self, layer, src, w, h, classes, thresh, anchors=ANCHORS, scale="1"):
        self.layer, self.src, self.w, self.h, self.classes = layer, src, w, h, classes      # src: the layer whose output the head reads
        self.thresh_text, self.scale_text, self.anchors = thresh, scale, tuple(tuple(a) for a in anchors)
        self.thresh, self.scale = f32(float(thresh)), f32(float(scale))                     # (float)atof(text), as both parsers do

    @property
    def slots(self):
        return 3 * self.w * self.h

    def text(self):
        return "[yolo]\nmask=0,1,2\nanchors=%s\nclasses=%d\nignore_thresh=%s\nscale_x_y=%s\n" % (
            ", ".join("%d,%d" % a for a in self.anchors), self.classes, self.thresh_text, self.scale_text)


class Case:
    """one cfg: `text` are the sections behind [net] / [dropout] / [upsample] stride=1 (layers 2 ..), heads in cfg order"""

    def __init__(self, name, netw, neth, classes, batch, heads, between=()):
        self.name, self.netw, self.neth, self.classes, self.batch, self.heads = name, netw, neth, classes, batch, heads
        self.c = 3 * (5 + classes)
        self.between = between
        self.slots = sum(h.slots for h in heads)

    def cfg_text(self):
        body = ["[net]\nwidth=%d\nheight=%d\nchannels=%d\n" % (self.netw, self.neth, self.c), "[dropout]\nprobability=.5\n", "[upsample]\nstride=1\n"]
        at = {h.layer: h for h in self.heads}
        extra = dict(self.between)
        n = 2
        while n in at or n in extra:
            body.append(at[n].text() if n in at else extra[n])
            n += 1
        self.nlayers = n
        return "\n".join(body)

    @property
    def shape(self):
        return (self.batch, self.c, self.neth, self.netw)


def single(name, w, h, classes, batch, thresh, **kw):
    """the head straight on the (staged) frames: net and head have one size"""
    return Case(name, w, h, classes, batch, [Head(2, 1, w, h, classes, thresh, **kw)])


def pooled():
    """a 7 x 5 head on a 56 x 40 net (an 8 x 8 average pool in front), scale_x_y 1.05, anchors of its own"""
    return Case("pooled_7x5", 56, 40, 3, 2, [Head(3, 2, 7, 5, 3, ".5", anchors=((5, 9), (13, 7), (31, 23)), scale="1.05")],
                between=((2, "[avgpool]\nsize=8\nstride=8\n"),))


def two_heads():
    """14 x 10 head, a [route] right behind it back to the head's own input (what the planner's side lane looks for), a 2 x 2 average pool and a
    7 x 5 head with other anchors, threshold and scale: two decode launches count into one ncand, the second head's keys start at 3 * 140"""
    return Case("two_heads", 14, 10, 2, 3,
                [Head(2, 1, 14, 10, 2, ".4", anchors=((2, 3), (5, 4), (7, 9)), scale="1.05"), Head(5, 4, 7, 5, 2, ".3", anchors=((3, 8), (9, 5), (12, 12)), scale="1.1")],
                between=((3, "[route]\nlayers=-2\n"), (4, "[avgpool]\nsize=2\nstride=2\n")))


# ---------------------------------------------------------------------------------------------------------------------------- the oracle's side
def nms_ordered(cand, thresh=0.5, use_min=1, s1=1, s2=1):
    """ffcnn.c:298-335 behind a TOTAL order: score descending, then position in `cand` (the emission order) ascending -- qsort leaves the order of
    equal scores unspecified.  Score 0 is the reference's `dead`: such a box never suppresses and is not kept.  Every operation is the C
    expression in float32, `a > b ? a : b` included (np.maximum would propagate a NaN the C code does not)."""
    u = np.array(cand, BOX_DTYPE)
    u = u[u["score"] != 0]
    u = u[np.argsort(-u["score"].astype(np.float64), kind="stable")]
    x1, y1, x2, y2, ty = u["x1"], u["y1"], u["x2"], u["y2"], u["type"]
    alive = np.ones(len(u), bool)
    thresh = f32(thresh)
    with np.errstate(all="ignore"):
        area = (x2 - x1) * (y2 - y1)
        for a in range(len(u)):
            if not alive[a]:
                continue
            j = np.nonzero(alive[a + 1:] & (ty[a + 1:] == ty[a]))[0] + a + 1
            if not len(j):
                continue
            xa, ya = np.where(x1[a] > x1[j], x1[a], x1[j]), np.where(y1[a] > y1[j], y1[a], y1[j])
            xb, yb = np.where(x2[a] < x2[j], x2[a], x2[j]), np.where(y2[a] < y2[j], y2[a], y2[j])
            inter = np.where((xa < xb) & (ya < yb), (xb - xa) * (yb - ya), f32(0))
            metric = inter / np.where(area[a] < area[j], area[a], area[j]) if use_min else inter / (area[a] + area[j] - inter)
            alive[j[metric > thresh]] = False
        k = u[alive].copy()
        for c in ("x1", "y1", "x2", "y2"):
            k[c] = k[c] * f32(s1) / f32(s2)
    assert k["x1"].dtype == f32 and area.dtype == f32
    return k


def one_nan(boxes):
    """a copy whose NaN coordinates are all the same NaN (their sign and payload are not part of the contract; that they are NaN is)"""
    b = np.array(boxes, BOX_DTYPE)
    for c in ("x1", "y1", "x2", "y2"):
        v = b[c]
        v[np.isnan(v)] = np.nan
        b[c] = v
    assert not np.isnan(b["score"]).any()
    return b


def tie_free(cand):
    return len(np.unique(cand["score"])) == len(cand)


def nms(orc, cand, s1=1, s2=1):
    """(expected boxes, True when they came from plain orc.nms)"""
    if tie_free(cand):
        return orc.nms(cand, 0.5, 1, s1, s2), True
    return nms_ordered(cand, 0.5, 1, s1, s2), False


def record(boxes, ncand, bbox_max):
    """the ffgpu_frame_dets of one frame: ncand counts every decoded candidate (zero scores and those beyond bbox_max included)"""
    r = np.zeros((), DETS_DTYPE)
    n = len(boxes)
    r["count"], r["nfull"], r["ncand"] = min(n, MAX_DET), n, ncand
    r["overflow"] = (1 if ncand > bbox_max else 0) | (4 if n > MAX_DET else 0)
    r["box"][:min(n, MAX_DET)] = boxes[:MAX_DET]
    return r


def decode(orc, case, head, x):
    return orc.yolo(x, head.classes, head.anchors, float(head.thresh), float(head.scale), case.netw, case.neth, cap=max(head.slots, 1))


class Want:
    pass


def expected(orc, case, read, bbox_max, s1=1, s2=1):
    """per frame: .full (every candidate, emission order), .cut (the first bbox_max: what the reference keeps), .boxes, .record, .plain"""
    out = []
    for f in range(case.batch):
        w = Want()
        w.full = np.concatenate([decode(orc, case, h, read(h.src, f)) for h in case.heads])
        w.cut = w.full[:bbox_max]
        w.boxes, w.plain = nms(orc, w.cut, s1, s2)
        w.record = record(w.boxes, len(w.full), bbox_max)
        out.append(w)
    return out


def cell_candidate(orc, case, head, x, k, i, j):
    """the candidates (none or one) of anchor k of cell (i, j) alone: every other objectness is NaN, which no threshold passes"""
    n = 5 + head.classes
    y = np.array(x, f32)
    keep = y[k * n + 4, i, j]
    y[4::n] = np.nan
    y[k * n + 4, i, j] = keep
    return decode(orc, case, head, y)


# ------------------------------------------------------------------------------------------------------------------------ crafted head tensors
def gauss(case, seed, sigma=2.0):
    return np.random.default_rng(seed).normal(0, sigma, case.shape).astype(f32)


def anchor_vec(x, f, k, i, j, classes):
    """the 5 + classes values of one anchor of one cell (a view)"""
    n = 5 + classes
    return x[f, k * n:(k + 1) * n, i, j]


def plant_specs(C):
    """[(name, write(v), claim)] -- v: tx ty tw th objectness class 0 .. C-1 of a cell that otherwise passes (objectness 5, classes below -1).
    claim: ("type", c) | ("absent",) | ("nan0",) | ("neginf",) | ("box", field, value)"""
    def put(pairs):
        def w(v):
            for at, val in pairs:
                v[at] = val
        return w
    S = []
    for c in sorted({0, 1, 62, 63, 64, C - 1}):
        if c < C:
            S.append(("maximum at class %d" % c, put([(5 + c, 30.0)]), ("type", c)))
    ties = [(0, C - 1)] if C >= 2 else []
    if C > 64:
        ties += [(1, 65 if C > 65 else 64), (3, 64)]             # one lane on its first and second trip; two lanes on different trips
    if C > 128:
        ties += [(64, 128)]
    for lo, hi in ties:
        S.append(("tie %d = %d" % (lo, hi), put([(5 + lo, 25.0), (5 + hi, 25.0)]), ("type", lo)))
    if C >= 2:
        a, b = (1 if C > 2 else 0), C - 1
        S.append(("-0 at %d, +0 at %d" % (a, b), put([(5 + a, -0.0), (5 + b, 0.0)]), ("type", a)))
        S.append(("+0 at %d, -0 at %d" % (a, b), put([(5 + a, 0.0), (5 + b, -0.0)]), ("type", a)))
    S.append(("+inf twice", put([(5 + (C - 1) // 2, np.inf), (5 + C - 1, np.inf)]), ("type", (C - 1) // 2)))
    S.append(("all -inf", lambda v: v.__setitem__(slice(5, None), -np.inf), ("neginf",)))
    if C >= 2:
        m = C - 2 if C > 2 else 0
        nans = [(5 + C - 1, np.nan)] + ([(5 + 1, np.nan)] if C > 3 else []) + ([(5 + 64, np.nan)] if C > 66 else [])
        S.append(("NaN above class 0", put(nans + [(5 + m, 30.0)]), ("type", m)))
    S.append(("NaN at class 0", put([(5, np.nan)] + ([(5 + C - 1, 30.0)] if C >= 2 else [])), ("nan0",)))
    S.append(("NaN objectness", put([(4, np.nan)]), ("absent",)))
    for fi, fname in enumerate(("tx", "ty", "tw", "th")):
        for val in (np.nan, np.inf, -np.inf):
            S.append(("%s = %s" % (fname, val), put([(fi, val), (5, 30.0)]), ("box", fi, val)))
    return S


def decode_scan(case, seed, part=None):
    """random logits with every plant_specs case at an anchor of its own (part: 0 / 1 = the even / odd specs, for a head too small for all).
    Returns (frames, [(name, frame, anchor, row, column, claim)])"""
    head = case.heads[0]
    C = head.classes
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, case.shape).astype(f32)
    specs = plant_specs(C)
    if part is not None:
        specs = specs[part::2]
    cells = head.w * head.h
    slots = rng.permutation(case.batch * 3 * cells)
    assert len(specs) <= len(slots)
    plants = []
    for s, (name, write, claim) in zip(slots, specs):
        f, rem = divmod(int(s), 3 * cells)
        k, cell = divmod(rem, cells)
        i, j = divmod(cell, head.w)
        v = anchor_vec(x, f, k, i, j, C)
        v[0:4] = rng.normal(0, 1, 4)
        v[4] = 5.0
        v[5:] = -1.0 - np.abs(rng.normal(0, 1, C))
        write(v)
        plants.append((name, f, k, i, j, claim))
    return x, plants


def check_plants(orc, case, frames, plants, fulls):
    """each planted case is what it claims in the ORACLE's eyes (fulls: the expected candidate list of every frame)"""
    head = case.heads[0]
    for name, f, k, i, j, claim in plants:
        one = cell_candidate(orc, case, head, frames[f], k, i, j)
        what = "%s: %s at frame %d anchor %d cell (%d, %d): %s" % (case.name, name, f, k, i, j, one)
        if len(one):
            assert any(c.tobytes() == one[0].tobytes() for c in fulls[f]), what
        if claim[0] == "type":
            assert len(one) == 1 and one[0]["type"] == claim[1] and one[0]["score"] > 0, what
        elif claim[0] == "absent":
            assert len(one) == 0, what
        elif claim[0] == "nan0":                                 # absent BECAUSE of the NaN: any number in its place and the cell emits
            assert len(one) == 0, what
            y = np.array(frames[f], f32)
            anchor_vec(y[None], 0, k, i, j, head.classes)[5] = 0.0
            assert len(cell_candidate(orc, case, head, y, k, i, j)) == 1, what
        elif claim[0] == "neginf":                               # conf = 1 / (1 + e^-bs (1 + inf)) = 0: a candidate of class 0 and score 0 when the threshold is 0
            if head.thresh > 0:
                assert len(one) == 0, what
            else:
                assert len(one) == 1 and one[0]["type"] == 0 and one[0]["score"] == 0, what
        else:
            _, fi, val = claim
            lo = one[0]["x1" if fi in (0, 2) else "y1"] if len(one) == 1 else None
            assert len(one) == 1 and one[0]["score"] > 0, what
            assert np.isnan(lo) if np.isnan(val) else (np.isinf(lo) if (fi >= 2 and val > 0) else np.isfinite(lo)), what


# ---- the threshold edge
THRESHOLDS = (".01", ".25", ".5", ".9", ".999", "0")


def ulp_walk(b0, n=64):
    """b0 - n ulps .. b0 + n ulps (2 n + 1 floats; -inf stays -inf on the way down)"""
    up, dn, v = [f32(b0)], [], f32(b0)
    for _ in range(n):
        v = np.nextafter(v, f32(np.inf))
        up.append(v)
    v = f32(b0)
    for _ in range(n):
        v = np.nextafter(v, f32(-np.inf))
        dn.append(v)
    return np.array(dn[::-1] + up, f32)


def threshold_case(thresh):
    return single("edge_t" + thresh.replace(".", "p"), 10, 10, 2, 2, thresh)


def threshold_edge(case):
    """frame 0: the class logit is +50, so 1 + e^-cs is 1 and conf = 1 / (1 + e^-bs), the bound the kernel's early-out tests (with 0.1 % slack, through
    __expf); objectness walks the 129 floats around logit(thresh).  Frame 1: class logits 0 (conf = 1 / (1 + 2 e^-bs), well below the bound) on the
    same walk, and one anchor at objectness +20.  Every other objectness is -20.  Returns (frames, [(frame, anchor, row, column)] of the walks)"""
    head = case.heads[0]
    t = float(head.thresh_text)
    b0 = f32(np.log(t / (1.0 - t))) if t > 0 else f32(-np.inf)
    walk = ulp_walk(b0)
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1, case.shape).astype(f32)
    x[:, 4::7] = -20.0
    cells = head.w * head.h
    slots = rng.permutation(3 * cells)
    where = []
    for f in range(2):
        for n, s in enumerate(slots[:len(walk) + 1]):
            k, cell = divmod(int(s), cells)
            i, j = divmod(cell, head.w)
            v = anchor_vec(x, f, k, i, j, 2)
            if n == len(walk):
                if f == 1:
                    v[4], v[5], v[6] = 20.0, 0.0, 0.0
                continue
            v[4] = walk[n]
            v[5:7] = ((50.0, -50.0) if n % 2 else (-50.0, 50.0)) if f == 0 else (0.0, 0.0)
            where.append((f, k, i, j))
    return x, where


def edge_passes(orc, case, frames, where):
    """which anchors of the walks the ORACLE emits"""
    return [len(cell_candidate(orc, case, case.heads[0], frames[f], k, i, j)) == 1 for f, k, i, j in where]


# ---- many candidates: threshold 0, Gaussian logits (sigma 2), every anchor a candidate
SCRATCH_HEAD = (2731, 1)                                     # 8193 slots: the smallest head whose NMS takes the global scratch
MANY = [("20x20", 20, 20, 3, 1), ("65x42 (8190 slots, the largest LDS case)", 65, 42, 2, 1), ("scratch", SCRATCH_HEAD[0], SCRATCH_HEAD[1], 2, 1)]
TIE_FREE = (20, 20, 3, 1)                                   # w, h, batch, seed: a list without equal scores, which goes through plain orc.nms


def many_case(w, h, batch, classes=2):
    return single("many_%dx%d_b%d" % (w, h, batch), w, h, classes, batch, "0")


# ---- record size: K disjoint tiny boxes
RECORD_KS = (0, 1, 127, 128, 129)


def record_case(batch):
    return single("records_b%d" % batch, 16, 16, 1, batch, ".5")


def record_frames(case, ks, seed=3):
    """frame f: ks[f] passing anchors, one per chosen cell, tx = ty = 0 and tw = th = -6 (boxes of 0.04 pixels in the middle of their cells),
    scores pairwise distinct; every other objectness is -20"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, case.shape).astype(f32)
    x[:, 4::6] = -20.0
    for f, K in enumerate(ks):
        for n, cell in enumerate(rng.permutation(256)[:K]):
            v = anchor_vec(x, f, n % 3, int(cell) // 16, int(cell) % 16, 1)
            v[:] = (0.0, 0.0, -6.0, -6.0, 3.0 + 0.01 * n, 5.0)
    return x


# ---- zero scores
def zero_case():
    return single("zero_scores", 8, 8, 3, 2, "0")


def zero_frames(case, seed=11, nzero=5):
    """Gaussian logits at threshold 0; class 2 wins nowhere (-30) but at nzero anchors per frame with objectness -100 (conf = +0) and tiny boxes in
    cells of their own: no other box of their class touches them.  One more anchor per frame has every class at -inf (conf 0 whatever its
    objectness, class 0 in the reference).  Returns (frames, [(frame, anchor, row, column, class)])"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, case.shape).astype(f32)
    x[:, 7::8] = -30.0
    where = []
    for f in range(case.batch):
        for n, cell in enumerate(rng.permutation(64)[:nzero + 1]):
            k, i, j = n % 3, int(cell) // 8, int(cell) % 8
            v = anchor_vec(x, f, k, i, j, 3)
            v[0:4] = (0.0, 0.0, -6.0, -6.0)
            if n < nzero:
                v[4], v[7] = -100.0, 30.0
                where.append((f, k, i, j, 2))
            else:
                v[4], v[5:8] = 5.0, -np.inf
                where.append((f, k, i, j, 0))
    return x, where
