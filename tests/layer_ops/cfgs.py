"""Tiny darknet cfgs for the layer-op tests: a 1x1 linear conv (or nothing: the op reads the net input), the op layers under test, a 1x1 conv
with 3 * (5 + 1) filters and a yolo head.  A Cfg records, per op layer, which layers it reads (so a test can apply the oracle's operator to the
executor's own copy of them) and, per plan, the launches the executor is expected to make for it -- stated by the author of each cfg, not derived
from the planner's rules, so a plan that silently changes (a pool that is no longer merged, a route that became a copy) fails the test."""
import numpy as np

ACT = {"linear": 0, "relu": 1, "leaky": 2}
SPP_MAX_PLANE = 8192             # the planner merges stride-1 max pools of one tensor up to this many pixels per plane


class Op:
    def __init__(self, layer, kind, src, **kw):
        self.layer, self.kind, self.src = layer, kind, list(src)      # src: REAL layers (aliases resolved), -1 = the net input
        self.size = kw.get("size", 0)
        self.stride = kw.get("stride", 1)
        self.act = kw.get("act", 0)
        self.merged = kw.get("merged", False)                         # max pool that a fused plan runs inside k_spp

    def __repr__(self):
        return "%s@%d(size %d stride %d act %d src %s)" % (self.kind, self.layer, self.size, self.stride, self.act, self.src)


class Cfg:
    def __init__(self, name, w, h, c, batch):
        self.name, self.w, self.h, self.c, self.batch = name, w, h, c, batch
        self.text = ["[net]\nwidth=%d\nheight=%d\nchannels=%d\n" % (w, h, c)]
        self.shape = []          # (c, h, w) of every layer's output
        self.real = []           # layer -> the layer whose tensor it is (dropout / one-source route: an alias; -1: the net input)
        self.kind = []
        self.ops = []
        self.steps = {True: [], False: []}        # expected layer_of of the launches (layers >= 0), fused plan / FFGPU_NO_FUSE plan
        self.extra = {True: 1, False: 2}          # launches that belong to no layer: the NMS, and the counter clear of an unfused plan
        self._staged = False
        self._last_pool = None                    # real source of the step just emitted when it is a stride-1 max pool

    # ---- plumbing
    @property
    def n(self):
        return len(self.shape)

    def out_shape(self, layer):
        return (self.c, self.h, self.w) if layer < 0 else self.shape[layer]

    def _add(self, kind, text, shape, real=None):
        self.text.append(text)
        self.kind.append(kind)
        self.shape.append(shape)
        self.real.append(self.n - 1 if real is None else real)
        return self.n - 1

    def _step(self, layer, fused=True, plain=True, times=1):
        if fused:
            self.steps[True] += [layer] * times
        if plain:
            self.steps[False] += [layer] * times
        self._last_pool = None

    def tip(self):
        """the real layer whose tensor the next layer reads"""
        return self.real[self.n - 1] if self.n else -1

    def _reads_input(self):
        """a pool / upsample / shortcut that reads the net input: frame-major -> CNHW staging first when the batch has several frames"""
        if self.batch > 1 and not self._staged:
            self._staged = True
            self.extra[True] += 1
            self.extra[False] += 1

    def _goto(self, src):
        """make `src` (a real layer, -1 = the net input behind a leading dropout) the chain input of the next layer"""
        if src is None or src == self.tip():
            return
        if src < 0:
            assert self.kind[0] == "dropout", "the net input can only be routed through a dropout at layer 0"
            self._add("route", "[route]\nlayers=%d\n" % (0 - self.n), self.shape[0], -1)
        else:
            self._add("route", "[route]\nlayers=%d\n" % (src - self.n), self.shape[src], self.real[src])

    # ---- layers
    def dropout(self):
        return self._add("dropout", "[dropout]\nprobability=.5\n", self.out_shape(self.n - 1), self.tip())

    def conv(self, filters, act="linear", src=None, size=1, groups=1, stride=1):
        """1x1 by default; size > 1: "same" padding (pad=1 in a cfg: size / 2), so that at stride 1 the plane keeps its shape; stride 2 halves an even plane"""
        self._goto(src)
        c, h, w = self.out_shape(self.n - 1)
        assert size % 2 == 1 and c % groups == 0 and filters % groups == 0 and (stride == 1 or (h % stride == 0 and w % stride == 0))
        i = self._add("conv", "[convolutional]\nfilters=%d\nsize=%d\nstride=%d\npad=%d\n%sactivation=%s\n" % (
            filters, size, stride, 1 if size > 1 else 0, "groups=%d\n" % groups if groups > 1 else "", act), (filters, (h - 1) // stride + 1, (w - 1) // stride + 1))
        self._step(i)
        return i

    def absorbed_shortcut(self, frm, act="linear"):
        """out = act(the conv right in front + layer `frm`), the form a fused plan absorbs into that conv's epilogue (ffgpu_plan.hpp: the conv is read by
        nobody else and `frm` is a tensor of its own, not the net input): no launch of its own there, one k_add_act launch in an unfused plan.  Not an op
        of verify(): tests/conv_kernels checks it against the float64 restatement of the conv."""
        assert self.kind[self.n - 1] == "conv" and frm >= 0 and self.real[frm] >= 0
        assert self.out_shape(self.n - 1) == self.out_shape(self.real[frm])
        i = self._add("shortcut", "[shortcut]\nfrom=%d\nactivation=%s\n" % (frm - self.n, act), self.out_shape(self.n - 1))
        self._step(i, fused=False)
        return i

    def pool(self, kind, size, stride, src=None, _merge=None):
        assert kind in ("max", "avg")
        self._goto(src)
        s = self.tip()
        c, h, w = self.out_shape(self.n - 1)
        assert w // stride >= 1 and h // stride >= 1
        if kind == "max" and stride == 1 and _merge is None:
            # two stride-1 max pools of one tensor in a row would be merged by a fused plan: spp() is the way to ask for that
            assert self._last_pool is None or self._last_pool != s, "adjacent stride-1 max pools of layer %d: use spp()" % s
        i = self._add(kind + "pool", "[%spool]\nsize=%d\nstride=%d\n" % (kind, size, stride), (c, h // stride, w // stride))
        if s < 0:
            self._reads_input()
        self.ops.append(Op(i, kind + "pool", [s], size=size, stride=stride, merged=bool(_merge)))
        self._step(i, fused=_merge != "tail")
        if kind == "max" and stride == 1:
            self._last_pool = s
        return i

    def spp(self, sizes, src=None):
        """the SPP block of a yolo cfg: stride-1 max pools of ONE tensor with one-source routes between them.  A fused plan merges them (three
        at the most) into one k_spp launch when the plane has at most SPP_MAX_PLANE pixels and the source is not read from the frames directly
        (batch 1 with the net input as the source)."""
        assert 2 <= len(sizes) <= 3
        self._goto(src)
        s = self.tip()
        c, h, w = self.out_shape(self.n - 1)
        merge = w * h <= SPP_MAX_PLANE and not (s < 0 and self.batch == 1)
        out = []
        for k, size in enumerate(sizes):
            out.append(self.pool("max", size, 1, src=s, _merge=("head" if k == 0 else "tail") if merge else "none"))
            if not merge:
                self.ops[-1].merged = False
        return out

    def upsample(self, stride, src=None):
        self._goto(src)
        s = self.tip()
        c, h, w = self.out_shape(self.n - 1)
        i = self._add("upsample", "[upsample]\nstride=%d\n" % stride, (c, h * stride, w * stride))
        if s < 0:
            self._reads_input()
        self.ops.append(Op(i, "upsample", [s], stride=stride))
        self._step(i)
        return i

    def shortcut(self, frm, act="linear", src=None):
        """out = act(chain input + layer `frm`); the chain input must not be a private conv output (a fused plan would absorb the add there)"""
        self._goto(src)
        s = self.tip()
        assert self.kind[self.n - 1] != "conv", "a conv right in front of the shortcut absorbs it"
        fr = -1 if frm < 0 else self.real[frm]
        assert self.out_shape(s) == self.out_shape(fr)
        i = self._add("shortcut", "[shortcut]\nfrom=%d\nactivation=%s\n" % ((0 if frm < 0 else frm) - self.n, act), self.out_shape(s))
        if s < 0 or fr < 0:
            self._reads_input()
        self.ops.append(Op(i, "shortcut", [s, fr], act=ACT[act]))
        self._step(i)
        return i

    def route(self, srcs, inplace):
        """a route of several sources.  inplace: what a fused plan does -- True when every source tensor can be placed inside the route's
        tensor (each once, none of them already inside another route), so no launch; False: one k_copy per source, as in every unfused plan"""
        assert len(srcs) >= 2 and all(s >= 0 for s in srcs)
        c = sum(self.shape[s][0] for s in srcs)
        _, h, w = self.shape[srcs[0]]
        i = self._add("route", "[route]\nlayers=%s\n" % ",".join(str(s - self.n) for s in srcs), (c, h, w))
        self.ops.append(Op(i, "route", [self.real[s] for s in srcs]))
        self._step(i, fused=not inplace, times=len(srcs))
        return i

    def tail(self, shrink=0):
        """the detection head every cfg needs; shrink: a strided pool first, so that a large plane does not become 10^5 candidates for the NMS"""
        if shrink:
            self.pool("avg", 1, shrink)
        i = self.conv(18)
        y = self._add("yolo", "[yolo]\nmask=0,1,2\nanchors=4,6, 8,12, 16,14\nclasses=1\nignore_thresh=.5\n", (0, 0, 0))
        self._step(y)
        return self

    def cfg_text(self):
        return "\n".join(self.text)


# ------------------------------------------------------------------------------------------------------------------------------- the cases
POOL_SIZES = (1, 2, 3, 4, 5, 9, 13)
POOL_PLANES = ((7, 5), (13, 11), (17, 1), (1, 9))          # (w, h)


def pool_grid(w, h, c, batch, first_layer=False, strides=(1, 2, 3)):
    """case 1: every size x stride 1..3 x max / avg of one plane through k_pool.  Strides that would leave an empty tensor (w / stride == 0)
    do not exist as nets.  Max and avg alternate, so no two stride-1 max pools follow each other (they would be merged)."""
    g = Cfg("pool_%dx%d_c%d_b%d%s%s" % (w, h, c, batch, "_in" if first_layer else "", "" if len(strides) == 3 else "_s" + "".join(map(str, strides))), w, h, c, batch)
    src = -1
    if first_layer:
        g.dropout()
    else:
        src = g.conv(c)
    for stride in strides:
        if w // stride < 1 or h // stride < 1:
            continue
        for size in POOL_SIZES:
            if size == 2 and stride == 2:
                g.pool("avg", size, stride, src=src)       # (max 2 / 2 is case 2's; here on w % 8 != 0 it is k_pool's as well)
                g.pool("max", size, stride, src=src)
            else:
                g.pool("max", size, stride, src=src)
                g.pool("avg", size, stride, src=src)
    return g.tail()


def pool_big():
    """8 channels x 3 frames of 256 x 192 at stride 1: 1 179 648 outputs > 4096 * 256, the grid-stride loop runs a second time"""
    g = Cfg("pool_big", 256, 192, 3, 3)
    s = g.conv(8)
    g.pool("max", 3, 1, src=s)
    g.pool("avg", 2, 1, src=s)
    return g.tail(shrink=32)


POOL2_W, POOL2_H = (8, 16, 24, 40, 136), (2, 6, 10)
POOL2_FALLBACK = ((12, 6), (20, 6), (16, 7))               # w % 8 != 0, odd h: k_pool


def pool2x2(w, h, first_layer=False, c=5, batch=3):
    g = Cfg("pool2x2_%dx%d%s" % (w, h, "_in" if first_layer else ""), w, h, c, batch)
    if first_layer:
        g.dropout()
        g.pool("max", 2, 2, src=-1)
    else:
        g.pool("max", 2, 2, src=g.conv(c))
    return g.tail()


SPP_PLANES = ((10, 10), (13, 7), (1, 12), (12, 1))
SPP_CASCADE = ((3, 5, 9), (5, 9, 13), (5, 9))
SPP_DIRECT = ((9, 5, 3), (5, 5), (2, 4), (3, 4, 9))


def spp(w, h, sizes_list, c=5, batch=3, first_layer=False, name=None):
    """several SPP blocks of one tensor; an avg pool between two blocks keeps them apart (15 planes at c 5 / batch 3: the last trip of a
    workgroup holds one plane)"""
    g = Cfg(name or "spp_%dx%d_c%d_b%d%s" % (w, h, c, batch, "_in" if first_layer else ""), w, h, c, batch)
    if first_layer:
        g.dropout()
        src = -1
    else:
        src = g.conv(c)
    for k, sizes in enumerate(sizes_list):
        if k:
            g.pool("avg", 1, 1, src=src)
        g.spp(sizes, src=src)
    return g.tail()


def spp_many_planes():
    """129 channels x 65 frames of 4 x 4: 8385 planes > 2 * 4096, so a workgroup loops, and the count is odd"""
    return spp(4, 4, [(3, 5, 9)], c=129, batch=65, name="spp_many_planes")


SPP_EDGE_PLANES = ((64, 64), (80, 52), (128, 64), (128, 65))   # 64 KB of LDS exactly, just above, 128 KB (the largest merged plane), not merged


def upsample_grid(w, h, c=3, batch=2, first_layer=False):
    g = Cfg("upsample_%dx%d_c%d_b%d%s" % (w, h, c, batch, "_in" if first_layer else ""), w, h, c, batch)
    if first_layer:
        g.dropout()
        src = -1
    else:
        src = g.conv(c)
    for stride in (1, 2, 3, 4):
        g.upsample(stride, src=src)
    return g.tail()


UPSAMPLE_PLANES = ((1, 1), (1, 7), (7, 1), (3, 5), (13, 17), (20, 20), (257, 3))


def upsample_big():
    """8 x 3 x 256 x 192 = 1 179 648 input elements > 4096 * 256: k_upsample32's grid-stride loop runs a second time"""
    g = Cfg("upsample_big", 256, 192, 3, 3)
    g.upsample(2, src=g.conv(8))
    return g.tail(shrink=32)


def upsample_wide():
    """4096 x 4, 16 channels, batch 4: n_in * w = 2^32 exactly, the smallest reach of the 64-bit k_upsample"""
    g = Cfg("upsample_wide", 4096, 4, 3, 4)
    g.upsample(2, src=g.conv(16))
    return g.tail(shrink=8)


def shortcuts(w, h, c, batch, name=None):
    """case 6: shortcuts no conv can absorb -- behind a pool, behind a route, with the net input as one side (either side) -- in all three
    activations, and routes that must copy: two and three sources with odd element counts"""
    g = Cfg(name or "add_%dx%d_c%d_b%d" % (w, h, c, batch), w, h, c, batch)
    g.dropout()                                            # layer 0: the net input under a layer number
    a = g.conv(c)
    b = g.conv(c, act="leaky", src=a)
    for act in ("linear", "leaky", "relu"):
        g.pool("avg", 1, 1, src=a)
        g.shortcut(b, act)                                 # behind a pool
        g.shortcut(b, act, src=a)                          # behind a route
        g.shortcut(-1, act, src=b)                         # the net input as the `from` side
        g.shortcut(a, act, src=-1)                         # ... and as the chain side
    return g.tail()


ADD_SHAPES = ((7, 5, 3, 1), (5, 7, 3, 2), (3, 3, 3, 1), (4, 3, 1, 2))      # (w, h, c, batch): 105, 210, 27 and 24 elements -- n % 4 = 1, 2, 3, 0
ROUTE_SHAPES = ((7, 5, 1), (3, 3, 3))                                   # (w, h, batch)


def shortcut_big():
    """8 x 3 x 512 x 352 = 4 325 376 elements > 4 Mi: k_add_act's grid-stride loop runs a second time (4096 workgroups x 256 lanes x 4)"""
    g = Cfg("add_big", 512, 352, 3, 3)
    a = g.conv(8)
    b = g.conv(8, act="leaky", src=a)
    g.shortcut(b, "leaky", src=a)
    return g.tail(shrink=32)


def routes(w, h, batch):
    """routes through k_copy with sources of 3, 5 and 1 channels on an odd plane: odd element counts, so the second and third destination are
    not 16-byte aligned.  In a fused plan the first route of a tensor is built in place (no launch); a second route of the same tensors copies."""
    g = Cfg("route_%dx%d_b%d" % (w, h, batch), w, h, 3, batch)
    a = g.conv(3)
    b = g.conv(5, src=a)
    c = g.conv(1, src=a)
    g.route([a, b], inplace=True)
    g.route([b, a], inplace=False)
    g.route([c, b, a], inplace=False)
    g.route([a, a], inplace=False)
    return g.tail()


def route_big():
    """a route of one 8 x 3 x 512 x 352 tensor twice: 4 325 376 elements per copy > 4 Mi, so k_copy's grid-stride loop runs a second time (the
    same tensor twice cannot be built in place, so the fused plan copies as well)"""
    g = Cfg("route_big", 512, 352, 3, 3)
    a = g.conv(8)
    g.route([a, a], inplace=False)
    return g.tail(shrink=32)


def every_cfg():
    """every cfg the GPU tests use (the CPU test loads each of them in the oracle)"""
    out = []
    for (w, h) in POOL_PLANES:
        out += [pool_grid(w, h, 3, 2), pool_grid(w, h, 5, 1)]
    out += [pool_big()]
    out += [pool2x2(w, h) for w in POOL2_W for h in POOL2_H] + [pool2x2(w, h) for (w, h) in POOL2_FALLBACK]
    out += [spp(w, h, SPP_CASCADE, name="spp_cascade_%dx%d" % (w, h)) for (w, h) in SPP_PLANES]
    out += [spp(w, h, SPP_DIRECT, name="spp_direct_%dx%d" % (w, h)) for (w, h) in SPP_PLANES]
    out += [spp_many_planes()] + [spp(w, h, [(3, 5, 9)], c=3, batch=1) for (w, h) in SPP_EDGE_PLANES]
    out += [upsample_grid(w, h) for (w, h) in UPSAMPLE_PLANES] + [upsample_big(), upsample_wide()]
    out += [shortcut_big(), route_big()]
    out += [make() for (_, make, _, _) in NONFINITE_CASES]          # (the first-layer cfgs, the shortcut and the route cfgs are all among them)
    out = list({g.name: g for g in out}.values())                  # (a few cases use the same cfg with other inputs)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the inputs
SPECIALS = np.array([0x7fc00000, 0x7f800000, 0xff800000, 0x80000000, 0x7fc12345, 0xffc00001], np.uint32).view(np.float32)
#                    NaN         +Inf        -Inf        -0          NaN with a payload, negative NaN


def special_positions(h, w):
    """interior, the four corners, the last row, and -- every pixel of a stride-1 plane being some window's first element and some other
    window's centre -- pixels that are first (even / even) and not first (odd / odd) in a 2 x 2 / stride 2 window"""
    pos = [(h // 2, w // 2), (0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (h - 1, w // 3), (2 * (h // 4), 2 * (w // 4)), (min(1, h - 1), min(3, w - 1)),
           (h // 3, (2 * w) // 3)]
    return list(dict.fromkeys(pos))


def crafted_frames(g, seed, pixel=False, every=3, block=False):
    """(batch, c, h, w) frames in [-1, 1) with exact zeros and the SPECIALS at special_positions.  pixel=False: one channel per position (the
    values rotate over positions, channels and frames; every `every`-th plane stays finite, so launches see finite and non-finite planes side
    by side).  pixel=True: NaN in EVERY channel of two pixels and one +-Inf in ONE channel of two others -- what survives a 1x1 conv.
    block: the last 7 rows x 7 columns of one otherwise finite plane of frame 0 are -Inf (pixel=True: +Inf in channel 0, which a conv turns into
    either sign per output channel) -- a max pool gives -Inf only where its whole window is -Inf, and the clipped window of size 13 in that corner
    is 7 x 7."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (g.batch, g.c, g.h, g.w)).astype(np.float32)
    x[rng.uniform(0, 1, x.shape) < 0.05] = 0.0
    pos = special_positions(g.h, g.w)
    if pixel:
        for f in range(g.batch):
            (y0, x0), (y1, x1) = pos[f % len(pos)], pos[(f + 2) % len(pos)]
            x[f, :, y0, x0] = SPECIALS[0]
            x[f, :, y1, x1] = SPECIALS[4]
            (y2, x2), (y3, x3) = pos[(f + 1) % len(pos)], pos[(f + 3) % len(pos)]
            if (y2, x2) not in ((y0, x0), (y1, x1)):
                x[f, f % g.c, y2, x2] = SPECIALS[1]
            if (y3, x3) not in ((y0, x0), (y1, x1), (y2, x2)):
                x[f, (f + 1) % g.c, y3, x3] = SPECIALS[2]
        if block:
            x[0, 0, max(g.h - 7, 0):, max(g.w - 7, 0):] = SPECIALS[1]
        return x
    k = 0
    for f in range(g.batch):
        for ch in range(g.c):
            if (f * g.c + ch) % every == every - 1:
                continue
            for j, (yy, xx) in enumerate(pos):
                x[f, ch, yy, xx] = SPECIALS[(k + j) % len(SPECIALS)]
            k += 1
    if block:
        x[0, min(every, g.c) - 1, max(g.h - 7, 0):, max(g.w - 7, 0):] = SPECIALS[2]
    return x


def inf_frames(g, seed):
    """+Inf, -Inf and -0 at special_positions of every plane, the -Inf block of crafted_frames in one of them, and NO NaN: non-finite data for the
    path of k_spp that planes without a NaN take (the cascade)"""
    x = plain_frames(g, seed)
    pos = special_positions(g.h, g.w)
    for f in range(g.batch):
        for ch in range(g.c):
            for j, (yy, xx) in enumerate(pos):
                x[f, ch, yy, xx] = SPECIALS[1 + (f * g.c + ch + j) % 3]
    x[0, g.c - 1, max(g.h - 7, 0):, max(g.w - 7, 0):] = SPECIALS[2]
    assert not np.isnan(x).any()
    return x


def plain_frames(g, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (g.batch, g.c, g.h, g.w)).astype(np.float32)
    x[rng.uniform(0, 1, x.shape) < 0.05] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------- reference and comparison
def expected(orc, op, srcs):
    """the oracle's operator on the given source tensors ((c, h, w) each)"""
    if op.kind in ("maxpool", "avgpool"):
        return orc.pool(srcs[0], op.size, op.stride, 1 if op.kind == "maxpool" else 0)
    if op.kind == "upsample":
        return orc.upsample(srcs[0], op.stride)
    if op.kind == "shortcut":
        return orc.shortcut(srcs[0], srcs[1], op.act)
    assert op.kind == "route"
    return np.concatenate(srcs, axis=0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(op, got, want, what, spp=False):
    """upsample / route: identical bits, NaN payloads and -0 included.  Pools through k_pool / k_pool2x2 (the reference's scan order), avg pool
    and shortcut (one rounding per operation, the same operations): identical NaN pattern, identical bits elsewhere.  spp: a max pool that ran
    inside k_spp -- identical NaN pattern, equal VALUES elsewhere; the sign of a zero maximum is not compared there: the cascade takes maxima of
    maxima (rows, then columns, each size from the previous one), and which of +0 / -0 `v < t ? t : v` keeps depends on the order they are met
    in, which only the reference's own scan reproduces."""
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if op.kind in ("upsample", "route"):
        bad = bits(got) != bits(want)
        assert not bad.any(), "%s: %d of %d elements differ in bits, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist())
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN pattern differs at %s (got NaN: %s)" % (what, np.argwhere(gn != wn)[:4].tolist(), gn[gn != wn][:4].tolist())
    if spp:
        bad = ~wn & (got != want)
    else:
        bad = ~wn & (bits(got) != bits(want))
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def assert_nonfinite_reach(seen, spp_only=False):
    """the inputs did their job: +Inf and -Inf both occur in the expected outputs, and the oracle has a NaN at a position where the input has
    none -- for EVERY stride-1 max pool of size >= 3 (the window's first element is not its centre there), which is what a k_spp that leaves a
    NaN where it was gets wrong"""
    allw = np.concatenate([w.ravel() for (_, op, _, _, w) in seen if op.kind == "maxpool" and op.size >= 2 and (op.merged or not spp_only)])
    assert np.isposinf(allw).any() and np.isneginf(allw).any() and np.isnan(allw).any()
    moved = {}
    for plan, op, f, srcs, want in seen:
        if op.kind == "maxpool" and op.stride == 1 and op.size >= 3 and (op.merged or not spp_only):
            moved[(plan, op.layer)] = moved.get((plan, op.layer), False) or bool((np.isnan(want) & ~np.isnan(srcs[0])).any())
    assert moved and all(moved.values()), moved


def verify(orc, g, read, frames, plan, merged):
    """every op layer of `g`, every frame: read(op layer, frame) against the oracle's operator on read(source layer, frame).  merged: the plan
    runs the SPP pools inside k_spp.  Returns [(plan, op, frame, sources, expected)] for the assertions a test makes about its inputs."""
    cache, seen = {}, []

    def tensor(layer, f):
        if (layer, f) not in cache:
            cache[(layer, f)] = read(layer, f)
            if layer < 0:
                assert np.array_equal(bits(cache[(layer, f)]), bits(frames[f])), "the net input read back differs from the frames"
        return cache[(layer, f)]
    for op in g.ops:
        for f in range(g.batch):
            srcs = [tensor(s, f) for s in op.src]
            want = expected(orc, op, srcs)
            got = read(op.layer, f)
            check(op, got, want, "%s, %s plan, frame %d, %r" % (g.name, plan, f, op), spp=merged and op.merged)
            cache[(op.layer, f)] = got
            seen.append((plan, op, f, srcs, want))
    return seen


def pool2x2_skips_nan(seen):
    """a NaN that is not its 2 x 2 window's first element is skipped: some non-NaN output has one in its window"""
    for _, op, _, srcs, want in seen:
        c, h, w = srcs[0].shape
        win = np.isnan(srcs[0]).reshape(c, h // 2, 2, w // 2, 2).any(axis=(2, 4))
        if (win & ~np.isnan(want)).any():
            return True
    return False


# (name, cfg, frames, purpose) -- shared by the GPU test and tests/test_layer_ops_ref.py
NONFINITE_CASES = [
    ("pools 13x11 batch 2 input", lambda: pool_grid(13, 11, 3, 2, first_layer=True), lambda g: crafted_frames(g, 8, block=True, every=4), "pools"),
    ("pools 7x5 batch 1 input", lambda: pool_grid(7, 5, 5, 1, first_layer=True), lambda g: crafted_frames(g, 8, block=True, every=4), "pools"),
    # (strides 1 only: a net the reference itself can run, see tests/test_layer_ops_ref.py)
    ("pools 13x11 stride 1 batch 2 input", lambda: pool_grid(13, 11, 3, 2, first_layer=True, strides=(1,)), lambda g: crafted_frames(g, 8, block=True, every=4), "pools"),
    ("pools behind conv", lambda: pool_grid(13, 11, 3, 2), lambda g: crafted_frames(g, 9, block=True, pixel=True), "pools"),
    ("pool2x2 24x6 batch 3 input", lambda: pool2x2(24, 6, first_layer=True), lambda g: crafted_frames(g, 10, block=True, every=4), "pool2x2"),
    ("pool2x2 40x10 batch 1 input", lambda: pool2x2(40, 10, first_layer=True, batch=1), lambda g: crafted_frames(g, 10, block=True, every=4), "pool2x2"),
    ("pool2x2 16x6 behind conv", lambda: pool2x2(16, 6), lambda g: crafted_frames(g, 10, block=True, pixel=True), "pool2x2"),
    # batch 1: the pools read the frames directly and stay three launches; batch 2: they read the staged CNHW copy and are merged
    ("spp 10x10 batch 1 input", lambda: spp(10, 10, [(3, 5, 9)], c=3, batch=1, first_layer=True), lambda g: crafted_frames(g, 7, block=True), "pools unmerged"),
    ("spp 10x10 batch 2 input", lambda: spp(10, 10, [(3, 5, 9)], c=3, batch=2, first_layer=True), lambda g: crafted_frames(g, 7, block=True), "spp"),
    ("spp 13x11 every form input", lambda: spp(13, 11, list(SPP_CASCADE + SPP_DIRECT), c=4, batch=2, first_layer=True, name="spp_nonfinite_in"),
     lambda g: crafted_frames(g, 11, block=True), "spp"),
    ("spp 13x11 cascade, Inf and -0 without NaN", lambda: spp(13, 11, SPP_CASCADE, c=4, batch=2, first_layer=True, name="spp_inf_in"),
     lambda g: inf_frames(g, 20), "spp cascade"),
    ("spp 10x10 behind conv", lambda: spp(10, 10, [(3, 5, 9)]), lambda g: crafted_frames(g, 12, block=True, pixel=True), "spp"),
    ("upsample 13x17 batch 2 input", lambda: upsample_grid(13, 17, first_layer=True), lambda g: crafted_frames(g, 14), "bits"),
    ("upsample 3x5 batch 1 input", lambda: upsample_grid(3, 5, batch=1, first_layer=True), lambda g: crafted_frames(g, 14), "bits"),
] + [("shortcuts %dx%d c%d batch %d" % a, (lambda a=a: shortcuts(*a)), lambda g: crafted_frames(g, 17, pixel=True), "add") for a in ADD_SHAPES] \
  + [("routes %dx%d batch %d" % a, (lambda a=a: routes(*a)), lambda g: crafted_frames(g, 19, pixel=True), "copy") for a in ROUTE_SHAPES]


def assert_inputs_reach(purpose, g, seen):
    """what a non-finite case's inputs must achieve, or the test would pass without testing"""
    allw = np.concatenate([w.ravel() for (_, _, _, _, w) in seen])
    merged = any(op.merged and plan == "fused" for (plan, op, _, _, _) in seen)
    if purpose == "spp cascade":                              # no NaN anywhere: every workgroup trip of k_spp takes the cascade, with +-Inf in it
        assert merged and not np.isnan(allw).any() and not any(np.isnan(s).any() for (_, _, _, srcs, _) in seen for s in srcs)
        pools = np.concatenate([w.ravel() for (_, op, _, _, w) in seen if op.merged and op.size >= 3])
        assert np.isposinf(pools).any() and np.isneginf(pools).any() and (pools == 0).any()
        return
    assert np.isnan(allw).any()
    if purpose in ("pools", "pools unmerged", "spp"):
        assert merged == (purpose == "spp")
        assert_nonfinite_reach(seen, spp_only=purpose == "spp")
    elif purpose == "pool2x2":
        assert np.isposinf(allw).any() and np.isneginf(allw).any()
        assert pool2x2_skips_nan(seen)
    elif purpose == "bits":                                   # every special value, bit for bit, in the expected outputs
        assert np.isin(bits(SPECIALS), np.concatenate([bits(w).ravel() for (_, _, _, _, w) in seen])).all()
    elif purpose == "add":
        assert sorted({op.act for (_, op, _, _, _) in seen if op.kind == "shortcut"}) == [0, 1, 2]
        adds = np.concatenate([w.ravel() for (_, op, _, _, w) in seen if op.kind == "shortcut"])
        assert np.isnan(adds).any() and (np.isinf(adds).any() or g.c == 1)      # (one channel: +Inf and -Inf may meet in every sum)
    else:
        assert purpose == "copy" and np.isinf(allw).any()
