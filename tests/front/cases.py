"""The table of cases of tests/front: k_front (ffgpu_front.inc), the net's first four layers as one launch, reached through a four-layer headless net whose
filter rows the test writes itself.  tests/test_front_ref.py holds the table to its purpose without a GPU (the coverage list below is asserted from the table, every
case's probe line names the instantiation the rule gives, the oracle meets the hard bound, the touched set of the geometry is front64's non-finite set);
tests/front/test_gpu_kernels.py runs every case on the device.

A Case is one executor: N frames, an 8-channel plane of W x H (the net input is 2 W x 2 H), FFGPU_FRONT_NC (None: unset), FFGPU_FRONT_BAND (None: the computed
default), the four activations (0 linear, 1 relu, 2 leaky) and a seed.  With NC output columns per lane a row takes lpr = ceil(W / NC) lanes and the last lane slides
left by sl = lpr NC - W columns (NC = 4: W % 4 == 0, sl = 0).

  CASES      part 1 (error bound, the fp32 form).  NC = 3: W = 8 (lpr 3, sl 1), 12 (sl 0), 16 (sl 2), 44 (lpr 15), 48 (lpr 16, sl 0: the last lane is lane 15),
             52 (lpr 18, sl 2: the seam crosses a DPP row), 184 / 188 / 192 (lpr 62 / 63 / 64, sl 2 / 1 / 0).  NC = 4: W = 4 (one lane; the knob says 3, the rule 4), 8,
             64 / 68 (last lanes 15 / 16), 196 (no knob: four columns because 66 lanes do not fit), 256 (lpr 64).  H = 1, H < band, H = band, H = band + 1, bands
             1, 2, 3, 16 and the default, odd and even band lengths, N x nbands not a multiple of 4.  Every activation in every slot.
  NF_CASES   part 3: planes wide enough to leave outputs untouched, both NC, several activation tuples, with +Inf, -Inf and NaN planted by plant()
  FORM_CASES part 2: the u8 / resizing BGR / NV12 forms against the fp32 form, bit for bit

Weights (make_inputs): blockref.make_filter rows; scale' is made NEGATIVE on channels 1 and 5 of layer 0, 2 of layer 1, 4 of the depthwise layer and 1 of layer 3,
and ZERO on channel 3 of layer 0 and 6 of the depthwise layer (part 3: on channel 2 of layer 3 only -- 0 x Inf = NaN on a middle channel would turn every touched
output into NaN, and the touched outputs are meant to hold all of NaN, +Inf and -Inf).

Part 3's weights are also made sign-definite where an Inf has to survive three more layers (plant()): under linear activations a lone +Inf in input channel 2
becomes +Inf on all eight channels of layers 0, 1 and 2 and +-Inf by the sign of the row in layer 3; every other planted value ends as NaN, as in the reference.
Magnitudes stay random.  Where plant() puts the values (each on a pixel of its own; rows and frames go round so that the footprints spread):
  corners        the four corners of the input (channel 2, frame 0): +Inf, -Inf, NaN, +Inf
  frame-seam     the last pixel of the last channel of frame N - 2 and the first pixel of frame N - 1
  lane           input columns 2 NC k - 1 and 2 NC k, both sides of a lane boundary: k = 1, and k = 16, 32 (DPP row boundaries) where the width has them
  seam           the first and the last input column the slid last lane shares with its neighbour, and the column just left of the overlap (sl = 0: the last
                 lane's first column and the one left of it)
  last-column    input column 2 W - 1
  band           input rows 2 y0 - 2 .. 2 y0 + 1 around the start y0 of the second band, which both bands read
  rows           an odd and an even input row, and row 2 H - 1
  pair           +Inf and -Inf at one pixel of channels 0 and 1: filter 0 of layer 0 has positive taps on both (NaN), filter 1 positive and negative (+Inf), filter 2
                 ZERO taps on channel 0 (0 x Inf = NaN, as in the reference)
touched() follows from the geometry alone: the 3x3 stride-2 footprint of the pixel in the 8-channel plane, dilated by the depthwise 3x3, in all four output channels."""
import collections
import functools

import numpy as np

from front import frontref
from irb_blocks import blockref
from irb_stage import nets

Case = collections.namedtuple("Case", "id N W H nc band acts seed")
INF, NAN = np.float32(np.inf), np.float32(np.nan)
ACT = nets.ACT


def nc_rule(knob, W):
    """ffgpu_front_nc: three columns per lane iff the knob (default 3) says 3, W >= 6 and the row fits a wave that way"""
    return 3 if (knob is None or knob == 3) and W >= 6 and (W + 2) // 3 <= 64 else 4


def default_band(N, H):
    """thin_band of ffgpu_conv_kernels.inc"""
    band = 2
    while band < 16 and N * H >= 640 * band * 2:
        band *= 2
    return band


def geometry(c):
    """NC, lpr, sl, band, nbands, ntasks, grid"""
    NC = nc_rule(c.nc, c.W)
    lpr = -(-c.W // NC)
    band = c.band if c.band is not None else default_band(c.N, c.H)
    nbands = -(-c.H // band)
    return NC, lpr, lpr * NC - c.W, band, nbands, c.N * nbands, (c.N * nbands + 3) // 4


# (N, W, H, FFGPU_FRONT_NC, FFGPU_FRONT_BAND, activations)
TABLE = [
    (1, 8, 1, 3, None, (1, 2, 0, 2)),          # H = 1 < the default band; one task: a ragged workgroup
    (2, 12, 3, 3, 3, (0, 1, 2, 0)),            # H = band, an odd band length
    (3, 16, 4, 3, 3, (2, 0, 1, 1)),            # H = band + 1: a last band of one row; 6 tasks
    (1, 44, 5, 3, 2, (2, 2, 2, 0)),            # even bands and an odd last one
    (1, 48, 9, 3, 16, (1, 1, 1, 2)),           # H < band 16
    (2, 52, 7, 3, 1, (0, 0, 0, 0)),            # band 1: every row re-expands both neighbours; 14 tasks
    (1, 184, 2, 3, 2, (2, 1, 2, 1)),
    (1, 188, 3, 3, 2, (1, 2, 0, 0)),
    (5, 192, 2, 3, 1, (2, 2, 2, 0)),           # no idle lane; 10 tasks
    (1, 4, 9, 3, 3, (1, 0, 2, 2)),             # NC = 3 is refused below 6 columns
    (5, 8, 1, 4, 1, (0, 2, 1, 0)),
    (1, 64, 4, 4, 16, (2, 2, 2, 0)),
    (2, 68, 5, 4, 2, (2, 1, 0, 1)),
    (1, 196, 3, None, None, (2, 2, 2, 0)),     # default four-column territory
    (1, 256, 2, 4, 1, (0, 2, 2, 2)),
]
NF_TABLE = [
    (3, 16, 9, 3, 4, (0, 0, 0, 0)),
    (3, 16, 9, 3, 4, (1, 1, 1, 1)),
    (2, 52, 8, 3, 3, (2, 2, 2, 0)),
    (2, 52, 8, 3, 3, (1, 2, 0, 2)),
    (2, 188, 6, 3, 2, (2, 1, 2, 0)),
    (2, 192, 5, 3, None, (0, 2, 1, 2)),
    (4, 12, 9, 4, 3, (2, 0, 2, 1)),
    (2, 68, 7, 4, 4, (1, 2, 2, 0)),
    (2, 196, 5, None, 2, (0, 1, 0, 2)),
]
# part 2: (W, H, FFGPU_FRONT_NC, FFGPU_FRONT_BAND); the resizing forms exist at NC = 3 only
FORM_TABLE = [(8, 5, 3, 2), (12, 4, 3, None), (16, 3, 3, 3), (52, 4, 3, 2), (188, 3, 3, None), (8, 3, 4, 2), (68, 4, 4, None)]
FORM_ACTS = (2, 2, 2, 0)
FORM_N = 10
# mean and norm of part 2: not (0, 1 / 255), one norm negative
MEAN, NORM = (104.0, 117.5, 123.25), (0.017, -0.0175, 0.0171)


def _id(N, W, H, nc, band, acts):
    return "w%d-h%d-n%d-nc%s-band%s-act%d%d%d%d" % ((W, H, N, "x" if nc is None else nc, "x" if band is None else band) + tuple(acts))


def _cases(table, seed, tag=""):
    out = [Case(_id(*row) + tag, *row, seed + k) for k, row in enumerate(table)]
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases(TABLE, 11000)
NF_CASES = _cases(NF_TABLE, 12000, "-nf")
FORM_CASES = [Case("w%d-h%d-nc%d-band%s" % (W, H, nc, "x" if band is None else band), FORM_N, W, H, nc, band, FORM_ACTS, 13000 + k) for k, (W, H, nc, band) in enumerate(FORM_TABLE)]
IDS, NF_IDS, FORM_IDS = ([c.id for c in t] for t in (CASES, NF_CASES, FORM_CASES))


def cfg_text(c):
    return "[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (2 * c.W, 2 * c.H) + nets.conv(8, 3, ACT[c.acts[0]], stride=2) + nets.conv(8, 1, ACT[c.acts[1]]) + \
        nets.conv(8, 3, ACT[c.acts[2]], groups=8) + nets.conv(4, 1, ACT[c.acts[3]])


def layers(f0, f1, fd, f2):
    """what nets.put takes"""
    return [(0, 27, f0), (1, 8, f1), (2, 9, fd), (3, 8, f2)]


def env(c):
    e = {"FFGPU_FRONT_MIN_PX": "1"}
    if c.nc is not None:
        e["FFGPU_FRONT_NC"] = str(c.nc)
    if c.band is not None:
        e["FFGPU_FRONT_BAND"] = str(c.band)
    return e


def set_switches(monkeypatch, c, **more):
    """every variable the library reads unset, then the case's"""
    from test_irb_choice import knob_names
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)
    for k, v in dict(env(c), **more).items():
        monkeypatch.setenv(k, v)


def plan_line(probe, c, form="f32"):
    """under set_switches(c)"""
    return probe(c.N, c.W, c.H, form)


def want_line(c, form="f32"):
    """the line the probe must write, from the rule and the launch arithmetic restated here"""
    NC, _, _, band, nbands, ntasks, grid = geometry(c)
    if form in ("bgr_frames", "nv12_frames") and NC != 3:
        return "staged"
    return "front<4,%d,%d,%d,%d> W=%d H=%d N=%d band=%d nbands=%d ntasks=%d grid=%d block=256" % (
        form != "f32", NC, form in ("bgr_frames", "nv12_frames"), form == "nv12_frames", c.W, c.H, c.N, band, nbands, ntasks, grid)


def make_inputs(c, nf=False):
    """frames (N, 3, 2H, 2W) uniform(-1, 1) and the four layers' filter rows"""
    rng = np.random.default_rng(c.seed)
    frames = rng.uniform(-1, 1, (c.N, 3, 2 * c.H, 2 * c.W)).astype(np.float32)
    f0, f1, fd, f2 = (blockref.make_filter(rng, fn, K) for fn, K in ((8, 27), (8, 8), (8, 9), (4, 8)))
    for f, k4, neg in ((f0, 28, (1, 5)), (f1, 8, (2,)), (fd, 12, (4,)), (f2, 8, (1,))):
        f[list(neg), k4] *= -1
    if nf:
        f2[2, 8] = 0.0
    else:
        f0[3, 28] = 0.0
        fd[6, 12] = 0.0
    return frames, f0, f1, fd, f2


# ---- part 3
def placements(c):
    """[(channel, frame, input row, input column, value, what)], each pixel once"""
    N, W, H = c.N, c.W, c.H
    NC, lpr, sl, band, nbands, _, _ = geometry(c)
    IW, IH = 2 * W, 2 * H
    out, used = [], set()
    turn = [0]
    vals = (INF, -INF, NAN)

    def put(ch, n, y, x, v, what):
        pos = (ch, min(max(n, 0), N - 1), min(max(y, 0), IH - 1), min(max(x, 0), IW - 1))
        if pos not in used:
            used.add(pos)
            out.append(pos + (v, what))

    def col(x, what, y=None):
        """a value at input column x: the value, the frame and (unless given) the row go round; +-Inf in channel 2, NaN in any"""
        if not 0 <= x < IW:
            return
        k = turn[0]
        turn[0] += 1
        v = vals[k % 3]
        put(2 if v is not NAN else k % 2, k % N, (3 + 5 * k) % IH if y is None else y, x, v, what)

    for (y, x, v) in ((0, 0, INF), (0, IW - 1, -INF), (IH - 1, 0, NAN), (IH - 1, IW - 1, INF)):
        put(2, 0, y, x, v, "corners")
    put(2, N - 2, IH - 1, IW - 1, -INF, "frame-seam")
    put(0, N - 1, 0, 0, INF, "frame-seam")
    for k in (1, 16, 32):
        if 2 * NC * k < IW:
            col(2 * NC * k - 1, "lane")
            col(2 * NC * k, "lane")
    first = 2 * (W - NC)                                            # the last lane's first input column
    col(first, "seam")
    col(first - 1, "seam")
    if sl:
        col(2 * (lpr - 1) * NC - 1, "seam")                         # the last column the neighbour holds too
    col(IW - 1, "last-column")
    if nbands > 1:
        for k, y in enumerate(range(2 * band - 2, 2 * band + 2)):
            col((IW // 5) * (k + 1) % IW, "band", y)
    col(IW // 2 + 1, "rows", 1)
    col(IW // 3, "rows", 2 * (IH // 4))
    col((2 * IW) // 3, "rows", IH - 1)
    yq, xq = (2 * IH) // 3, IW // 4 + 1
    put(0, N - 1, yq, xq, INF, "pair")
    put(1, N - 1, yq, xq, -INF, "pair")
    return out


def plant(c, frames, f0, f1, fd, f2):
    """in place; returns the placements"""
    P = placements(c)
    for ch, n, y, x, v, _ in P:
        frames[n, ch, y, x] = v
    # the pair (channels 0 and 1, nine taps each)
    f0[0, 0:18] = np.abs(f0[0, 0:18]) + np.float32(0.01)
    f0[1, 0:9], f0[1, 9:18] = np.abs(f0[1, 0:9]) + np.float32(0.01), -np.abs(f0[1, 9:18]) - np.float32(0.01)
    f0[2, 0:9] = 0.0
    # a lone +Inf in channel 2 is +Inf on every channel of layers 0, 1, 2 under linear activations: the weights take their scale's sign; layer 3's rows alternate
    f0[:, 18:27] = (np.abs(f0[:, 18:27]) + np.float32(0.01)) * np.sign(f0[:, 28])[:, None]
    f1[:, :8] = (np.abs(f1[:, :8]) + np.float32(0.01)) * np.sign(f1[:, 8])[:, None]
    fd[:, :9] = (np.abs(fd[:, :9]) + np.float32(0.01)) * np.sign(fd[:, 12])[:, None]
    f2[:, :8] = (np.abs(f2[:, :8]) + np.float32(0.01)) * np.array([1, -1, 1, -1], np.float32)[:, None]
    return P


def touched(c, P):
    """(4, N, H, W) bool: outputs that a planted pixel reaches -- its 3x3 stride-2 footprint in the 8-channel plane, dilated by the depthwise 3x3"""
    t = np.zeros((4, c.N, c.H, c.W), bool)
    for ch, n, y, x, _, _ in P:
        ys = [oy for oy in range(c.H) if 0 <= y - (2 * oy - 1) < 3]
        xs = [ox for ox in range(c.W) if 0 <= x - (2 * ox - 1) < 3]
        t[:, n, max(ys[0] - 1, 0):ys[-1] + 2, max(xs[0] - 1, 0):xs[-1] + 2] = True
    return t


def classes(v):
    return ({"nan"} if np.isnan(v).any() else set()) | ({"+inf"} if np.isposinf(v).any() else set()) | ({"-inf"} if np.isneginf(v).any() else set())


def _freeze(r):
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def _refs(orc, c, frames, f0, f1, fd, f2, ok=None):
    y64 = frontref.front64(frames, f0, f1, fd, f2, c.acts)
    y32 = frontref.front32(orc, frames, f0, f1, fd, f2, c.acts)
    b = frontref.bound(frames, f0, f1, fd, f2, c.acts)
    ok = np.ones(y64.shape, bool) if ok is None else ok
    d = np.abs(np.where(ok, y32, 0).astype(np.float64) - np.where(ok, y64, 0))
    return dict(frames=frames, f0=f0, f1=f1, fd=fd, f2=f2, y64=y64, y32=y32, bound=b, ok=ok, E_ref=float(d.max()), ymax=float(np.abs(y64[ok]).max()))


@functools.lru_cache(maxsize=None)
def reference(i):
    """inputs and references of CASES[i], computed once and shared (read only): frames, f0, f1, fd, f2, y64, y32 (the oracle), bound, E_ref, ymax"""
    from oracle import orc
    orc.build()
    return _freeze(_refs(orc, CASES[i], *make_inputs(CASES[i])))


@functools.lru_cache(maxsize=None)
def nf_reference(i):
    """the same for NF_CASES[i] with the planted values: also P, touched, lin64 (front64 under linear activations), ok = ~touched, E_ref / ymax over ok"""
    from oracle import orc
    orc.build()
    c = NF_CASES[i]
    frames, f0, f1, fd, f2 = make_inputs(c, nf=True)
    P = plant(c, frames, f0, f1, fd, f2)
    t = touched(c, P)
    r = _refs(orc, c, frames, f0, f1, fd, f2, ~t)
    r.update(P=P, touched=t, lin64=frontref.front64(frames, f0, f1, fd, f2, (0, 0, 0, 0)))
    return _freeze(r)


# ---- part 2: the sources of a mixed batch, as (what, w, h, pitch - 3 w (BGR) or pitch - w (Y plane), bytes the base is off a dword)
def frame_specs(c):
    IW, IH = 2 * c.W, 2 * c.H
    return [("net-size", IW, IH, (-3 * IW) % 4, 0),                # aligned rows: the contiguous-dword branch of the BGR form
            ("off1", IW, IH, 7 - (3 * IW) % 2, 1), ("off2", IW, IH, 5 - (3 * IW) % 2, 2), ("off3", IW, IH, 9 - (3 * IW) % 2, 3),     # odd pitches
            ("up", c.W + 1, c.H, 2, 1), ("down", 5 * c.W + 3, 5 * c.H + 1, 0, 2),
            ("narrow", IW - 5, IH, 3, 0), ("short", IW, IH - 3, 1, 3),        # sw = 2W - 5: zero columns start inside a lane's six; sh = 2H - 3: zero rows inside a band
            ("1-wide", 1, IH + 3, 0, 1), ("1-high", IW + 5, 1, 0, 2)]


# A case that passes everything but the factor 2 of E_k <= factor * E_ref + 1e-6 gets its measured ratio times 1.5, at most 4, here -- with the measured
# value and the date beside it (the rule of tests/irb_blocks/cases.py).  Keyed by the case's id.  (None so far.)
FACTOR = {}
