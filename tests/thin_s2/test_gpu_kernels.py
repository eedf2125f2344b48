"""The streaming form of the stride-2 block 4 -> 24 -> 8 (k_irb_thin_s2: a band of output rows per wave, the frames of a group side by side in the wave, three
output columns per lane, packed fp32 on the vector ALU) against the fp32 reference chain under the float64 bound of tests/irb_blocks.

Every case runs one block through the block-level entry as an FFGPU_CONCURRENT executor would launch it, at four band heights (FFGPU_THIN_S2_BAND = 1, 2, 3
and 16: for every plane one that divides the output height, one that does not, and one longer than the plane); the output lies between guard words in one
allocation and starts as NaN.  ffgpu_irb_s2_launch_text says which form each launch took, so a case that was meant for the streaming form cannot pass on the
wave kernel.  Planes: 160 x 6 with two frames and 160 x 7 with three (an odd batch: the last group's second slot has no frame; an odd height: the last
output row reads one row outside), 158 wide (79 output columns: the last lane slides), 156 wide (78: no slide), 16 x 4 (21 slots of three lanes), and
200 wide / one frame, where the rule keeps the wave kernel.  The seams: non-finite values in slot A's last column and slot B's first one.  Then the whole
net with 2 and 33 frames, the knob at 1 and at 0: layer 11 against the oracle -- SAMPLED at 33 frames: six of them (0, 1, 2, 30, 31, 32), an oracle forward
takes 0.4 s; every frame's layer 11 is compared between the two settings under the same criterion --, and the detection records of the two settings against
each other.  (Which form a launch took is read from ffgpu_irb_s2_launch_text, which asks the same thin_s2_form the launch asks, on a descriptor filled the
same way; the launch itself does not report it -- the paired thin form's tests do the same.)

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import functools

import numpy as np
import pytest

from irb_blocks import blockref

pytestmark = pytest.mark.gpu

GUARD_BITS = 0x5A5AA5A5
ACTS = (2, 2, 0, 0)
BANDS = (1, 2, 3, 16)
IC, EC, OC = 4, 24, 8
# (N, W, H, the streaming form takes it)
PLANES = [(2, 160, 6, True), (3, 160, 7, True), (2, 158, 5, True), (2, 156, 4, True), (2, 16, 4, True), (2, 200, 4, False), (1, 160, 6, False)]
# E_k <= FACTOR * E_ref + 1e-6 (blockref.criterion): 2.0, the suite's own factor (measured over every case of this file: E_k / E_ref 0.65 to 1.02).  A larger
# one would have to be measured against the chain and written here with the number.
FACTOR = 2.0


@pytest.fixture(scope="module")
def env():
    import torch
    from ffcnn_amd import capi
    capi.lib()
    return capi, torch


@pytest.fixture()
def clean(monkeypatch):
    from test_irb_choice import knob_names
    for v in knob_names():
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def full_shape(N, W, H, acts=ACTS):
    return (N, W, H, IC, EC, OC, 2) + tuple(acts)


@functools.lru_cache(maxsize=None)
def reference(N, W, H, acts=ACTS, planted=False):
    """inputs (read only), the fp32 chain, float64 and the criterion's terms"""
    from oracle import orc
    orc.build()
    shape = (N, W, H, IC, EC, OC, 2)
    x, f1, fd, f2, _ = blockref.make_inputs(9000 + 13 * W + 5 * N + H, *shape)
    if planted:
        plant(x, N, W, H)
    y32 = blockref.chain32(orc, x, f1, fd, f2, None, *shape, acts)
    y64 = blockref.block64(x, f1, fd, f2, None, *shape, acts)
    ok = np.isfinite(y32) & np.isfinite(y64)
    for a in (x, f1, fd, f2, y32, y64, ok):
        a.setflags(write=False)
    return dict(x=x, f1=f1, fd=fd, f2=f2, y32=y32, y64=y64, ok=ok, E_ref=float(np.abs(y32[ok] - y64[ok]).max()), ymax=float(np.abs(y64[ok]).max()))


def plant(x, N, W, H):
    """a NaN with a payload, +Inf and -Inf at the seam of neighbouring slots -- the last column of an even frame (slot A), the first column of an odd one
    (slot B) -- in the first, a middle and the last row; a batch's odd last frame (what the idle slot of its wave re-reads) gets them in both columns"""
    xf = x.reshape(IC, N, H, W).view(np.uint32)
    vals = [0x7FC12345, 0x7F800000, 0xFF800000]
    rows = [0, H // 2, H - 1]
    for n in range(N):
        cols = [W - 1] if n % 2 == 0 else [0]
        if n % 2 == 0 and n == N - 1:
            cols = [0, W - 1]
        for k, (row, col) in enumerate((r, c) for r in rows for c in cols):
            xf[(n + k) % IC, n, row, col] = vals[(n + k) % 3]


def launch(capi, torch, r, N, W, H, acts=ACTS):
    """one launch as an FFGPU_CONCURRENT executor makes it, into a guarded, NaN-filled output: the output's bits (oc, N, OH, OW)"""
    OH, OW = blockref.out_dims(H, W, 2)
    n_out = OC * N * OH * OW
    guard = (2 * H * W + 63) & ~63
    host = [r["x"], r["f1"], r["fd"], r["f2"]]
    dev = [torch.from_numpy(a.copy()).cuda() for a in host]
    buf = torch.full((guard + n_out + guard,), GUARD_BITS, dtype=torch.int32, device="cuda")
    out = buf[guard:guard + n_out].view(torch.float32)
    out.fill_(float("nan"))
    capi.irb_dev(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), None, out.data_ptr(), N, W, H, IC, EC, OC, 2, *acts, flags=capi.FFGPU.CONCURRENT)
    torch.cuda.synchronize()
    bits = buf.cpu().numpy().view(np.uint32)
    assert (bits[:guard] == GUARD_BITS).all() and (bits[guard + n_out:] == GUARD_BITS).all(), "guard words overwritten"
    for d, h in zip(dev, host):
        assert d.cpu().numpy().tobytes() == h.tobytes(), "an input changed"
    return bits[guard:guard + n_out].reshape(OC, N, OH, OW).copy()


def confirm_form(capi, N, W, H, s2, band, acts=ACTS):
    line = capi.irb_s2_launch_text(full_shape(N, W, H, acts), capi.FFGPU.CONCURRENT)
    if s2:
        assert line.startswith("thin_s2<4,24,8,3> ") and " band=%d " % band in line, line
    else:
        assert line.startswith("irbw<1,1,2,"), line


def same_bits(a, b, what):
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%s: %d of %d outputs differ in their bits, first at (channel, frame, y, x) %r: %#x / %#x" % (
        what, len(bad), a.size, bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def bound(bits, ref, what):
    got = bits.view(np.float32)
    y32, y64, ok = ref["y32"], ref["y64"], ref["ok"]
    assert np.array_equal(np.isnan(got), np.isnan(y32)), "%s: NaN at %r, the chain's at %r" % (what, np.argwhere(np.isnan(got))[:4].tolist(), np.argwhere(np.isnan(y32))[:4].tolist())
    inf = np.isinf(y32)
    assert np.array_equal(got[inf], y32[inf]), "%s: +-Inf outputs differ" % what
    assert np.isfinite(got[ok]).all() and ok.any(), what
    E_k = float(np.abs(got[ok] - y64[ok]).max())
    print("RATIO %s E_k %.3g E_ref %.3g ymax %.3g E_k/E_ref %.3f E_k/ymax %.3g" % (what, E_k, ref["E_ref"], ref["ymax"], E_k / max(ref["E_ref"], 1e-30), E_k / ref["ymax"]))
    assert blockref.criterion(E_k, ref["E_ref"], ref["ymax"], FACTOR), (what, E_k, ref["E_ref"], ref["ymax"])


@pytest.mark.parametrize("plane", PLANES, ids=["%dx%dx%d" % p[:3] for p in PLANES])
def test_against_the_chain(env, clean, plane):
    capi, torch = env
    N, W, H, s2 = plane
    r = reference(N, W, H)
    for band in BANDS:
        what = "%dx%dx%d band %d" % (N, W, H, band)
        clean.setenv("FFGPU_THIN_S2_BAND", str(band))
        confirm_form(capi, N, W, H, s2, band)
        got = launch(capi, torch, r, N, W, H)
        assert not np.isnan(got.view(np.float32)).any(), "%s: unwritten outputs" % what
        bound(got, r, what)


SEAMS = [(2, 160, 6), (3, 160, 7), (2, 158, 5), (2, 16, 4)]


@pytest.mark.parametrize("acts", [(2, 2, 0, 0), (1, 1, 0, 0)], ids=["leaky", "relu"])
@pytest.mark.parametrize("case", SEAMS, ids=["%dx%dx%d" % s for s in SEAMS])
def test_nothing_crosses_the_seam(env, clean, case, acts):
    """NaN (with a payload), +Inf and -Inf in slot A's last column and slot B's first, rows first / middle / last, and in the frame the idle slot of an odd
    batch re-reads: the NaN positions are the chain's, the +-Inf values equal, and every finite output of the OTHER frames has the bits of a run without the
    planted values"""
    capi, torch = env
    N, W, H = case
    r, base = reference(N, W, H, acts, True), reference(N, W, H, acts, False)
    assert not np.isfinite(r["x"]).all() and np.isfinite(base["x"]).all()
    touched = [np.nonzero(~np.isfinite(r["x"].reshape(IC, N, H, W)[:, n]).reshape(-1))[0].size > 0 for n in range(N)]
    assert all(touched)
    for band in (1, 2, 16):
        what = "seam %dx%dx%d acts %r band %d" % (N, W, H, acts, band)
        clean.setenv("FFGPU_THIN_S2_BAND", str(band))
        confirm_form(capi, N, W, H, True, band, acts)
        got = launch(capi, torch, r, N, W, H, acts)
        plain = launch(capi, torch, base, N, W, H, acts)
        bound(got, r, what)
        bound(plain, base, what + " (nothing planted)")
        # a frame's planted values change that frame's outputs alone: wherever the chain's output did not move with them, the kernel's bits did not either
        same = r["y32"].view(np.uint32) == base["y32"].view(np.uint32)
        assert same.mean() > 0.5, what
        same_bits(np.where(same, got, 0), np.where(same, plain, 0), what + ": outputs the planted values do not reach")
        # and in particular the seam columns of the neighbouring frames: frame B's column 0 under frame A's last input column, and the other way round
        OW = got.shape[3]
        for n in range(N):
            for col, nb in ((0, n - 1), (OW - 1, n + 1)):
                if 0 <= nb < N:
                    m = same[:, n, :, col]
                    same_bits(np.where(m, got[:, n, :, col], 0), np.where(m, plain[:, n, :, col], 0), "%s, frame %d column %d" % (what, n, col))


@functools.lru_cache(maxsize=None)
def net_inputs(N):
    """the frames of the whole-net test and the oracle's layer 11 (computed once, read only) -- of every frame of a small batch; of a large one (an oracle
    forward takes 0.4 s) of the first group's two frames, the frame behind them, the last full group and the odd last frame, whose slot neighbour is idle"""
    from oracle import orc
    orc.build()
    bgr, w, h = orc.load_bmp()
    o = orc.Oracle()
    o.set_input_image(bgr, w, h)
    base = np.array(o.input, np.float32)
    rng = np.random.default_rng(N)
    frames = np.stack([np.roll(base, 7 * k, axis=2)[:, :, ::-1 if k % 3 == 1 else 1] + (rng.uniform(-0.02, 0.02, base.shape).astype(np.float32) if k % 2 else 0) for k in range(N)]).astype(np.float32)
    l11 = {}
    for k in (range(N) if N <= 4 else (0, 1, 2, N - 3, N - 2, N - 1)):
        o.input[...] = frames[k]
        o.forward(0)
        l11[k] = np.array(o.layer_out(11), np.float32)
    o.close()
    frames.setflags(write=False)
    return frames, l11


@pytest.mark.parametrize("N", [2, 33])
def test_whole_net(env, clean, N):
    """yolo-fastest through an FFGPU_CONCURRENT | FFGPU_KEEP_ALL executor with the knob at 1 and at 0: layer 11 of both against the oracle (SAMPLED at 33 frames: net_inputs says which six) and of
    every frame against the other setting's under the per-layer criterion of tests/test_gpu_round5.py, and the two settings' detections against each other under the record tolerances (class, order, score within 1e-4,
    corners within 0.05 px + 1e-4 of the box's scale; a box on one side only at a threshold).  The two need not be bit-identical: the accumulation order
    changes from the MFMA's to the reference's."""
    capi, torch = env
    from test_gpu_round5 import close
    from test_gpu_round4 import _yolo_thresholds, boxes_match_up_to_threshold_flips
    frames, l11 = net_inputs(N)
    shape = (N, 160, 160, IC, EC, OC, 2) + ACTS
    got = {}
    with capi.Net() as net:
        thresholds = _yolo_thresholds(net)
        for knob in ("1", "0"):
            clean.setenv("FFGPU_THIN_S2", knob)
            line = capi.irb_s2_launch_text(shape, capi.FFGPU.CONCURRENT)
            assert line.startswith("thin_s2<4,24,8,3> " if knob == "1" else "irbw<1,1,2,3"), line
            with net.executor(N, capi.FFGPU.CONCURRENT | capi.FFGPU.KEEP_ALL) as ex:   # (KEEP_ALL: read_layer; the blocks stay fused)
                ex.set_scale(1, 1)
                ex.forward_host(frames)
                mine = [ex.read_layer(11, k) for k in range(N)]
                for k, ref in l11.items():
                    close(mine[k], ref, "knob %s frame %d layer 11 vs oracle" % (knob, k))
                got[knob] = ([ex.read_boxes(k) for k in range(N)], mine)
    assert sum(len(b) for b in got["1"][0]) > 0, "no detections at all"
    for k in range(N):
        close(got["1"][1][k], got["0"][1][k], "frame %d layer 11, knob 1 against knob 0" % k)       # every frame, the sampled ones included
        boxes_match_up_to_threshold_flips(got["1"][0][k], got["0"][0][k], thresholds, "frame %d of %d, knob 1 against knob 0" % (k, N))
