"""The paired form of the thin fused block (k_irb_thin_pair: two frames side by side in a wave, 3 / 4 / 5 columns per lane) against the single form
(k_irb_thin, FFGPU_THIN_PAIR=0) bit for bit -- NaN payloads included -- and against the fp32 reference chain under the float64 bound of tests/irb_blocks.

Every case runs one block through the block-level entry as an FFGPU_CONCURRENT executor would launch it, at four band heights (FFGPU_THIN_BAND = 1, 2, 3 and
16: for every plane one that divides the height, one that does not, and one longer than the plane), with and without a residual; the output lies between
guard words in one allocation and starts as NaN.  ffgpu_irb_thin_launch_text says which form each launch took, so a case that was meant for the paired form
cannot pass on the single one.  Planes: 160 x 5 (five columns, both halves full), 140 x 7 with three frames (five columns, an odd batch: the last pair's upper
half has no frame), 20 x 7 with three frames and 128 x 3 (four columns), 12 x 4 (three columns), 164 wide (no column count: single form) and one frame (single
form).  The seams: non-finite values in frame A's last column and frame B's first one, and in the frame an idle upper half re-reads.  Then the whole net with
2 and 33 frames, the knob at 1 and at 0: detection records and layer 8.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import functools

import numpy as np
import pytest

from irb_blocks import blockref, cases

pytestmark = pytest.mark.gpu

GUARD_BITS = 0x5A5AA5A5
ACTS = (2, 2, 0, 0)
BANDS = (1, 2, 3, 16)
# (N, W, H, columns per lane of the paired form or 0 for the single one)
PLANES = [(2, 160, 5, 5), (3, 140, 7, 5), (3, 20, 7, 4), (2, 128, 3, 4), (2, 12, 4, 3), (2, 164, 5, 0), (1, 160, 5, 0)]
CHANNELS = [(4, 4), (8, 8), (8, 4), (4, 8)]
CASES = [(p, c) for p in PLANES for c in CHANNELS]


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


def built(ic, ncp):
    return ncp and not (ic == 8 and ncp == 5)                  # five columns of 8 input channels spill: not built, the single form stays


@functools.lru_cache(maxsize=None)
def reference(N, W, H, ic, oc, acts=ACTS, planted=False):
    """inputs (read only) and, per residual choice, the fp32 chain, float64 and the criterion's terms"""
    from oracle import orc
    orc.build()
    shape = (N, W, H, ic, 8, oc, 1)
    x, f1, fd, f2, res = blockref.make_inputs(7000 + 13 * W + 5 * N + ic + 2 * oc, *shape)
    if planted:
        plant(x, N, W, H, ic)
    out = {}
    for with_res in (False, True):
        r = res if with_res else None
        y32 = blockref.chain32(orc, x, f1, fd, f2, r, *shape, acts)
        y64 = blockref.block64(x, f1, fd, f2, r, *shape, acts)
        ok = np.isfinite(y32) & np.isfinite(y64)
        out[with_res] = dict(y32=y32, y64=y64, ok=ok, E_ref=float(np.abs(y32[ok] - y64[ok]).max()), ymax=float(np.abs(y64[ok]).max()))
    for a in (x, f1, fd, f2, res):
        a.setflags(write=False)
    return dict(x=x, f1=f1, fd=fd, f2=f2, res=res, refs=out)


def plant(x, N, W, H, ic):
    """a NaN with a payload, +Inf and -Inf at the seam of every pair -- the last column of its first frame, the first column of its second -- in the first,
    a middle and the last row; a batch's odd last frame (what the idle upper half of its wave re-reads) gets them in both columns"""
    xf = x.reshape(ic, N, H, W).view(np.uint32)
    vals = [0x7FC12345, 0x7F800000, 0xFF800000]
    rows = [0, H // 2, H - 1]
    for n in range(N):
        cols = [W - 1] if n % 2 == 0 else [0]
        if n % 2 == 0 and n == N - 1:
            cols = [0, W - 1]
        for k, (row, col) in enumerate((r, c) for r in rows for c in cols):
            xf[(n + k) % ic, n, row, col] = vals[(n + k) % 3]


def launch(capi, torch, r, with_res, N, W, H, ic, oc, acts=ACTS):
    """one launch as an FFGPU_CONCURRENT executor makes it, into a guarded, NaN-filled output: the output's bits (oc, N, H, W)"""
    n_out = oc * N * H * W
    guard = (2 * H * W + 63) & ~63
    host = [r["x"], r["f1"], r["fd"], r["f2"]] + ([r["res"]] if with_res else [])
    dev = [torch.from_numpy(a.copy()).cuda() for a in host]
    buf = torch.full((guard + n_out + guard,), GUARD_BITS, dtype=torch.int32, device="cuda")
    out = buf[guard:guard + n_out].view(torch.float32)
    out.fill_(float("nan"))
    capi.irb_dev(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr() if with_res else None, out.data_ptr(),
                 N, W, H, ic, 8, oc, 1, *acts, flags=capi.FFGPU.CONCURRENT)
    torch.cuda.synchronize()
    bits = buf.cpu().numpy().view(np.uint32)
    assert (bits[:guard] == GUARD_BITS).all() and (bits[guard + n_out:] == GUARD_BITS).all(), "guard words overwritten"
    for d, h in zip(dev, host):
        assert d.cpu().numpy().tobytes() == h.tobytes(), "an input changed"
    return bits[guard:guard + n_out].reshape(oc, N, H, W).copy()


def both_forms(capi, torch, clean, r, with_res, band, N, W, H, ic, oc, ncp, acts=ACTS):
    """(paired, single) bits at FFGPU_THIN_BAND = band; the text function confirms the form of each launch"""
    shape = (N, W, H, ic, 8, oc, 1) + tuple(acts)
    clean.setenv("FFGPU_THIN_BAND", str(band))
    clean.delenv("FFGPU_THIN_PAIR", raising=False)
    line = capi.irb_thin_launch_text(shape, capi.FFGPU.CONCURRENT)
    if built(ic, ncp):
        assert line.startswith("thin_pair<%d,8,%d,%d> " % (ic, oc, ncp)) and " band=%d " % band in line, line
    else:
        assert line.startswith("thin<%d,8,%d> " % (ic, oc)), line
    pair = launch(capi, torch, r, with_res, N, W, H, ic, oc, acts)
    clean.setenv("FFGPU_THIN_PAIR", "0")
    assert capi.irb_thin_launch_text(shape, capi.FFGPU.CONCURRENT).startswith("thin<%d,8,%d> " % (ic, oc))
    single = launch(capi, torch, r, with_res, N, W, H, ic, oc, acts)
    return pair, single


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
    assert blockref.criterion(E_k, ref["E_ref"], ref["ymax"], cases.FACTOR.get("thin<8,8,4>", 2.0)), (what, E_k, ref["E_ref"], ref["ymax"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx%dx%d-%d-%d" % (p[:3] + c) for p, c in CASES])
def test_pair_equals_single(env, clean, i):
    capi, torch = env
    (N, W, H, ncp), (ic, oc) = CASES[i]
    r = reference(N, W, H, ic, oc)
    for with_res in (False, True):
        for band in BANDS:
            what = "%dx%dx%d %d->8->%d band %d%s" % (N, W, H, ic, oc, band, " +res" if with_res else "")
            pair, single = both_forms(capi, torch, clean, r, with_res, band, N, W, H, ic, oc, ncp)
            same_bits(pair, single, what)
            assert not np.isnan(pair.view(np.float32)).any(), "%s: unwritten outputs" % what
            bound(pair, r["refs"][with_res], what)


SEAMS = [(2, 160, 5, 5, 4, 4), (3, 140, 7, 5, 4, 8), (3, 20, 7, 4, 8, 8), (2, 12, 4, 3, 8, 4), (2, 128, 3, 4, 4, 4)]


@pytest.mark.parametrize("acts", [(2, 2, 0, 0), (1, 1, 0, 1)], ids=["leaky", "relu"])
@pytest.mark.parametrize("case", SEAMS, ids=["%dx%dx%d" % s[:3] for s in SEAMS])
def test_nothing_crosses_the_seam(env, clean, case, acts):
    """NaN (with a payload), +Inf and -Inf in frame A's last column and frame B's first, rows first / middle / last of a band, and in the frame the idle upper
    half of an odd batch re-reads: the paired form's bits are the single form's -- frame B's column 0 and frame A's column W - 1 first of all -- and the
    chain's NaN and Inf pattern"""
    capi, torch = env
    N, W, H, ncp, ic, oc = case
    r = reference(N, W, H, ic, oc, acts, True)
    assert not np.isfinite(r["x"]).all()
    for with_res in (False, True):
        for band in (H, 2, 16):                                  # the planted rows are a band's first, middle and last; then bands that cut between them
            what = "seam %dx%dx%d acts %r band %d%s" % (N, W, H, acts, band, " +res" if with_res else "")
            pair, single = both_forms(capi, torch, clean, r, with_res, band, N, W, H, ic, oc, ncp, acts)
            for n in range(N):
                same_bits(pair[:, n, :, [0, W - 1]], single[:, n, :, [0, W - 1]], "%s, frame %d, columns 0 and W - 1" % (what, n))
            same_bits(pair, single, what)
            bound(pair, r["refs"][with_res], what)


@pytest.mark.parametrize("N", [2, 33])
def test_whole_net(env, clean, N):
    """yolo-fastest through an FFGPU_CONCURRENT | FFGPU_KEEP_ALL executor with the knob at 1 and at 0: the same detection records and the same layer 8, bit for bit"""
    capi, torch = env
    from oracle import orc
    bgr, w, h = orc.load_bmp()
    o = orc.Oracle()
    o.set_input_image(bgr, w, h)
    base = np.array(o.input, np.float32)
    o.close()
    rng = np.random.default_rng(N)
    frames = np.stack([np.roll(base, 7 * k, axis=2)[:, :, ::-1 if k % 3 == 1 else 1] + (rng.uniform(-0.02, 0.02, base.shape).astype(np.float32) if k % 2 else 0) for k in range(N)]).astype(np.float32)
    assert capi.irb_thin_launch_text((N, 160, 160, 4, 8, 4, 1, 2, 2, 0, 0), capi.FFGPU.CONCURRENT).startswith("thin_pair<4,8,4,5> ")
    got = {}
    with capi.Net() as net:
        for knob in ("1", "0"):
            clean.setenv("FFGPU_THIN_PAIR", knob)
            with net.executor(N, capi.FFGPU.CONCURRENT | capi.FFGPU.KEEP_ALL) as ex:   # (KEEP_ALL: read_layer; the blocks stay fused)
                ex.forward_host(frames)
                dets = ex.read_dets()
                got[knob] = (dets.tobytes(), int(dets["count"].sum()), np.stack([ex.read_layer(8, k) for k in range(N)]).view(np.uint32))
    assert got["1"][1] > 0, "no detections at all"
    assert got["1"][0] == got["0"][0], "detection records differ"
    same_bits(got["1"][2].transpose(1, 0, 2, 3), got["0"][2].transpose(1, 0, 2, 3), "layer 8, %d frames" % N)
