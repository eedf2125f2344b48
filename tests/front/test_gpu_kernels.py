"""k_front (ffgpu_front.inc: the net's first four layers as one launch) against a float64 restatement of the four layers (frontref.front64), one test per case of
tests/front/cases.py.  The kernel has no entry point of its own: every case is a four-layer headless net whose filter rows the test writes (irb_stage.nets.put),
run by an FFGPU_KEEP_ALL executor under FFGPU_FRONT_MIN_PX=1, FFGPU_FRONT_NC and FFGPU_FRONT_BAND.  Every test first proves that k_front ran and which form of it:
the probe (ffgpu_front_plan_text) names the instantiation and the launch shape the case is there for, the plan has one launch that carries a layer, layer 0 is "not
materialised", and the u8 / resizing forms capture a graph of their own at their first call.  tests/test_front_ref.py holds table, bound and oracle to their purpose on the CPU.

Part 1 (test_error_bound), the fp32 form, three and four columns per lane.  Two forwards give the same bits, no output is NaN, and both hold:
    per output   |got - front64| <= frontref.bound                                   the hard bound carried through the four stages: no correct fp32 evaluation exceeds it
    per case     E_k <= 2 E_ref + 1e-6  and  E_k <= 8e-7 max |y| + 1e-6               blockref.criterion, E_ref = max |oracle - front64| the yardstick (cases.FACTOR: the
                                                                                     cases that need more than 2, if any, with the measured ratio)
Part 2 (test_forms_agree_in_bits): layer 3 from u8 frames of the net's size (forward_bgr_dev), from a mixed batch of u8 BGR frames (forward_bgr_frames_dev) and of
NV12 frames (forward_nv12_frames_dev under FFGPU_NV12_FRONT=1, matrices 0 and 1), fused and staged (FFGPU_NO_U8_FRONT=1), is bit for bit what the fp32 form gives
for the oracle's net_input of the same frames -- with random weights, at the seams, under a mean and norm that are not the default, one norm negative.  A mixed batch
(cases.frame_specs, ten frames in one call -- the one place a case has more than five frames) holds a frame of the net's size with aligned rows (the contiguous-dword branch), the
same picture off a dword by 1, 2 and 3 bytes with odd pitches, an up-scaled and a down-scaled frame, letterboxes that end inside a lane's six columns and inside a band,
a one-pixel-wide and a one-pixel-high source.  Every source lies inside a larger buffer of random bytes, the pitch padding included.

Part 3 (test_non_finite_inputs): +Inf, -Inf and NaN in the frames where the kernel's addressing can go wrong (cases.placements).  NaN exactly where front64 has NaN,
+-Inf equal, every other output -- the untouched ones, and the touched ones a relu has brought back to numbers or exact zeros (either sign) -- finite and within
the bound; the untouched ones also meet the criterion.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the kernel tests.)"""
import numpy as np
import pytest

from front import cases, frontref
from front.cases import CASES, NF_CASES, FORM_CASES
from irb_blocks import blockref
from irb_stage import nets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    from ffcnn_amd import capi
    capi.lib()
    return capi


def load(F, tmp_path, c, r):
    cfg = str(tmp_path / "front.cfg")
    with open(cfg, "w") as fp:
        fp.write(cases.cfg_text(c))
    net = F.Net(cfg, None)
    nets.put(net, cases.layers(r["f0"], r["f1"], r["fd"], r["f2"]))
    return net, cfg


def front_ran(F, ex, c, form="f32"):
    """the plan is k_front and nothing else that carries a layer; the probe's line is the case's"""
    assert cases.plan_line(F.front_plan_text, c, form) == cases.want_line(c, form)
    model = [lay for lay, _ in ex.step_model()]
    assert [lay for lay in model if lay >= 0] == [0] and ex.kernel_count == len(model), model
    with pytest.raises(RuntimeError, match="not materialised"):
        ex.read_layer(0, 0)


def layer3(ex, N):
    import torch
    torch.cuda.synchronize()
    return np.stack([ex.read_layer(3, n) for n in range(N)], 1)


def assert_error(c, got, r, ok):
    """both conditions of part 1 over the outputs `ok`; the hard bound over every finite output of front64"""
    fin = np.isfinite(r["y64"])
    assert np.isfinite(got[fin]).all(), "%s: %d outputs are not finite" % (c.id, int((~np.isfinite(got[fin])).sum()))
    d = np.abs(np.where(fin, got, 0).astype(np.float64) - np.where(fin, r["y64"], 0))
    share = np.where(fin, d / np.maximum(r["bound"], 1e-300), 0)
    E_k, E_ref, ymax = float(d[ok].max()), r["E_ref"], r["ymax"]
    NC, lpr, sl = cases.geometry(c)[:3]
    print("RATIO %s NC %d lpr %d sl %d E_k %.3g E_ref %.3g ymax %.3g E_k/E_ref %.3f bound used %.4f" % (c.id, NC, lpr, sl, E_k, E_ref, ymax, E_k / max(E_ref, 1e-30), float(share.max())))
    assert (d[fin] <= r["bound"][fin]).all(), "%s: %.3g of the hard bound at (channel, frame, y, x) %r" % (c.id, float(share.max()), np.argwhere(share == share.max())[0].tolist())
    assert blockref.criterion(E_k, E_ref, ymax, cases.FACTOR.get(c.id, 2.0)), (c.id, E_k, E_ref, ymax)


# ---------------------------------------------------------------------------------------------------------------------------- part 1
@pytest.mark.parametrize("i", range(len(CASES)), ids=cases.IDS)
def test_error_bound(F, i, tmp_path, monkeypatch):
    c, r = CASES[i], cases.reference(i)
    cases.set_switches(monkeypatch, c)
    net, _ = load(F, tmp_path, c, r)
    with net, net.executor(c.N, F.FFGPU.KEEP_ALL) as ex:
        front_ran(F, ex, c)
        ex.forward_host(r["frames"])
        got = layer3(ex, c.N)
        ex.forward_host(r["frames"])
        again = layer3(ex, c.N)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "%s: a second forward gives other bits" % c.id
    assert not np.isnan(got).any(), c.id
    assert_error(c, got, r, r["ok"])


# ---------------------------------------------------------------------------------------------------------------------------- part 3
@pytest.mark.parametrize("i", range(len(NF_CASES)), ids=cases.NF_IDS)
def test_non_finite_inputs(F, i, tmp_path, monkeypatch):
    c, r = NF_CASES[i], cases.nf_reference(i)
    lin, t, y64 = r["lin64"], r["touched"], r["y64"]
    assert np.array_equal(~np.isfinite(lin), t) and cases.classes(lin) == {"nan", "+inf", "-inf"}, "test set-up: the touched outputs, and no others, are non-finite in the reference"
    cases.set_switches(monkeypatch, c)
    net, _ = load(F, tmp_path, c, r)
    with net, net.executor(c.N, F.FFGPU.KEEP_ALL) as ex:
        front_ran(F, ex, c)
        ex.forward_host(r["frames"])
        got = layer3(ex, c.N)
    leaked = ~t & ~np.isfinite(got)
    assert not leaked.any(), "%s: a non-finite value leaked into %d untouched outputs, first at (channel, frame, y, x) %r" % (c.id, int(leaked.sum()), np.argwhere(leaked)[:4].tolist())
    nan = np.isnan(y64)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN at %r, expected at %r" % (c.id, np.argwhere(np.isnan(got) & ~nan)[:4].tolist(), np.argwhere(nan & ~np.isnan(got))[:4].tolist())
    inf = np.isinf(y64)
    assert np.array_equal(got[inf], y64[inf].astype(np.float32)), "%s: +-Inf outputs differ at %r" % (c.id, np.argwhere(inf & (got != y64.astype(np.float32)))[:4].tolist())
    assert_error(c, got, r, r["ok"])


# ---------------------------------------------------------------------------------------------------------------------------- part 2
class Sources:
    """device buffers of random bytes with the frames inside: BGR (rows of 3 w bytes at the spec's pitch, the base off a dword by the spec's bytes) or NV12 (a Y
    plane laid out the same way and an interleaved U V plane at an even address with an even pitch); .desc for the frame tables, .bgr the pictures as (h, w, 3) B G R"""

    def __init__(self, torch, rng, specs, nv12=None):
        self.keep, self.desc, self.bgr = [], [], []
        first = None                                                    # the frame of the net's size: "off1" .. "off3" are the same picture
        for k, (what, w, h, extra, off) in enumerate(specs):
            same = first is not None and what.startswith("off")
            if nv12 is None:
                img = first if same else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                first = img if first is None else first
                pitch = 3 * w + extra
                buf = rng.integers(0, 256, 64 + off + pitch * h + 64, dtype=np.uint8)
                buf[64 + off:64 + off + pitch * h].reshape(h, pitch)[:, :3 * w] = img.reshape(h, 3 * w)
                dev = torch.from_numpy(buf).cuda()
                assert dev.data_ptr() % 4 == 0
                self.desc.append((dev.data_ptr() + 64 + off, w, h, pitch))
            else:
                from nv12_frames.test_gpu_fuzz_input import nv12_to_bgr
                cw, ch = 2 * ((w + 1) // 2), (h + 1) // 2
                Y, UV = first if same else (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8))
                first = (Y, UV) if first is None else first
                py, pu = w + extra, cw + 2 * (k % 3)
                uvo = (64 + off + py * h + 5 + 1) & ~1
                buf = rng.integers(0, 256, uvo + pu * ch + 64, dtype=np.uint8)
                buf[64 + off:64 + off + py * h].reshape(h, py)[:, :w] = Y
                buf[uvo:uvo + pu * ch].reshape(ch, pu)[:, :cw] = UV
                dev = torch.from_numpy(buf).cuda()
                assert dev.data_ptr() % 4 == 0
                self.desc.append((dev.data_ptr() + 64 + off, dev.data_ptr() + uvo, w, h, py, pu, nv12))
                img = nv12_to_bgr(Y, UV, w, h, nv12)
            self.keep.append(dev)
            self.bgr.append(img)
        torch.cuda.synchronize()


def net_input(o, imgs, mean, norm):
    """the oracle's net_input of every picture: (N, 3, 2H, 2W) float32"""
    out = []
    for img in imgs:
        h, w = img.shape[:2]
        pk = np.zeros((h, (3 * w + 3) & ~3), np.uint8)
        pk[:, :3 * w] = img.reshape(h, 3 * w)
        o.set_input_image(pk, w, h, mean, norm)
        out.append(np.array(o.input))
    return np.stack(out)


def same_bits(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d outputs differ in their bits, first at (channel, frame, y, x) %r: %r / %r" % (
        what, len(bad), got.size, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("i", range(len(FORM_CASES)), ids=cases.FORM_IDS)
def test_forms_agree_in_bits(F, orc, i, tmp_path, monkeypatch):
    import torch
    c = FORM_CASES[i]
    N, IW, IH = c.N, 2 * c.W, 2 * c.H
    _, f0, f1, fd, f2 = cases.make_inputs(c)
    rng = np.random.default_rng(c.seed)
    cases.set_switches(monkeypatch, c, FFGPU_NV12_FRONT="1")
    net, cfg = load(F, tmp_path, c, dict(f0=f0, f1=f1, fd=fd, f2=f2))
    o = orc.Oracle(cfg=cfg, weights=None)
    mean, norm = cases.MEAN, cases.NORM
    with net, net.executor(N, F.FFGPU.KEEP_ALL) as ex:
        front_ran(F, ex, c)

        def fp32(frames):
            ex.forward_host(frames)
            return layer3(ex, N)

        def both_routes(what, form, call, want):
            """the fused route (a graph of its own at the first call of the form, k_front's instantiation named by the probe), then the staged one"""
            assert cases.plan_line(F.front_plan_text, c, form).startswith("front<4,1,%d,%d,%d> " % (c.nc, form != "u8", form == "nv12_frames"))
            c0 = ex.graph_captures
            call()
            got = layer3(ex, N)
            assert ex.graph_captures == c0 + (0 if what.endswith("again") else 1), "%s: %d graphs captured" % (what, ex.graph_captures - c0)
            with pytest.raises(RuntimeError, match="no fp32 input tensor exists"):
                ex.read_layer(-1, 0)                                    # the kernel read the bytes itself
            same_bits(got, want, "%s %s, fused" % (c.id, what))
            monkeypatch.setenv("FFGPU_NO_U8_FRONT", "1")
            c1 = ex.graph_captures
            call()
            got = layer3(ex, N)
            monkeypatch.delenv("FFGPU_NO_U8_FRONT")
            assert ex.graph_captures == c1 and ex.read_layer(-1, 0).shape == (3, IH, IW)
            same_bits(got, want, "%s %s, staged" % (c.id, what))

        # the u8 form: frames of the net's size, one behind the other at the pitch forward_bgr_dev expects, the base dword aligned
        u8 = rng.integers(0, 256, (N, IH, IW, 3), dtype=np.uint8)
        pitch = (3 * IW + 3) & ~3
        buf = rng.integers(0, 256, 64 + N * IH * pitch + 64, dtype=np.uint8)
        buf[64:64 + N * IH * pitch].reshape(N * IH, pitch)[:, :3 * IW] = u8.reshape(N * IH, 3 * IW)
        dev = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        assert (dev.data_ptr() + 64) % 4 == 0
        want = fp32(net_input(o, list(u8), mean, norm))
        assert np.array_equal(net_input(o, list(u8), mean, norm).view(np.uint32), frontref.u8_input(u8, mean, norm).view(np.uint32))
        both_routes("u8", "u8", lambda: ex.forward_bgr_dev(dev.data_ptr() + 64, IW, IH, mean, norm), want)
        if c.nc == 3:
            specs = cases.frame_specs(c)
            src = Sources(torch, rng, specs)
            frames = net_input(o, src.bgr, mean, norm)
            # set-up: the letterboxes end where the specs say (mean is not 0: a pixel of the picture is never 0.0 in all three planes of a whole column / row)
            kind = [s[0] for s in specs]
            narrow, short = frames[kind.index("narrow")], frames[kind.index("short")]
            assert (narrow[:, :, IW - 5:] == 0).all() and (narrow[:, :, IW - 6] != 0).any() and (short[:, IH - 3:] == 0).all() and (short[:, IH - 4] != 0).any()
            assert (frames[kind.index("1-wide")] == 0).all() and (frames[kind.index("1-high")] == 0).all()
            both_routes("bgr frames", "bgr_frames", lambda: ex.forward_bgr_frames_dev(src.desc, mean, norm), fp32(frames))
            for matrix in (0, 1):
                src = Sources(torch, rng, specs, nv12=matrix)
                want = fp32(net_input(o, src.bgr, mean, norm))
                both_routes("nv12 frames, matrix %d%s" % (matrix, ", again" if matrix else ""), "nv12_frames", lambda: ex.forward_nv12_frames_dev(src.desc, mean, norm), want)
        else:
            assert cases.plan_line(F.front_plan_text, c, "bgr_frames") == cases.plan_line(F.front_plan_text, c, "nv12_frames") == "staged"
    o.close()
