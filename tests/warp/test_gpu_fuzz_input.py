"""Warp surfaces on the device: ffgpu_warp_bgr_dev / _nv12_dev on synthetic frames, and in front of a forward on the real net, against
tests/warp/warpref.py, the numpy restatement of the contract in include/ffcnn_hip.h.  Sources, destinations, meshes and 64 guard bytes around each
lie in one arena of seeded random bytes; the WHOLE arena is compared byte for byte, so every byte the contract leaves alone -- the sources, the
meshes, row padding, the rest of a surface round a pane, the guards -- must have stayed; the call is then repeated from the same bytes and must give
the same.  The seeded cases are built on the CPU once (tests/warp/fuzzcases.py) and shared by the tests; tests/test_warp_abi.py holds the conditions
that keep them from passing vacuously.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import os
import re

import numpy as np
import pytest

from warp import fuzzcases, warpref
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
GUARD = fuzzcases.GUARD


def differ(what, got, want, regions=()):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return
    for name, lo, nb in regions:
        hit = bad[(bad >= lo - GUARD) & (bad < lo + nb + GUARD)]
        if len(hit):
            pytest.fail("%s: %s: %d bytes differ, first at region offset %d (region of %d bytes): got %d, want %d"
                        % (what, name, len(hit), int(hit[0]) - lo, nb, got[hit[0]], want[hit[0]]), pytrace=False)
    pytest.fail("%s: %d bytes differ, first at %d: got %d, want %d" % (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]]), pytrace=False)


def descs(c, which, base, a=0, b=None):
    """the case's sources or destinations a .. b - 1 as the wrappers take them"""
    out = []
    for d in which[a:b]:
        if d is None:
            out.append(None)
        elif c.fmt == "bgr":
            out.append((base + d[0], d[1], d[2], d[3]))
        else:
            out.append((base + d[0], base + d[1], d[2], d[3], d[4], d[5]))
    return out


def c_spec(F, c):
    return F.warp_spec(c.filt, c.border, c.fill)


def c_meshes(F, c, base, a=0, b=None):
    """the meshes a .. b - 1 where they lie in the arena on the device"""
    out = []
    for k in range(a, c.n if b is None else b):
        if c.dsts[k] is None:
            out.append(None)
            continue
        w, h = c.size(c.dsts[k])
        out.append(F.warp_mesh(base + c.mesh_off[k], w, h, c.meshes[k][1]))
    return out


def run(F, c, splits=None):
    """the case on the device, as one call or split into several at the given job numbers; returns the arena's bytes afterwards"""
    import torch
    dev = torch.from_numpy(c.start.copy()).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    fn = F.warp_bgr_dev if c.fmt == "bgr" else F.warp_nv12_dev
    cuts = [0] + list(splits or []) + [c.n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a != b:
            fn(descs(c, c.srcs, base, a, b), descs(c, c.dsts, base, a, b), c_meshes(F, c, base, a, b), c_spec(F, c))
    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("fmt,name", fuzzcases.PARAMS)
def test_warp(F, fmt, name):
    """one call: the whole arena against warpref; the same call again from the same bytes: the same bytes"""
    c = fuzzcases.get(fmt, name)
    got = run(F, c)
    differ(c.what, got, c.want, c.regions())
    assert run(F, c).tobytes() == got.tobytes(), "two runs differ"


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_split_calls_leave_the_same_bytes(F, fmt):
    """130 jobs in one call and in calls of 1, 65, 3 and 61 jobs"""
    c = fuzzcases.cases(fmt)["launch table"]
    assert c.n == 130
    differ("%s split" % c.what, run(F, c, [1, 66, 69]), c.want, c.regions())


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_rejections(F, fmt):
    """one call per reason, the message matched, with the job's index where there is one; nothing is launched: the arena stays; a working call
    afterwards"""
    import torch
    c = fuzzcases.cases(fmt)["cells"]
    dev = torch.from_numpy(c.start.copy()).cuda()
    base, L = dev.data_ptr(), F.lib()
    nv12 = fmt == "nv12"
    fn = L.ffgpu_warp_nv12_dev if nv12 else L.ffgpu_warp_bgr_dev
    table = F.nv12_frame_table if nv12 else F.bgr_frame_table
    n = c.n
    gs, gd = descs(c, c.srcs, base), descs(c, c.dsts, base)

    def tab(which, k=None, **kw):
        t = table(which)
        for name_, v in kw.items():
            setattr(t[k], name_, v)
        return t

    def meshes(k=None, **kw):
        arr = (F.WarpMesh * n)(*c_meshes(F, c, base))
        for name_, v in kw.items():
            setattr(arr[k], name_, v)
        return arr

    def sp(**kw):
        s = c_spec(F, c)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(srcs=tab(gs), dsts=tab(gd), ms=meshes(), n_=n, spec=sp()):
        return fn(srcs, dsts, ms, n_, spec, None)
    fill3 = sp()
    fill3.fill[3] = 1
    addr = "y" if nv12 else "bgr"
    m1 = base + c.mesh_off[1]
    cases = [(dict(srcs=None), "NULL srcs"), (dict(dsts=None), "NULL dsts"), (dict(ms=None), "NULL meshes"), (dict(spec=None), "NULL spec"),
             (dict(n_=0), "0 jobs (1..4096)"), (dict(n_=4097), "4097 jobs (1..4096)"), (dict(spec=sp(filter=2)), "filter 2 is neither FFGPU_WARP_BILINEAR nor FFGPU_WARP_NEAREST"),
             (dict(spec=sp(border=2)), "border 2 is neither FFGPU_WARP_FILL nor FFGPU_WARP_CLAMP"), (dict(spec=fill3), "fill[3] must be 0"), (dict(spec=sp(reserved=1)), "spec: reserved must be 0"),
             (dict(srcs=tab(gs, 1, w=0)), "source 1: bad size 0 x 44"), (dict(dsts=tab(gd, 3, h=0)), "destination 3: bad size 70 x 0"),
             (dict(srcs=tab(gs, 0, reserved=1)), "source 0: reserved must be 0"), (dict(dsts=tab(gd, 2, reserved=1)), "destination 2: reserved must be 0"),
             (dict(srcs=tab(gs, 2, h=8193)), "job 2: a source of 50 x 8193 (1..8192 each)"),
             (dict(dsts=tab(gd, 1, h=8200), ms=meshes(1, mh=514)), "job 1: a destination of 70 x 8200 (1..8192 each)"),
             (dict(ms=meshes(1, xy=None)), "job 1: mesh: NULL xy"), (dict(ms=meshes(1, xy=m1 + 4)), "job 1: mesh: xy 0x%x is not 8-byte aligned" % (m1 + 4)),
             (dict(ms=meshes(0, mw=9)), "job 0: mesh: 9 x 6 points, a destination of 70 x 40 with cells of 8 has 10 x 6"),
             (dict(ms=meshes(3, mh=4)), "job 3: mesh: 3 x 4 points, a destination of 70 x 40 with cells of 64 has 3 x 2"),
             (dict(ms=meshes(2, cell=33)), "job 2: mesh: cell 33 is none of 8, 16, 32, 64"), (dict(ms=meshes(2, cell=16)), "job 2: mesh: 4 x 3 points, a destination of 70 x 40 with cells of 16 has 6 x 4"),
             (dict(ms=meshes(0, reserved=7)), "job 0: mesh: reserved must be 0"),
             (dict(srcs=tab(gs, 3, **{addr: gd[3][0]})), "job 3: the source and the destination are the same pixels"),
             (dict(dsts=tab(gd, 2, **{addr: gd[0][0]})), "jobs 0 and 2 have the same destination")]
    if nv12:
        cases += [(dict(srcs=tab(gs, 0, pitch_y=10)), "source 0: pitch_y 10 is below w = 50"), (dict(dsts=tab(gd, 1, matrix=4)), "destination 1: matrix 4"),
                  (dict(srcs=tab(gs, 3, uv=gs[3][1] + 1)), "is odd (U V pairs are read"), (dict(dsts=tab(gd, 0, uv=gd[0][1] + 1)), "is odd (U V pairs are written")]
    else:
        cases += [(dict(srcs=tab(gs, 0, pitch=50)), "source 0: pitch 50 is below 3 w = 150"), (dict(dsts=tab(gd, 0, pitch=100)), "destination 0: pitch 100 is below 3 w = 210")]
    for kw, msg in cases:
        assert call(**kw) < 0, kw
        assert re.search(re.escape(msg), F.last_error()), (msg, F.last_error())
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == c.start.tobytes()                            # nothing was launched
    differ("after the rejections", run(F, c), c.want, c.regions())


# ---------------------------------------------------------------------------------------------------------------- in front of the real net
@pytest.fixture(scope="module")
def picture(F):
    rows, w, h = F.load_bmp(os.path.join(F.DATA, "test.bmp"))
    assert (w, h) == (640, 424)
    return np.ascontiguousarray(rows[:, :3 * w].reshape(h, w, 3))


@pytest.mark.parametrize("fmt", fuzzcases.FORMATS)
def test_identity_warp_then_forward(F, net, picture, fmt):
    """data/test.bmp and its mirror image through the identity warp into frames of their own, then the forward on the real net: the records are byte
    for byte those of the forward on the sources, and the warped frames are byte copies"""
    import torch
    from nv12_frames.test_gpu_fuzz_input import bgr_to_nv12
    rng = np.random.default_rng(9600)
    h, w = picture.shape[:2]
    pics = [picture, np.ascontiguousarray(picture[:, ::-1])]
    ar = fuzzcases.Arena()
    frames = []
    for kind in ("source", "warped"):
        for k in range(2):
            pad = (4, 7)[k] if kind == "source" else (0, 5)[k]
            pitches, sizes = fuzzcases.frame_bytes(fmt, w, h, pad)
            if fmt == "bgr":
                frames.append((ar.alloc("%s %d" % (kind, k), sizes[0], 4, k == 1), w, h, pitches[0]))
            else:
                frames.append((ar.alloc("%s %d y" % (kind, k), sizes[0], 4, k == 1), ar.alloc("%s %d uv" % (kind, k), sizes[1], 2), w, h, pitches[0], pitches[1]))
    xy = warpref.mesh_orient(w, h, 0, 32)[1]
    o_mesh = ar.alloc("mesh", xy.nbytes, 8)
    arena = ar.fill(rng)
    arena[o_mesh:o_mesh + xy.nbytes] = xy.view(np.uint8).reshape(-1)
    for k, pic in enumerate(pics):
        f = frames[k]
        if fmt == "bgr":
            warpref.view(arena, f[0], h, 3 * w, f[3])[...] = pic.reshape(h, 3 * w)
        else:
            Y, UV = bgr_to_nv12(pic)
            warpref.view(arena, f[0], h, w, f[4])[...] = Y
            warpref.view(arena, f[1], (h + 1) // 2, 2 * ((w + 1) // 2), f[5])[...] = UV
    dev = torch.from_numpy(arena.copy()).cuda()
    base = dev.data_ptr()

    def at(d):
        return (base + d[0],) + tuple(d[1:]) if fmt == "bgr" else (base + d[0], base + d[1]) + tuple(d[2:])
    srcs, dsts = [at(f) for f in frames[:2]], [at(f) for f in frames[2:]]
    mesh = F.warp_mesh(base + o_mesh, w, h, 32)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()                                                           # warp and forward on ONE stream: stream order is the only barrier
    with net.executor(2) as ex:
        fwd = ex.forward_bgr_frames_dev if fmt == "bgr" else ex.forward_nv12_frames_dev
        fwd(srcs, stream=st.cuda_stream)
        plain = ex.read_dets().tobytes()
        boxes = ex.read_boxes(0)
        (F.warp_bgr_dev if fmt == "bgr" else F.warp_nv12_dev)(srcs, dsts, [mesh, mesh], F.warp_spec(), stream=st.cuda_stream)
        fwd(dsts, stream=st.cuda_stream)
        warped = ex.read_dets().tobytes()
    st.synchronize()
    want = warpref.warp(arena.copy(), fmt, frames[:2], frames[2:], [(xy, 32)] * 2)
    assert (want != arena).sum() > w * h
    differ("%s identity warp" % fmt, dev.cpu().numpy(), want, ar.regs)
    assert len(boxes) > 0 and warped == plain
