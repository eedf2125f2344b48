"""Convert surfaces on the device: ffgpu_convert_bgr_dev / _nv12_dev against tests/convert/convertref.py, the numpy restatement of the contract in
include/ffcnn_hip.h.  Sources, destinations with their row padding and 64 guard bytes round each plane lie in one arena of seeded random bytes; the
WHOLE arena is compared byte for byte, so every byte the contract leaves alone must have stayed.  Then NV12 frames converted and sent through the
BGR forward of the real net against the NV12 forward of the same frames.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other post-pass fuzz tests.)"""
import numpy as np
import pytest

from convert import convertref as R
from test_gpu_round2 import F, net  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
GUARD = 64


class Arena:
    """planes laid out behind each other at 256-byte bases; general: every plane a byte (its alignment) off the base, pitches the least + that;
    aligned: pitches the next multiple of 4 and a padding dword"""
    def __init__(self):
        self.size, self.jobs = 256, []

    def plane(self, rows, least, align, general):
        off, pitch = self.size + (align if general else 0), least + align if general else ((least + 3) & ~3) + 4
        self.size = (off + rows * pitch + GUARD + 255) & ~255
        return off, rows, pitch, least

    def job(self, fmt, nv12, w, h, general, matrix):
        src = [self.plane(rows, least, align, general) for rows, least, align in R.planes(fmt, w, h)]
        dst = [self.plane(rows, least, align, general) for rows, least, align in (R.planes(5, w, h) if nv12 else R.planes(0, w, h))]
        self.jobs.append((fmt, w, h, matrix, src, dst))
        return len(self.jobs) - 1


def view(a, p, logical=True):
    off, rows, pitch, least = p
    return a[off:off + rows * pitch].reshape(rows, pitch)[:, :least if logical else pitch]


def run(F, arena, nv12, start, skip=()):
    """the arena's jobs in ONE call on the device, and what convertref makes of them: (got, want)"""
    import torch
    want = start.copy()
    dev = torch.from_numpy(start).cuda()
    base, srcs, dsts = dev.data_ptr(), [], []
    assert base % 256 == 0
    for k, (fmt, w, h, matrix, src, dst) in enumerate(arena.jobs):
        srcs.append(None if k in skip else F.surface(fmt, w, h, [base + p[0] for p in src], [p[2] for p in src], matrix))
        dsts.append((base + dst[0][0], base + dst[1][0], w, h, dst[0][2], dst[1][2]) if nv12 else (base + dst[0][0], w, h, dst[0][2]))
        if k in skip:
            continue
        planes = [view(start, p, False) for p in src]
        out = R.to_nv12(fmt, planes, w, h, matrix) if nv12 else [R.to_bgr(fmt, planes, w, h, matrix).reshape(h, 3 * w)]
        for p, o in zip(dst, out):
            view(want, p)[...] = o
    (F.convert_nv12_dev if nv12 else F.convert_bgr_dev)(srcs, dsts)
    torch.cuda.synchronize()
    return dev.cpu().numpy(), want


def random_arena(arena, seed):
    """seeded random bytes everywhere (P010 samples with random low six bits among them): sources, the destinations' pattern, padding and guards"""
    return np.random.default_rng(seed).integers(0, 256, arena.size, dtype=np.uint8)


def differ(what, got, want):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d bytes differ, first at %d: got %d, want %d" % (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


# 1 x 1, 2 x 2, 3 x 5, 7 x 2: odd edges, a single block, a lone last row or column; a tile seam in both directions with a ragged end; two seams in a row pair
SHAPES = ((1, 1), (2, 2), (3, 5), (7, 2), (256 + 5, 8 + 3), (2 * 256 + 2, 2))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("nv12", (0, 1), ids=("bgr", "nv12"))
@pytest.mark.parametrize("fmt", range(12), ids=R.FORMATS)
def test_convert_equals_convertref(F, fmt, nv12, shape):
    """job 0 in the aligned form, job 1 the same pixels in the general form: both equal convertref, hence each other"""
    tw, th, _ = F.convert_tile()
    assert SHAPES[4:] == ((tw + 5, th + 3), (2 * tw + 2, 2))
    w, h = SHAPES[shape]
    arena, matrix = Arena(), (fmt + shape) & 3
    a, g = arena.job(fmt, nv12, w, h, False, matrix), arena.job(fmt, nv12, w, h, True, matrix)
    start = random_arena(arena, 9700 + 100 * fmt + 10 * nv12 + shape)
    for pa, pg in zip(arena.jobs[a][4], arena.jobs[g][4]):
        view(start, pg)[...] = view(start, pa)
    got, want = run(F, arena, nv12, start)
    differ("%s to %s, %d x %d" % (R.FORMATS[fmt], "nv12" if nv12 else "bgr", w, h), got, want)
    for pa, pg in zip(arena.jobs[a][5], arena.jobs[g][5]):
        assert view(got, pa).tobytes() == view(got, pg).tobytes() != view(start, pa).tobytes()


@pytest.mark.parametrize("nv12", (0, 1), ids=("bgr", "nv12"))
def test_convert_many_jobs(F, nv12):
    """one call: every format at a size of its own in both forms, one job skipped by a NULL address, and one NV12 job more than a launch takes"""
    njobs = F.convert_tile()[2]
    arena = Arena()
    for k in range(24):
        arena.job(k % 12, nv12, 5 + 23 * k, 1 + (7 * k) % 19, k >= 12, k & 3)
    for k in range(njobs + 1):
        arena.job(5, nv12, 3 + k % 9, 2 + k % 5, k & 1, k & 3)
    start = random_arena(arena, 9790 + nv12)
    got, want = run(F, arena, nv12, start, skip=(7,))
    differ("many jobs", got, want)
    assert (want != start).sum() > 10000


def test_convert_then_forward_equals_the_nv12_forward(F, net):
    """random NV12 frames, a matrix each: ffgpu_convert_bgr_dev + the BGR forward leaves the records of the NV12 forward on the frames themselves"""
    import torch
    sizes, arena = ((640, 424), (333, 201), (97, 480), (512, 288)), Arena()
    for k, (w, h) in enumerate(sizes):
        arena.job(5, 0, w, h, k & 1, k)
    dev = torch.from_numpy(random_arena(arena, 9799)).cuda()
    base = dev.data_ptr()
    nv, bgr = [], []
    for fmt, w, h, matrix, src, dst in arena.jobs:
        nv.append((base + src[0][0], base + src[1][0], w, h, src[0][2], src[1][2], matrix))
        bgr.append((base + dst[0][0], w, h, dst[0][2]))
    with net.executor(4) as ex:
        ex.forward_nv12_frames_dev(nv)
        want = ex.read_dets().tobytes()
        F.convert_bgr_dev([F.surface(5, f[2], f[3], f[:2], f[4:6], f[6]) for f in nv], bgr)
        ex.forward_bgr_frames_dev(bgr)
        assert ex.read_dets().tobytes() == want
