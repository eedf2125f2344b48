"""Convert surfaces, without a GPU: the four exported symbols, the layout of ffgpu_surface in the ctypes mirror, ffgpu_convert_check on one surface
per format and one case per rejection it can reach, the host glue under ASan + UBSan (san/convert_driver.cc, run as a child process: every rejection
with its message and the job table of an accepted call per source class), four properties of tests/convert/convertref.py, and the device entry points
failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sanrun import check_summary, run_driver
from convert import convertref as R

SYMBOLS = ["ffgpu_convert_check", "ffgpu_convert_tile", "ffgpu_convert_bgr_dev", "ffgpu_convert_nv12_dev"]


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_convert_symbols_and_layout(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s
    S = capi.Surface
    assert C.sizeof(S) == 56 and [getattr(S, f).offset for f in ("p", "pitch", "w", "h", "format", "matrix", "reserved")] == [0, 24, 36, 40, 44, 48, 52]
    assert capi.PIX_NAMES == R.FORMATS and [getattr(capi, "PIX_" + n) for n in R.FORMATS] == list(range(12))
    hdr = open(os.path.join(ROOT, "include", "ffcnn_hip.h")).read()
    for k, n in enumerate(R.FORMATS):
        assert int(re.search(r"#define FFGPU_PIX_%s\s+(\d+)" % n, hdr).group(1)) == k
    assert capi.convert_tile() == (256, 8, 48)


REJECTIONS = [(dict(format=12), "format 12 is none of FFGPU_PIX_* (0..11)"), (dict(matrix=4), "matrix 4 is none of FFGPU_YUV_* (0..3)"),
              (dict(reserved=1), "surface: reserved must be 0"), (dict(w=8193), "a source of 8193 x 12 (1..8192 each)"),
              (dict(h=13), "a source of 21 x 13 for a destination of 21 x 12"), (dict(pitch=(20, 0, 0)), "pitch[0] 20 is below 21"),
              (dict(pitch=(0, 23, 0)), "pitch[1] 23 is odd"), (dict(p=(0x1000, 0x2001, 0)), "plane 1's address 0x2001 is odd"),
              (dict(p=(0x1001, 0, 0)), "plane 1's address"), (dict(p=(0x1000, 0, 0x3000)), "p[2] must be NULL: format 5 has 2 planes")]


def test_convert_check(capi):
    for fmt in range(12):
        for nv12 in (0, 1):
            assert capi.convert_check(capi.surface(fmt, 21, 12, (0x1000,)), nv12, 21, 12)
    for change, msg in REJECTIONS:                                                     # an NV12 surface of 21 x 12 with one field changed
        s = capi.surface(capi.PIX_NV12, 21, 12, change.get("p", (0x1000, 0, 0)), change.get("pitch", (0, 0, 0)))
        for f in ("format", "matrix", "reserved", "w", "h"):
            setattr(s, f, change.get(f, getattr(s, f)))
        with pytest.raises(Exception, match=re.escape("job 0: " + msg)):
            capi.convert_check(s, 1, 21, 12)
    with pytest.raises(Exception, match="NULL src"):
        capi.convert_check(None, 0, 21, 12)


def test_host_glue_under_the_sanitizers():
    out = run_driver("convert", "convert")
    check_summary(out, "convert", 100)
    text = "\n".join(out)
    for msg in ("NULL srcs", "NULL dsts", "0 jobs (1..4096)", "target 3: bad size", "is none of FFGPU_PIX_*", "matrix 4 is none of", "surface: reserved must be 0", "(1..8192 each)",
                "for a destination of 70 x 35", "pitch[0] 69 is below 70", "pitch[1] 71 is odd", "plane 1's address 0x200001 is odd", "p[2] must be NULL",
                "a source plane and a destination plane are the same address", "jobs 0 and 3 have the same destination"):
        assert msg in text, msg


def random_planes(rng, fmt, w, h):
    return [rng.integers(0, 256, (rows, n), dtype=np.uint8) for rows, n, _ in R.planes(fmt, w, h)]


def test_convertref_properties():
    rng = np.random.default_rng(9600)
    w, h = 13, 7
    for m in range(4):                                                                  # grey gives U = V = 128, white gives Y = 235 or 255
        g = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
        for fmt, img in ((0, np.repeat(g, 3, 2)), (3, np.concatenate([np.repeat(g, 3, 2), 255 - g], 2))):
            assert (R.to_nv12(fmt, [img.reshape(h, -1)], w, h, m)[1] == 128).all()
        assert (R.to_nv12(1, [np.full((h, 3 * w), 255, np.uint8)], w, h, m)[0] == (235, 255)[m & 1]).all()
    assert R.to_nv12(0, [np.tile(np.array([255, 0, 0], np.uint8), (h, w))], w, h, 1)[1][0, 0] == 255      # full-range pure blue: 256 before the clamp
    nv, bgr, i420 = random_planes(rng, 5, w, h), random_planes(rng, 0, w, h), random_planes(rng, 7, w, h)
    y, uv = R.to_nv12(5, nv, w, h)
    assert y.tobytes() == nv[0].tobytes() and uv.tobytes() == nv[1].tobytes() and R.to_bgr(0, bgr, w, h).tobytes() == bgr[0].tobytes()
    y, uv = R.to_nv12(7, i420, w, h)
    assert y.tobytes() == i420[0].tobytes() and uv.tobytes() == np.stack([i420[1], i420[2]], -1).tobytes()
    assert R.to_nv12(8, [i420[0], i420[2], i420[1]], w, h)[1].tobytes() == uv.tobytes()                    # YV12: the same planes, V first


def test_convert_without_device(capi):
    """with no HIP device both device entry points say so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    for call in (L.ffgpu_convert_bgr_dev, L.ffgpu_convert_nv12_dev):
        assert call(None, None, 1, None) < 0
        assert ("NULL" if torch.cuda.is_available() else "no HIP device") in capi.last_error()
