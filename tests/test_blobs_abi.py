"""Motion blobs, without a GPU: the two exported symbols, the layout of the spec struct in the ctypes mirror, the constants, ffgpu_blobs_spec_check
on one bad value per field and on the cell cap, the device entry point failing the way every entry point of the library does when no HIP device is
visible, and tests/blobs/blobref.py itself on three grids written out by hand."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from blobs import blobref


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_blobs_symbols_layout_spec_check_and_no_device(capi):
    for s in ("ffgpu_blobs_spec_check", "ffgpu_blobs_dev"):
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s
    fields = ("w", "h", "cell_log2", "min_pixels", "warmup", "connect", "min_cells", "max_cells", "max_boxes", "pad", "type", "flags", "reserved")
    assert C.sizeof(capi.BlobsSpec) == 64 and [getattr(capi.BlobsSpec, f).offset for f in fields] == list(range(0, 52, 4))
    assert (capi.BLOBS_WORDS, capi.BLOBS_MAX_CELLS, capi.BLOBS_COMPONENTS) == (blobref.WORDS, blobref.MAX_CELLS, blobref.COMPONENTS) == (8, 32768, 2048)
    capi.blobs_spec_check(capi.blobs_spec(2048, 1024, 3, 64, 65535, 4, 32768, 32768, 128, 256, -7))          # 256 x 128 cells: the cap itself
    capi.blobs_spec_check(capi.blobs_spec(3840, 2160, 4, 1))
    for field, value, msg in (("w", 0, "a model of 0 x 33 pixels (1..8192 each)"), ("h", 8193, "a model of 65 x 8193 pixels"), ("cell_log2", 7, "cell_log2 7 is outside 2..6"),
                              ("min_pixels", 65, "min_pixels 65 is outside 1..64"), ("warmup", 65536, "warmup 65536 is outside 0..65535"), ("connect", 6, "connect 6 is neither 4 nor 8"),
                              ("min_cells", 0, "min_cells 0 is outside 1..32768"), ("max_cells", 1, "max_cells 1 is neither 0 nor in 2..32768"),
                              ("max_boxes", 129, "max_boxes 129 is outside 1..128"), ("pad", 257, "pad 257 is outside 0..256"), ("flags", 1, "unknown flags 0x1"),
                              ("reserved", (C.c_int * 4)(0, 0, 0, 1), "reserved must be 0")):
        sp = capi.blobs_spec(65, 33, 3, 8, min_cells=2)
        setattr(sp, field, value)
        with pytest.raises(Exception, match=re.escape(msg)):
            capi.blobs_spec_check(sp)
    with pytest.raises(Exception, match=re.escape("a grid of 480 x 270 cells (32768 cells at most)")):
        capi.blobs_spec_check(capi.blobs_spec(1920, 1080, 2, 1))
    assert capi.lib().ffgpu_blobs_dev(None, 1, None, None, 1, None, None, None, None) < 0
    assert ("NULL" if torch.cuda.is_available() else "no HIP device") in capi.last_error(), capi.last_error()


def test_reference_on_grids_written_out(capi):
    def one(rows, **kw):
        sp = blobref.Spec(4 * len(rows[0]) - 1, 4 * len(rows) - 2, 2, min_pixels=2, **kw)
        words, rec, labels = blobref.target(sp, 1, np.array(rows, "<u4"))
        return words[:5].tolist(), [tuple(float(v) for v in b.tolist()) for b in rec["box"][:rec["count"]]], labels.tolist(), (int(rec["ncand"]), int(rec["overflow"]))
    diag = [[16, 0, 0], [0, 9, 0], [0, 0, 2]]                    # the last cell is 3 x 2 pixels: min(2, 6) of 6
    assert one(diag, connect=8, type_=5) == ([3, 1, 1, 1, 0], [(5, (16 + 9 + 2) * 256 // 38 / 256, 0, 0, 10, 9)], [[1, 0, 0], [0, 1, 0], [0, 0, 1]], (1, 0))
    assert one(diag, connect=4, max_boxes=2, pad=1) == ([3, 3, 3, 2, 0], [(0, 1.0, 0, 0, 4, 4), (0, 9 / 16, 3, 3, 8, 8)], [[1, 0, 0], [0, 2, 0], [0, 0, 0xFFFF]], (3, 1))
    u = [[2, 1, 2], [2, 1, 2], [2, 2, 2]]                        # one component whose arms meet only in the last row; a cell of 1 stays out
    assert one(u, connect=4) == ([7, 1, 1, 1, 0], [(0, 14 * 256 // 78 / 256, 0, 0, 10, 9)], [[1, 0, 1], [1, 0, 1], [1, 1, 1]], (1, 0))
    tie = [[0, 3, 3, 1, 3, 3], [0, 0, 0, 1, 0, 0], [5, 0, 0, 0, 0, 0]]                                       # equal pixels and cells: the smaller root first; min_cells 2
    assert one(tie, connect=4, min_cells=2) == ([5, 3, 2, 2, 0], [(0, 6 * 256 // 32 / 256, 4, 0, 11, 3), (0, 6 * 256 // 28 / 256, 16, 0, 22, 3)],
                                                [[0, 1, 1, 0, 2, 2], [0] * 6, [0xFFFF, 0, 0, 0, 0, 0]], (2, 0))
