"""ffgpu_exec_forward_nv12_frames_dev without a GPU: the frame descriptor's layout in the ctypes mirror, the exported symbol, the
descriptor helper, and the call failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_nv12_frame_struct_layout(capi):
    F = capi.Nv12Frame
    assert C.sizeof(F) == 40
    assert (F.y.offset, F.uv.offset, F.w.offset, F.h.offset, F.pitch_y.offset, F.pitch_uv.offset, F.matrix.offset,
            F.reserved.offset) == (0, 8, 16, 20, 24, 28, 32, 36)
    assert (capi.YUV_BT601_LIMITED, capi.YUV_BT601_FULL, capi.YUV_BT709_LIMITED, capi.YUV_BT709_FULL) == (0, 1, 2, 3)


def test_nv12_frames_symbol_exported(capi):
    assert "ffgpu_exec_forward_nv12_frames_dev" in capi.EXPORTS
    assert hasattr(capi.lib(), "ffgpu_exec_forward_nv12_frames_dev")


def test_header_names_the_matrices():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffcnn_hip.h")).read()
    got = dict(re.findall(r"#define (FFGPU_YUV_\w+)\s+(\d+)", hdr))
    assert got == {"FFGPU_YUV_BT601_LIMITED": "0", "FFGPU_YUV_BT601_FULL": "1", "FFGPU_YUV_BT709_LIMITED": "2", "FFGPU_YUV_BT709_FULL": "3"}
    assert "} ffgpu_nv12_frame;" in hdr


def test_nv12_descriptors_from_tuples(capi):
    assert capi.nv12_frame_desc((4096, 0, 640, 424)) == (4096, 0, 640, 424, 0, 0, 0, 0)
    assert capi.nv12_frame_desc((4096, None, 640, 424), matrix=2) == (4096, 0, 640, 424, 0, 0, 2, 0)
    assert capi.nv12_frame_desc((4097, 8192, 5, 3, 17, 6)) == (4097, 8192, 5, 3, 17, 6, 0, 0)
    assert capi.nv12_frame_desc((4097, 8192, 5, 3, 17, 6, 3), matrix=1) == (4097, 8192, 5, 3, 17, 6, 3, 0)
    f = capi.Nv12Frame(*capi.nv12_frame_desc((4097, 0, 5, 3, 17, 6, 3)))
    assert (f.y, f.uv, f.w, f.h, f.pitch_y, f.pitch_uv, f.matrix, f.reserved) == (4097, None, 5, 3, 17, 6, 3, 0)


def test_nv12_descriptors_of_neither_form(capi):
    import numpy as np
    for f in ((4096, 640, 424), (np.int64(4096), np.int64(8192)), (None, None), 4096, (1, 0, 2, 3, 4, 5, 6, 7)):
        with pytest.raises(ValueError, match="a frame is"):
            capi.nv12_frame_desc(f)


def test_nv12_frames_without_device(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    frames = (capi.Nv12Frame * 1)(capi.Nv12Frame(4096, None, 320, 320, 0, 0, 0, 0))
    m, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    rc = capi.lib().ffgpu_exec_forward_nv12_frames_dev(None, frames, 1, m, s, None)
    assert rc < 0
    assert "no HIP device" in capi.last_error()


def test_nv12_frame_tensors_must_be_device_u8(capi):
    """a host tensor's address or another element type never reaches the kernels"""
    import torch
    with pytest.raises(ValueError, match="device tensors"):
        capi.nv12_frame_desc((torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((2, 6), dtype=torch.uint8)))
    for dt in (torch.int8, torch.bool, torch.float32):
        with pytest.raises(TypeError, match="torch.uint8"):
            capi.nv12_frame_desc((torch.zeros((4, 6), dtype=dt), torch.zeros((2, 6), dtype=dt)))
