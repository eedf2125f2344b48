"""ffgpu_exec_forward_bgr_frames_dev without a GPU: the frame descriptor's layout in the ctypes mirror, the exported symbol, and the call
failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_bgr_frame_struct_layout(capi):
    F = capi.BgrFrame
    assert C.sizeof(F) == 24
    assert (F.bgr.offset, F.w.offset, F.h.offset, F.pitch.offset, F.reserved.offset) == (0, 8, 12, 16, 20)


def test_bgr_frames_symbol_exported(capi):
    assert "ffgpu_exec_forward_bgr_frames_dev" in capi.EXPORTS
    assert hasattr(capi.lib(), "ffgpu_exec_forward_bgr_frames_dev")


def test_frame_descriptors_from_tuples(capi):
    assert capi.bgr_frame_desc((4096, 640, 424)) == (4096, 640, 424, 0, 0)
    assert capi.bgr_frame_desc((4097, 5, 3, 17)) == (4097, 5, 3, 17, 0)


def test_bgr_frames_without_device(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    frames = (capi.BgrFrame * 1)(capi.BgrFrame(4096, 320, 320, 0, 0))
    m, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    rc = capi.lib().ffgpu_exec_forward_bgr_frames_dev(None, frames, 1, m, s, None)
    assert rc < 0
    assert "no HIP device" in capi.last_error()


def test_frame_tensors_must_be_device_u8(capi):
    """a host tensor's address or another element type never reaches the kernels"""
    import torch
    with pytest.raises(ValueError, match="device tensors"):
        capi.bgr_frame_desc(torch.zeros((4, 5, 3), dtype=torch.uint8))
    for dt in (torch.int8, torch.bool, torch.float32):
        with pytest.raises(TypeError, match="torch.uint8"):
            capi.bgr_frame_desc(torch.zeros((4, 15), dtype=dt))
