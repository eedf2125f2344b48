"""Flow maps, without a GPU: the seven exported symbols, the layout of the spec struct in the ctypes mirror, ffgpu_flow_state_bytes against the
reference's layout, ffgpu_flow_spec_check on one bad value per field, the host glue under ASan + UBSan (san/flow_driver.cc, run as a child process:
every rejection with its message), and the device entry points failing the way every entry point of the library does when no HIP device is visible."""
import ctypes as C
import re

import pytest

from sanrun import check_summary, run_driver
from flow import flowref

SYMBOLS = ["ffgpu_flow_state_bytes", "ffgpu_flow_spec_check", "ffgpu_flow_reset_dev", "ffgpu_flow_update_bgr_dev", "ffgpu_flow_update_nv12_dev",
           "ffgpu_flow_boxes_dev", "ffgpu_exec_flow_boxes"]


@pytest.fixture(scope="module")
def capi():
    from ffcnn_amd import capi as m
    m.build_library()
    return m


def test_flow_symbols_exported(capi):
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s


def test_flow_struct_layout_and_state_bytes(capi):
    Sp = capi.FlowSpec
    assert C.sizeof(Sp) == 64 and capi.FLOW_RECORD_DTYPE == flowref.RECORD and flowref.RECORD.itemsize == 8
    assert [getattr(Sp, f).offset for f in ("w", "h", "block_log2", "range", "min_spread", "flags", "min_score", "nclasses", "classes", "reserved")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert (capi.FLOW_DETS, capi.FLOW_ROW, capi.FLOW_WORDS, capi.FLOW_MAX_SIDE, capi.FLOW_STATE_HEADER, capi.FLOW_ENTRIES, capi.FLOW_MERGED) == \
        (flowref.DETS, flowref.ROW, flowref.WORDS, flowref.MAX_SIDE, flowref.STATE_HEADER, 0, 1)
    for args in ((1, 5, 3, 4), (3, 71, 37, 3), (2, 1920, 1080, 4)):
        assert capi.flow_state_bytes(*args) == flowref.state_nbytes(*args) > 0, args
    for args in ((0, 1, 1, 3), (65537, 1, 1, 3), (1, 0, 1, 3), (1, 1, 8193, 3), (1, 1, 1, 2), (1, 1, 1, 5)):
        assert capi.flow_state_bytes(*args) == 0 == flowref.state_nbytes(*args), args
    st = flowref.State(2, 71, 37, 3)
    st.hdr[1], st.planes[1, 1, 36, 70], st.recs[1, 4, 8] = (5, -1, 2, 3), 200, (-3, 4, 500, 600)
    hdr, planes, recs = capi.flow_state(st.raw, 2, 71, 37, 3)
    assert hdr.tolist() == st.hdr.tolist() and planes.tobytes() == st.planes.tobytes() and recs.tobytes() == st.recs.tobytes() and recs.shape == (2, 5, 9)


def test_flow_spec_check(capi):
    capi.flow_spec_check(capi.flow_spec(65, 33, 4, 16, 65535, 0.5, classes=[1, 0, 2]))
    for field, value, msg in (("w", 0, "a model of 0 x 33 pixels (1..8192 each)"), ("h", 8193, "a model of 65 x 8193 pixels"), ("block_log2", 5, "block_log2 5 is outside 3..4"),
                              ("range", 17, "range 17 is outside 1..16"), ("min_spread", 65536, "min_spread 65536 is outside 0..65535"), ("flags", 2, "unknown flags 0x2"),
                              ("nclasses", 2, "nclasses 2 (0 with NULL classes, else 1..256)"), ("reserved", (C.c_int * 6)(0, 0, 0, 0, 0, 1), "reserved must be 0")):
        sp = capi.flow_spec(65, 33, 3, 8)
        setattr(sp, field, value)
        with pytest.raises(Exception, match=re.escape(msg)):
            capi.flow_spec_check(sp)


def test_host_glue_under_the_sanitizers():
    """san/flow_driver.cc: the state's layout, the spec's plan, the argument checks of ffgpu_flow_host.hpp and the rounds of an update call on the CPU
    under ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the child: the test fails with it."""
    check_summary(run_driver("flow", "flow"), "flow", 60)


def test_flow_without_device(capi):
    """with no HIP device every device entry point says so (with one, the same calls are rejected for their NULL arguments)"""
    import torch
    L = capi.lib()
    want = "NULL" if torch.cuda.is_available() else "no HIP device"
    for call in (lambda: L.ffgpu_flow_reset_dev(None, 1, 1, 1, 3, -1, None),
                 lambda: L.ffgpu_flow_update_bgr_dev(None, 1, None, None, None, 1, None, None),
                 lambda: L.ffgpu_flow_update_nv12_dev(None, 1, None, None, None, 1, None, None),
                 lambda: L.ffgpu_flow_boxes_dev(None, None, 0, None, None, 1, None, None, 1, None, None),
                 lambda: L.ffgpu_exec_flow_boxes(None, 0, None, 1, None, None, 1, None, None)):
        assert call() < 0 and want in capi.last_error(), capi.last_error()
