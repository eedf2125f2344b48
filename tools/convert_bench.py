#!/usr/bin/env python3
"""Device time of the convert launches: HIP events on one stream, 64 surfaces of 1920 x 1080 converted in one call.  Six legs: NV12 to
BGR, I420 to NV12, BGR to NV12, YUY2 to BGR, P010 to NV12 with every plane at a 256-byte address and pitches that are multiples of 4 (the aligned
form), and NV12 to BGR from rows offset by one byte (the general form).  10 warm-up calls a leg, then three repeats that ALTERNATE between the legs,
20 timed calls a leg and repeat, a 256 MB memset in front of every sample; per leg the median of each repeat, and of the middle repeat its
algorithmic bytes -- every source byte once plus every destination byte once -- as bytes/s and as a fraction of 8 TB/s.  The yardsticks for a frame
reader of this tree are the motion update, the preview and the warp: run tools/motion_bench.py, tools/preview_bench.py and tools/warp_bench.py on
the same box in the same sitting.
Prints one line per leg; with a path argument they are written there too:  python tools/convert_bench.py [profiles/convert_bench.txt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ffcnn_amd import capi as F  # noqa: E402

B, W, H, PEAK, WARM, TIMED, REPEATS = 64, 1920, 1080, 8e12, 10, 20, 3
CW, CH = (W + 1) // 2, (H + 1) // 2
st = torch.cuda.Stream()
S = st.cuda_stream
L = F.lib()
# the planes of a layout as (rows, bytes of a row)
LAYOUT = {"NV12": [(H, W), (CH, 2 * CW)], "I420": [(H, W), (CH, CW), (CH, CW)], "BGR": [(H, 3 * W)], "YUY2": [(H, 4 * CW)], "P010": [(H, 2 * W), (CH, 4 * CW)]}
PIX = {"NV12": F.PIX_NV12, "I420": F.PIX_I420, "BGR": F.PIX_BGR24, "YUY2": F.PIX_YUY2, "P010": F.PIX_P010}
LEGS = [("nv12_to_bgr_aligned", "NV12", "BGR", 0), ("i420_to_nv12_aligned", "I420", "NV12", 0), ("bgr_to_nv12_aligned", "BGR", "NV12", 0),
        ("yuy2_to_bgr_aligned", "YUY2", "BGR", 0), ("p010_to_nv12_aligned", "P010", "NV12", 0), ("nv12_to_bgr_rows_off_by_one", "NV12", "BGR", 1)]


def surfaces(layout, off):
    """B surfaces of random bytes in one buffer: (the buffer, per surface its planes as (address, pitch)); off = 1: every plane a byte (a pair
    plane two) behind a 256-byte address, every pitch that much longer"""
    one, rel = 0, []
    for k, (rows, nb) in enumerate(LAYOUT[layout]):
        o = off * (2 if layout == "NV12" and k == 1 else 1)
        rel.append((one + o, nb + o))
        one += (rows * (nb + o) + o + 255) & ~255
    buf = torch.randint(0, 256, (B * one,), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, [[(buf.data_ptr() + n * one + r, p) for r, p in rel] for n in range(B)]


def leg(src, dst, off):
    """(the buffers, a call of the leg, its algorithmic bytes)"""
    sbuf, sp = surfaces(src, off)
    dbuf, dp = surfaces(dst, off)
    ss = F._surfaces([F.surface(PIX[src], W, H, [a for a, _ in pl], [p for _, p in pl], 2) for pl in sp])
    if dst == "BGR":
        dd, fn = F.bgr_frame_table([(pl[0][0], W, H, pl[0][1]) for pl in dp]), L.ffgpu_convert_bgr_dev
    else:
        dd, fn = F.nv12_frame_table([(pl[0][0], pl[1][0], W, H, pl[0][1], pl[1][1]) for pl in dp]), L.ffgpu_convert_nv12_dev
    return (sbuf, dbuf, ss, dd), (lambda: fn(ss, dd, B, S)), B * sum(rows * nb for rows, nb in LAYOUT[src] + LAYOUT[dst])


def median_us(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        flush.zero_()                                       # the host runs ahead of the device: the events bracket the leg's kernels alone
        a.record(st)
        assert fn() == 0, F.last_error()
        b.record(st)
    st.synchronize()
    return sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)[n // 2]


with torch.cuda.stream(st):
    flush = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    legs = [(name,) + leg(src, dst, off) for name, src, dst, off in LEGS]
    for _, _, fn, _ in legs:
        median_us(fn, WARM)
    times = {name: [] for name, _, _, _ in legs}
    for _ in range(REPEATS):
        for name, _, fn, _ in legs:
            times[name].append(median_us(fn, TIMED))
lines = ["convert_bench: %d surfaces of %d x %d a call, tile %s, %d warm-up + %d x %d timed calls a leg, against %.0f TB/s" % (B, W, H, F.convert_tile(), WARM, REPEATS, TIMED, PEAK / 1e12)]
for name, _, _, nbytes in legs:
    t = sorted(times[name])
    lines.append("%-30s median us of the repeats %s  spread %5.1f %%  %6.1f MB  %7.1f GB/s  %5.3f of peak"
                 % (name, " ".join("%8.1f" % v for v in times[name]), 100 * (t[-1] - t[0]) / t[1], nbytes / 1e6, nbytes / (t[1] * 1e-6) / 1e9, nbytes / (t[1] * 1e-6) / PEAK))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
