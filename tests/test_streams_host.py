"""What the per-stream families (track, zones, trails, heat, motion) share on the host, without a GPU: ffgpu_streams_host.hpp's stream checks and the
bytes a reset clears, and ffgpu_args.hpp's colours, palettes and class tables, under ASan + UBSan (san/streams_driver.cc, run as a child process)."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")


def test_shared_host_pieces_are_plain_cpp_and_written_once():
    host = open(os.path.join(CSRC, "ffgpu_streams_host.hpp")).read()
    assert "hip/hip_runtime" not in host and "hipStream" not in host                    # plain C++: the sanitizer drivers compile it with no HIP
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".inc", ".hpp", ".hip", ".h", ".c"))}

    def where(text):
        return sorted(f for f, s in src.items() for _ in range(s.count(text)))
    assert where("stable_sort") == ["ffgpu_streams_host.hpp"]
    assert where("target %d: stream %d is outside -1 .. %d") == ["ffgpu_streams_host.hpp"]
    assert where("nclasses %d (0 with NULL classes") == ["ffgpu_args.hpp"] == where("npalette %d (0 with a NULL palette")
    assert where("hipMemsetAsync(p, 0, ") == ["ffgpu_kernels.hip"]
    for fam, header in (("TRACK", "ffgpu_track.inc"), ("ZONES", "ffgpu_zones_host.hpp"), ("TRAILS", "ffgpu_trails_host.hpp"), ("HEAT", "ffgpu_heat_host.hpp")):
        assert int(re.search(r"#define %s_ARG_ENTRIES\s+(\d+)" % fam, src[header]).group(1)) == (128 if fam in ("TRACK", "ZONES") else 64)
        assert "StreamEntries<%s_ARG_ENTRIES> en;" % fam in src["ffgpu_%s.inc" % fam.lower()]


def test_shared_host_pieces_under_the_sanitizers():
    """san/streams_driver.cc on the CPU under ASan + UBSan, as a child process; the driver checks every case itself.  A sanitizer report aborts the
    child: the test fails with it."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "streams"])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_streams_san")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err, out = r.stderr.decode(errors="replace"), r.stdout.decode().split("\n")[:-1]
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    assert re.fullmatch(r"streams_driver: (\d+) cases, 0 wrong", out[-1]) and int(out[-1].split()[1]) == len(out) - 1 >= 65, out[-1]
    assert not any("WRONG" in ln for ln in out)
    for ln in ("three.ntargets_first -1 op: 0 targets (ntargets >= 1)", "three.state_odd -1 op: the state must be 16-byte aligned",
               "range.high -1 op: target 1: stream 2 is outside -1 .. 1", "span.all 0 off=0 len=768", "span.first 0 off=0 len=256", "span.last 0 off=512 len=256",
               "span.which_nstreams -1 reset: stream 3 is outside -1 .. 2", "span.which_m2 -1 reset: stream -2 is outside -1 .. 2",
               "span.odd_state -1 reset: the state must be 16-byte aligned", "order.size_second -1 reset: 7 streams of 0 slots",
               "span.big_last 0 off=%d len=%d" % ((2 ** 48 - 1) * 65535, 2 ** 48 - 1), "colour.fourth_ignored 0x563412",
               "palette.count_257 -1 op: npalette 257 (0 with a NULL palette, else 1..256)", "classes.null_with_count -1 op: nclasses 80 (0 with NULL classes, else 1..256)"):
        assert ln in out, ln
