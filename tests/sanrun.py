"""Runs a stand-alone host-check driver (ffcnn_amd/csrc/san/<name>_driver.cc: plain host C++ with its own main, built under ASan + UBSan by
`make -C ffcnn_amd/csrc <target>`) as a child process -- test infrastructure.  A sanitizer report aborts the child: the calling test fails with it."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "ffcnn_amd", "csrc")


def run_driver(target, name, *argv):
    """builds `target`, runs bin/ffgpu_<name>_san with argv, wants exit code 0 and a stderr free of sanitizer reports; returns the lines of its stdout"""
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = os.path.join(ROOT, "ffcnn_amd", "bin", "ffgpu_%s_san" % name)
    r = subprocess.run([exe, *argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "rc %d\n%s" % (r.returncode, err[-3000:])
    return r.stdout.decode().split("\n")[:-1]


def check_summary(lines, name, at_least, exact=True):
    """the driver's own verdict: the last line is "<name>_driver: N cases, 0 wrong", the lines before it are at_least or more, N is their number
    (exact) or, for a driver that counts facts it prints no line for, at least their number, and no line is marked WRONG; returns N"""
    m = re.fullmatch(r"%s_driver: (\d+) cases, 0 wrong" % name, lines[-1])
    assert m, lines[-1]
    n, printed = int(m.group(1)), len(lines) - 1
    assert (n == printed if exact else n >= printed) and printed >= at_least, lines[-1]
    assert not any("WRONG" in ln for ln in lines)
    return n
