"""CPU: the MFMA root's label digit planes (mfma_digit_plan and mfma_label_digits,
spark-bagging_amd/csrc/sbag_mfma_plan.h) swept by the stand-alone program
tests/c/mfma_plan_check.cpp over image ranges at the edges of every plane count (|k| < 2^23),
with the encoding chosen by the host and forced either way: the digits of a label sum back to
k + dK0, each lies in [0, 127] or [-128, 127], dK0 fits int32, the plane count is the smallest
that holds the range about its offset, auto is the smaller of the two, 127 |d| 65536 < 2^31,
k_hist_mfma's int64 recombination cannot overflow for N <= 2^30, and no range needs more than 4
planes in either encoding.  Pure host arithmetic in a program of its own, so it also runs
under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "mfma_plan_check.cpp")
INC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_mfma_digit_plan_sweep(tmp_path, flags):
    exe = str(tmp_path / "mfma_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                           "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"mfma_plan_check: (\d+) ranges, (\d+) labels, max planes auto (\d+) / 7-bit (\d+) / "
                  r"balanced (\d+), 0 failures", p.stdout)
    assert m, p.stdout[-2000:]
    # the whole grid ran; k_hist_mfma<MT, 5> and <MT, 6> are unreachable
    assert int(m.group(1)) > 140_000 and int(m.group(2)) > 5_000_000
    assert (int(m.group(3)), int(m.group(4)), int(m.group(5))) == (4, 4, 4)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_plan_header_is_plain_host_code():
    """The header stays includable by a program with no HIP: only <cstdint>."""
    text = open(os.path.join(INC, "sbag_mfma_plan.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint"]
