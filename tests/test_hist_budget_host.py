"""CPU: the bit budget of the packed LDS histogram word (hist_word_budget,
spark-bagging_amd/csrc/sbag_budget.h) swept at the edges of every field by the stand-alone
program tests/c/budget_check.cpp, which checks each result in 128-bit integers: the low field
cannot carry into the count, the count cannot wrap, the sum-of-squares word stays in 64 bits,
the hand-over to the fp64 engine sits exactly at N cmax kabs^2 = 2^53, the row-lane kernel's
24- and 32-bit products hold, and flush_limit is the largest power of two that fits.  Pure host
arithmetic in a program of its own, so it also runs under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "budget_check.cpp")
INC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_hist_word_budget_sweep(tmp_path, flags):
    exe = str(tmp_path / "budget_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                           "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"budget_check: (\d+) cases \((\d+) handed to fp64, (\d+) at cshift 32\), 0 failures",
                  p.stdout)
    assert m, p.stdout[-2000:]
    # the whole grid ran, and both the hand-over and the raised cshift occur in it
    assert int(m.group(1)) > 500_000 and int(m.group(2)) > 0 and int(m.group(3)) > 0
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_budget_header_is_plain_host_code():
    """The header stays includable by a program with no HIP: only <cstdint> and <cmath>."""
    text = open(os.path.join(INC, "sbag_budget.h")).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["cmath", "cstdint"]
