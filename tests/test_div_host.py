"""CPU: div_rn_small (spark-bagging_amd/csrc/sbag_div.h), the by-hand rounding of a subnormal
quotient that the fp64 engine's gain kernels use (the GPU's division sequence rounds an exact
tie of a subnormal quotient either way; IEEE 754, and with it the JVM, rounds it to even),
swept by the stand-alone program tests/c/div_check.cpp against the host's own division bit
for bit: millions of quotients below 2^-1021, tens of thousands of exact ties among them.
Pure host arithmetic in a program of its own, so it also runs under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "div_check.cpp")
INC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_div_rn_small_sweep(tmp_path, flags):
    exe = str(tmp_path / "div_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags,
                           "-I", INC, "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"div_check: (\d+) cases \((\d+) exact ties\), 0 failures", p.stdout)
    assert m, p.stdout[-2000:]
    assert int(m.group(1)) > 5_000_000 and int(m.group(2)) > 10_000, m.group(0)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_gain_kernels_divide_through_div_rn():
    """Variance.calculate on the device (k_fb_finish, k_f64_split) takes both its divisions
    from the header."""
    for name, fn in (("sbag_f64s.hip", "var_imp"), ("sbag_f64.hip", "var_impurity")):
        text = open(os.path.join(INC, name)).read()
        assert '#include "sbag_div.h"' in text
        body = text[text.index(f"double {fn}("):]
        body = body[: body.index("\n}")]
        assert body.count("div_rn(") == 2 and " / " not in body, body
