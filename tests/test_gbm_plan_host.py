"""CPU: sbag_gbm_plan.h, the loss arithmetic, code cuts and sizes k_gbm_step shares with its
host code, swept by the stand-alone tests/c/gbm_plan_check.cpp, plain and under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "gbm_plan_check.cpp")
INC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_gbm_plan_sweep(tmp_path, flags):
    exe = str(tmp_path / "gbm_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags,
                           "-I", INC, "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"gbm_plan_check: (\d+) cases, 0 failures", p.stdout)
    assert m and int(m.group(1)) > 2_000_000, p.stdout[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
