"""CPU: sbag_ingest_plan.h, the key transform, set geometry, tiles and batches the ingest kernels
share with their host code, checked by the stand-alone tests/c/ingest_plan_check.cpp, plain and
under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "ingest_plan_check.cpp")
INC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_ingest_plan_check(tmp_path, flags):
    exe = str(tmp_path / "ingest_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert re.search(r"ingest_plan_check: \d+ cases, 0 failures", p.stdout), p.stdout[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
