"""CPU: which entry of its run a lane of k_fb_psum loads (psum_slot,
spark-bagging_amd/csrc/sbag_psum_index.h), swept by the stand-alone program
tests/c/psum_index_check.cpp over every R the kernel is instantiated for, run lengths 0..1100
and a few near 2^31 - 1, every step, round and lane: a load index is inside the run, an empty
run loads nothing, only valid lanes' entries are used, and the valid lanes cover every entry of
the run exactly once.  The kernel's reads past a run are masked out of its sums, so no GPU
output can show them: this rule is what keeps them inside the run.  Pure host arithmetic in a
program of its own, so it also runs under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "psum_index_check.cpp")
INC = os.path.join(ROOT, "spark-bagging_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address",
                                             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_psum_slot_sweep(tmp_path, flags):
    exe = str(tmp_path / "psum_index_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                           "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    m = re.search(r"psum_index_check: (\d+) cases \((\d+) slots, (\d+) of empty runs, (\d+) clamped\), "
                  r"0 failures", p.stdout)
    assert m, p.stdout[-2000:]
    # the whole grid ran: 4 values of R x (1101 lengths x 4 step counts + 7 long runs); empty
    # runs and lanes past a run's end both occur in it
    assert int(m.group(1)) == 4 * (1101 * 4 + 7), m.group(0)
    assert int(m.group(2)) > 100_000_000 and int(m.group(3)) > 0 and int(m.group(4)) > 0, m.group(0)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_psum_index_header_is_plain_host_code():
    """The header stays includable by a program with no HIP: only <cstdint>."""
    text = open(os.path.join(INC, "sbag_psum_index.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint"]
    # and the kernel takes its rule from it
    kernel = open(os.path.join(INC, "sbag_f64s.hip")).read()
    assert '#include "sbag_psum_index.h"' in kernel and kernel.count("psum_slot(") >= 2
