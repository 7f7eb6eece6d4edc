"""The host-only branch-length optimiser (csrc/brlen_opt.hpp), without a GPU: driven by
tests/cpp/brlen_opt_check.cpp on closed-form concave objectives whose optimum is known -- separable,
a pair of which only the sum is identified, optima at either bound, starts at a bound -- with, per
case, a lnL sequence that never decreases, every evaluated point inside the box, a predicted gain
below atol at exit when converged is reported, and converged = 0 for max_iters = 1.  Built plainly
and as a stand-alone AddressSanitizer + UBSan program."""
import os
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "brlen_opt_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_optimiser_on_closed_form_objectives(tmp_path, flags):
    exe = str(tmp_path / "brlen_opt_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("brlen opt OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 1000
