"""The 20-state device block exponential's operand layouts (csrc/k20_block_exp.hpp), without a GPU:
tests/cpp/k20_blockexp_check.cpp emulates v_mfma_f64_16x16x4_f64 by its lane map and, with small-integer
matrices without symmetry, proves exactly in every entry a left product taken straight from accumulator
layout, one full Taylor step, the re-deal of P and F into A operands through the LDS layout, and one
squaring step (P P and P F + F P); the transposed gather, which yields X^T D, must fail.  Built plainly
and as a stand-alone AddressSanitizer + UBSan program."""
import os
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "k20_blockexp_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_k20_blockexp_layouts(tmp_path, flags):
    exe = str(tmp_path / "k20_blockexp_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("k20 blockexp OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 100000
