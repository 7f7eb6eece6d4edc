"""The 20-state derivative consumer's host-side packing (csrc/k20_preorder.hpp, k20_pack_copy), without
a GPU: tests/cpp/k20_qcopy_check.cpp emulates the four-block 4x4x4 FP64 MFMA by its lane map and forms
z = Q y and z2 = Q z through the walk's forward gather from the packed copy of a random asymmetric
matrix -- both must equal the dense products in every lane, exactly (small integers); the copy of the
transposed matrix and the transposed gather must not.  Also the consumer's LDS layout inside the walk's
exchange area at 1 to 8 rate categories.  Built plainly and as a stand-alone AddressSanitizer + UBSan
program."""
import os
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "k20_qcopy_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_k20_qcopy_packing(tmp_path, flags):
    exe = str(tmp_path / "k20_qcopy_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("k20 qcopy OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 80000
