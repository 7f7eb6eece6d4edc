"""The 20-state pair-sum consumer's operand re-deal (csrc/k20_preorder.hpp, k20_pair_source_lane and
k20_pair_entry), without a GPU: tests/cpp/k20_pairsum_check.cpp emulates the four-block 4x4x4 FP64 MFMA
by its lane map and forms a wave's 20 x 20 sum over its 16 sites from small-integer t and L without
symmetry -- the re-dealt operands, the 25 MFMAs and the fold over the four quads of sites must give
every entry exactly, sites past S must add nothing, and the swapped gather, which yields N^T, must
fail.  Also the consumer's LDS layout inside the walk's exchange area at 1 to 8 rate categories.
Built plainly and as a stand-alone AddressSanitizer + UBSan program."""
import os
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "k20_pairsum_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_k20_pairsum_redeal(tmp_path, flags):
    exe = str(tmp_path / "k20_pairsum_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("k20 pairsum OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 48000
