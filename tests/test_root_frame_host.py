"""csrc/root_frame.hpp (host only): what the analyses at a root read off a schedule before any kernel
runs.  The stand-alone program tests/cpp/root_frame_check.cpp replays hand-written schedules of 3, 4
and 5 tips (node arrays against plan_outer_program's own output, every branch's place and length
against a linear search, the refusal of an incomplete traversal) and scatter_columns against an
index-by-index loop; built plainly and as an AddressSanitizer + UBSan program.  Everything compared
is an integer or a copied double: equality, no tolerance."""
import os
import subprocess

import pytest

import util

SRC = os.path.join(util.ROOT, "tests", "cpp", "root_frame_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_root_frame_and_column_scatter(tmp_path, flags):
    exe = str(tmp_path / "root_frame_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("root frame OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 1000
