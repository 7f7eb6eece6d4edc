"""Pure host logic of round 3, without a GPU: the subtree pattern-class census behind the
clade tables (csrc/clade_classes.hpp), the cutting of a 20-state operation list into
side-by-side pieces (csrc/k20_split.hpp), the traversal compiler of the fused evaluators
(csrc/traversal_compiler.hpp) as the schedule planner configures it (csrc/schedule_plan.hpp: the
programs rdamd_schedule_create hands the kernels, replayed symbolically), the rest of that planner
(the lists it refuses and where, the clades it folds into pseudo-tips, the layout of a schedule's
device block), the planner of the CLV traversal launches (csrc/clv_plan.hpp: its plans replayed
symbolically) and the rule that picks the fused 4-state evaluator's variant for a batch
(csrc/launch_plan.hpp), checked by tests/cpp/host_logic_check.cpp."""
import os
import subprocess

import util


def test_clade_classes_k20_split_and_traversal_compiler(tmp_path):
    exe = str(tmp_path / "host_logic_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(util.ROOT, "root_digger_amd", "csrc"),
                           "-I", os.path.join(util.ROOT, "include"),
                           # (fused.hpp includes the HIP runtime header for its prototypes: host mode)
                           "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(util.ROOT, "tests", "cpp", "host_logic_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("host logic OK"), out.stdout
    # (602 of them the CLV planner's, 1440 the schedule planner's, 1693 the launch rule's)
    assert int(out.stdout.split()[-1]) >= 5329
    # the launch rule's choice for the benchmark's workloads and the two launches beyond the LDS limit
    rule = [ln for ln in out.stderr.splitlines() if ln.startswith("launch rule")]
    print("\n".join(rule))
    for name in ("c2", "c4", "c5", "c4/8", "d125", "balanced700"):
        assert sum(ln.split()[2] == name for ln in rule) == 1, name
    assert sum("LDS case A" in ln and "182272 B" in ln and "RW 0" in ln for ln in rule) == 1
    assert sum("LDS case B" in ln and "303104 B" in ln and "RW 0" in ln for ln in rule) == 1


def test_host_logic_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same checks (the list cuts, their levels, the traversal compiler with its parks placed one by
    one, the CLV traversal planner) in an AddressSanitizer + UBSan build: the host code that decides
    what every kernel launch of the path looks like"""
    exe = str(tmp_path / "host_logic_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(util.ROOT, "root_digger_amd", "csrc"), "-I", os.path.join(util.ROOT, "include"),
                           "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(util.ROOT, "tests", "cpp", "host_logic_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("host logic OK"), (out.stdout, out.stderr[-2000:])

