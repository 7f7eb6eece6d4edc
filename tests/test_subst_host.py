"""rdamd_substitution_counts_from_pair_sums (csrc/subst_map.hpp, host only) against tests/subst_ref.py,
without a GPU, on pair sums made by grad_ref on a 10-taxon tree with P-matrices from
scipy.linalg.expm: K = 4 and K = 2, one rate matrix and two (params_indices [0,1,1,0]), and branch
lengths that include 0, 1e-6, 0.1 and 100.

Both sides evaluate one formula in double precision; they differ in the order of the operations (a
Taylor core with scaling and squaring here, SciPy's Pade of the 2K x 2K block matrix there).  The
figure compared is |x - x_ref| against 1e-11 of the entry's absolute-value companion: the same sum
with |X| and |N| (subst_ref.typed_counts; every term is non-negative, so the companion is the entry).

Also the stand-alone program tests/cpp/subst_counts_check.cpp (the count matrices C for K = 2, 4
and 20 from length 0 to 100, identities of the typed counts, the error codes), built plainly and
as an AddressSanitizer + UBSan program."""
import os
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
import grad_ref
import subst_ref
import util
from test_subst_reference import ten

TOL = 1e-11
SRC = os.path.join(util.ROOT, "tests", "cpp", "subst_counts_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


def make_case(K, sets, rng):
    pidx = [0, 1, 1, 0] if sets == 2 else None
    case = ten(rng, K=K, R=4, sets=sets, pidx=pidx, brl_set={1: 1e-6, 5: 0.1, 11: 100.0, 14: 0.0})
    assert {0.0, 1e-6, 0.1, 100.0} <= set(case["lengths"].ravel())
    N, _, _ = grad_ref.pair_sums(case["ops"], case["tips"], case["tipvec"], case["pmat"], case["pis"], case["w"],
                                 case["weights"])
    return case, N


@pytest.mark.parametrize("K,sets", [(4, 1), (4, 2), (2, 1), (2, 2)])
def test_host_counts_equal_the_restatement(K, sets):
    rng = np.random.default_rng(10 * K + sets)
    case, N = make_case(K, sets, rng)
    want, comp, _, _ = subst_ref.typed_counts(N, case["lengths"], case["qs"], case["rates"])
    got = rd.substitution_counts(N, case["lengths"], case["subst"], case["freqs"], case["pidx"], case["rates"])
    assert got.shape == want.shape == (len(case["ops"]), 2, K, K) and np.all(np.isfinite(got))
    ratio = np.abs(got - want) / np.where(comp > 0, comp, 1.0)
    print("K %d, %d rate matrices: largest |x - x_ref| / companion %.3e (largest entry %.3e)" % (K, sets, ratio.max(), want.max()))
    assert np.all(np.abs(got - want) <= TOL * comp)
    zero = case["lengths"] == 0.0
    assert np.all(got[zero] == 0.0)
    # identity D on the host's own numbers
    total = case["weights"].sum()
    dwell = np.trace(got, axis1=2, axis2=3)
    assert np.all(np.abs(dwell - case["lengths"] * total) <= TOL * case["lengths"] * total)
    # a pure function: the same again
    again = rd.substitution_counts(N, case["lengths"], case["subst"], case["freqs"], case["pidx"], case["rates"])
    assert got.tobytes() == again.tobytes()


def test_refusals():
    rng = np.random.default_rng(1)
    case, N = make_case(4, 2, rng)
    args = (case["subst"], case["freqs"])
    with pytest.raises(rd.RdamdError, match="index out of range"):
        rd.substitution_counts(N, case["lengths"], *args, [0, 2, 1, 0], case["rates"])
    assert rd.lib.rdamd_errno() == 7
    for bad in (-0.5, np.inf, np.nan):
        lengths = case["lengths"].copy()
        lengths[3, 1] = bad
        with pytest.raises(rd.RdamdError, match="negative or not finite"):
            rd.substitution_counts(N, lengths, *args, case["pidx"], case["rates"])
        assert rd.lib.rdamd_errno() == 64
    assert rd.lib.rdamd_substitution_counts_from_pair_sums(4, 4, 2, len(N), None, None, None, None, None, None, None) != 1
    assert rd.lib.rdamd_errno() == 64
    typed = np.zeros((len(N), 2, 4, 4))
    lengths = np.ascontiguousarray(case["lengths"])
    subst, freqs = np.ascontiguousarray(case["subst"]), np.ascontiguousarray(case["freqs"])
    pidx, rates = np.array(case["pidx"], dtype=np.uint32), np.ascontiguousarray(case["rates"])

    def call(states):
        return rd.lib.rdamd_substitution_counts_from_pair_sums(states, 4, 2, len(N), rd.api._dptr(N), rd.api._dptr(lengths),
                                                               rd.api._dptr(subst), rd.api._dptr(freqs), rd.api._uptr(pidx),
                                                               rd.api._dptr(rates), rd.api._dptr(typed))
    for states in (1, 65):
        assert call(states) != 1 and rd.lib.rdamd_errno() == 64
    assert call(4) == 1 and rd.lib.rdamd_errno() == 0   # a valid call after the refusals


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_count_matrices_stand_alone(tmp_path, flags):
    exe = str(tmp_path / "subst_counts_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("subst counts OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 10000
