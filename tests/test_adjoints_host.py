"""rdamd_pair_sum_adjoints on the host route, rdamd_gradient_from_adjoints and
rdamd_substitution_counts_from_adjoints (csrc/param_gradient.hpp, csrc/subst_map.hpp), without a GPU: on
pair sums made by grad_ref on a 10-taxon tree, K = 2, 4 and 20, one rate matrix and two
(params_indices [0,1,1,0]), branch lengths that include 0, 1e-6, 0.1, 1 and 100 and gamma rates at alpha 0.7.

The split is exact: the gradient and the typed counts assembled from the adjoints have the bytes of
gradient_from_pair_sums and substitution_counts, which are "adjoints on the host, then assemble".

The host adjoints at K = 20 against grad_ref.frechet (SciPy's expm of the 40 x 40 block), normwise per
problem, max|F - F_ref| / max|F_ref|: entry by entry SciPy itself is off by 1e-7 relative on small
entries at short lengths, so only the norm is compared.  Measured worst over both cases: 1.7e-13 (one
rate matrix, rho tau = 264, the length 100 at the top gamma rate; 9.0e-14 with two rate matrices); TOL
is 100 times that."""
import numpy as np
import pytest

import root_digger_amd as rd
import brlen_ref
import grad_ref
from test_subst_reference import ten

TOL = 100 * 1.7e-13
LENGTHS = {1: 1e-6, 5: 0.1, 11: 100.0, 14: 0.0, 8: 1.0}
CASES = {}


def case_of(K, sets):
    """the case and its pair sums, made once"""
    if (K, sets) not in CASES:
        rng = np.random.default_rng(10 * K + sets)
        case = ten(rng, K=K, R=4, S=23 if K == 20 else 41, sets=sets, pidx=[0, 1, 1, 0] if sets == 2 else None, brl_set=LENGTHS)
        assert {0.0, 1e-6, 0.1, 1.0, 100.0} <= set(case["lengths"].ravel())
        sums = grad_ref.pair_sums(case["ops"], case["tips"], case["tipvec"], case["pmat"], case["pis"], case["w"], case["weights"])
        for v in sums:
            v.setflags(write=False)
        CASES[(K, sets)] = case, sums
    return CASES[(K, sets)]


def model_args(case):
    return case["lengths"], case["subst"], case["freqs"], case["pidx"], case["rates"]


@pytest.mark.parametrize("K,sets", [(K, sets) for K in (2, 4, 20) for sets in (1, 2)])
def test_assemblies_from_host_adjoints_have_the_old_bytes(K, sets):
    case, (N, M, W) = case_of(K, sets)
    lengths, subst, freqs, pidx, rates = model_args(case)
    F = rd.pair_sum_adjoints(N, *model_args(case), where="host")
    assert rd.pair_sum_adjoints_last_ms() == 0
    assert F.shape == N.shape and np.all(np.isfinite(F)) and F.min() >= 0 and F.max() > 0
    assert F.tobytes() == rd.pair_sum_adjoints(N, *model_args(case), where="host").tobytes()
    if K != 20 or rd.device_count() == 0:   # auto: the host for every other state count, and where no device is
        assert F.tobytes() == rd.pair_sum_adjoints(N, *model_args(case)).tobytes()
    g = rd.gradient_from_adjoints(F, M, W, lengths, subst, freqs, pidx, pidx, rates, case["w"])
    old = rd.gradient_from_pair_sums(N, M, W, lengths, subst, freqs, pidx, pidx, rates, case["w"])
    assert all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(g, old))
    assert np.abs(g[0]).max() > 0 and np.abs(g[2]).max() > 0
    typed = rd.substitution_counts_from_adjoints(F, *model_args(case))
    assert typed.tobytes() == rd.substitution_counts(N, *model_args(case)).tobytes() and typed.max() > 0


@pytest.mark.parametrize("K", [2, 4, 20])
def test_zero_sums_and_zero_lengths_are_exact(K):
    case, (N, _, _) = case_of(K, 2)
    assert np.all(rd.pair_sum_adjoints(np.zeros_like(N), *model_args(case), where="host") == 0.0)
    F = rd.pair_sum_adjoints(N, *model_args(case), where="host")
    zero = case["lengths"] == 0.0
    assert zero.any() and F[zero].tobytes() == np.ascontiguousarray(N[zero]).tobytes()   # tau = 0: F = N
    empty = rd.pair_sum_adjoints(N[:0], case["lengths"][:0], *model_args(case)[1:], where="host")   # zero operations
    assert empty.shape == (0,) + N.shape[1:]


@pytest.mark.parametrize("sets", [1, 2])
def test_host_adjoints_against_scipy_at_20_states(sets):
    case, (N, _, _) = case_of(20, sets)
    F = rd.pair_sum_adjoints(N, *model_args(case), where="host")
    q = [brlen_ref.build_q(s, f) for s, f in zip(case["subst"], case["freqs"])]
    worst = (0.0, 0.0)
    for k in range(N.shape[0]):
        for c in range(2):
            for r in range(4):
                rt = case["rates"][r] * case["lengths"][k, c]
                ref = grad_ref.frechet(rt * q[case["pidx"][r]].T, N[k, c, r])
                err = np.abs(F[k, c, r] - ref).max() / np.abs(ref).max()
                worst = max(worst, (err, rt))
                assert err <= TOL, (k, c, r, rt, err)
    print("K 20, %d rate matrices: largest max|F - F_ref| / max|F_ref| %.3e at rho tau %.4g" % ((sets,) + worst))


def test_refusals():
    case, (N, M, W) = case_of(4, 2)
    lengths, subst, freqs, pidx, rates = model_args(case)
    with pytest.raises(rd.RdamdError, match="index out of range"):
        rd.pair_sum_adjoints(N, lengths, subst, freqs, [0, 2, 1, 0], rates, where="host")
    assert rd.lib.rdamd_errno() == 7
    for bad in (-0.5, np.inf, np.nan):
        moved = lengths.copy()
        moved[3, 1] = bad
        with pytest.raises(rd.RdamdError, match="negative or not finite"):
            rd.pair_sum_adjoints(N, moved, subst, freqs, pidx, rates)
        assert rd.lib.rdamd_errno() == 64
        moved = rates.copy()
        moved[2] = bad
        with pytest.raises(rd.RdamdError, match="negative or not finite"):
            rd.pair_sum_adjoints(N, lengths, subst, freqs, pidx, moved)
        assert rd.lib.rdamd_errno() == 64
    with pytest.raises(rd.RdamdError, match="20 states, not 4"):
        rd.pair_sum_adjoints(N, *model_args(case), where="device")
    assert rd.lib.rdamd_errno() == 63 and rd.pair_sum_adjoints_last_ms() == 0
    if rd.device_count() == 0:
        big, (N20, _, _) = case_of(20, 1)
        with pytest.raises(rd.RdamdError, match="no device is present"):
            rd.pair_sum_adjoints(N20, *model_args(big), where="device")
        assert rd.lib.rdamd_errno() == 63
    with pytest.raises(ValueError):
        rd.pair_sum_adjoints(N, *model_args(case), where="elsewhere")
    assert rd.lib.rdamd_pair_sum_adjoints(4, 4, 2, len(N), None, None, None, None, None, None, 1, None) != 1
    assert rd.lib.rdamd_errno() == 64
    out = np.zeros_like(N)
    pair = np.ascontiguousarray(N)
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (lengths, subst, freqs, rates)]
    pi = np.array(pidx, dtype=np.uint32)

    def call(states, where=1):
        return rd.lib.rdamd_pair_sum_adjoints(states, 4, 2, len(N), rd.api._dptr(pair), rd.api._dptr(a[0]), rd.api._dptr(a[1]),
                                              rd.api._dptr(a[2]), rd.api._uptr(pi), rd.api._dptr(a[3]), where, rd.api._dptr(out))
    for states in (1, 65):
        assert call(states) != 1 and rd.lib.rdamd_errno() == 64
    assert call(4, where=3) != 1 and rd.lib.rdamd_errno() == 64
    assert call(4) == 1 and rd.lib.rdamd_errno() == 0 and out.max() > 0   # a valid call after the refusals
    # the assemblies refuse as their siblings do
    with pytest.raises(rd.RdamdError, match="index out of range"):
        rd.gradient_from_adjoints(out, M, W, lengths, subst, freqs, [0, 2, 1, 0], pidx, rates, case["w"])
    assert rd.lib.rdamd_errno() == 7
    with pytest.raises(rd.RdamdError, match="index out of range"):
        rd.substitution_counts_from_adjoints(out, lengths, subst, freqs, [0, 2, 1, 0], rates)
    assert rd.lib.rdamd_errno() == 7
    moved = lengths.copy()
    moved[0, 0] = np.nan
    with pytest.raises(rd.RdamdError, match="negative or not finite"):
        rd.substitution_counts_from_adjoints(out, moved, subst, freqs, pidx, rates)
    assert rd.lib.rdamd_errno() == 64
