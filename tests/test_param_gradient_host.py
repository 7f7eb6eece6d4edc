"""rdamd_gradient_from_pair_sums (csrc/param_gradient.hpp, host only) against tests/grad_ref.py, without
a GPU, on pair sums made by grad_ref on the 10-taxon tree with P-matrices from scipy.linalg.expm:
K = 4 and K = 2, one rate matrix and two (params_indices [0,1,1,0], freqs_indices [1,1,0,0]), and
branch lengths that include 1e-6, 0.1 and 100, the ends of --brlen-min / --brlen-max.

Both sides evaluate one formula in double precision; they differ in the order of the operations (a
Taylor core with scaling and squaring here, SciPy's Pade there; a closed-form chain rule here, dQ/dx
as matrices there).  The figure compared is |g - g_ref| / C, C the absolute-value companion of the
contraction (grad_ref.gradient).  Measured worst over all cases and parameters: 2.0e-15 (K 4, two
rate matrices, the substitution rates); TOL is 100 times that.

Also the stand-alone program tests/cpp/param_gradient_check.cpp (F(X, E) for diagonal X against
the closed form, F(X, X) = X exp(X) and F(X, I) = exp(X) for commuting arguments), built plainly
and as an AddressSanitizer + UBSan program."""
import os
import subprocess

import numpy as np
import pytest
from scipy.linalg import expm

import root_digger_amd as rd
import brlen_ref
import grad_ref
import util

TOL = 100 * 2.0e-15
SRC = os.path.join(util.ROOT, "tests", "cpp", "param_gradient_check.cpp")
INCLUDES = ["-I", os.path.join(util.ROOT, "root_digger_amd", "csrc")]


def make_case(K, sets, rng):
    tree = rd.Tree.from_file(os.path.join(util.DATA, "10.tree"))
    rl = next(r for r in tree.roots() if 2 <= len(tree.side_tips(r)) <= tree.tip_count() - 2).with_ratio(0.3)
    ops, pmi, brl = tree.generate_operations(rl)
    pmi, brl = [int(m) for m in pmi], np.array(brl, dtype=np.float64)
    brl[[1, 5, 11]] = (1e-6, 0.1, 100.0)
    R, S = 4, 41
    pidx, fidx = ([0, 1, 1, 0], [1, 1, 0, 0]) if sets == 2 else ([0] * R, [0] * R)
    subst = [rng.uniform(0.1, 1.5, K * K - K) for _ in range(sets)]
    freqs = [rng.dirichlet(np.ones(K) * 4) for _ in range(sets)]
    rates = np.array(rd.compute_gamma_cats(0.7, R))
    w = rng.dirichlet(np.ones(R) * 3)
    weights = rng.integers(0, 4, S).astype(np.float64)
    q = [brlen_ref.build_q(subst[m], freqs[m]) for m in range(sets)]
    pmat = {m: np.array([expm(q[pidx[r]] * rates[r] * t) for r in range(R)]) for m, t in zip(pmi, brl)}
    # 0/1 code vectors with ambiguity: any non-empty subset of the states
    tipvec = {i: np.array([[(c >> j) & 1 for j in range(K)] for c in rng.integers(1, 2 ** K, S)], dtype=np.float64)
              for i in range(tree.tip_count())}
    N, M, W = grad_ref.pair_sums(ops, tree.tip_count(), tipvec, pmat, [freqs[m] for m in fidx], w, weights)
    lengths = grad_ref.branch_lengths(ops, pmi, brl)
    assert {1e-6, 0.1, 100.0} <= set(lengths.ravel())
    return N, M, W, lengths, subst, freqs, pidx, fidx, rates, w


@pytest.mark.parametrize("K,sets", [(4, 1), (4, 2), (2, 1), (2, 2)])
def test_host_gradient_equals_the_restatement(K, sets):
    rng = np.random.default_rng(10 * K + sets)
    N, M, W, lengths, subst, freqs, pidx, fidx, rates, w = make_case(K, sets, rng)
    want, comp = grad_ref.gradient(N, M, W, lengths, subst, freqs, pidx, fidx, rates, w)
    got = rd.gradient_from_pair_sums(N, M, W, lengths, subst, freqs, pidx, fidx, rates, w)
    for name, g, ref, C in zip(("subst", "freqs", "rates", "weights"), got, want, comp):
        assert g.shape == ref.shape and np.all(np.isfinite(g))
        ratio = np.abs(g - ref) / C
        print("K %d, %d rate matrices, %s: largest |g - g_ref| / C %.3e (largest |g| %.3e)" % (
            K, sets, name, ratio.max(), np.abs(ref).max()))
        assert np.all(np.abs(g - ref) <= TOL * C)
    assert got[3].tobytes() == np.asarray(W).tobytes()
    # a pure function: the same again
    again = rd.gradient_from_pair_sums(N, M, W, lengths, subst, freqs, pidx, fidx, rates, w)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_refusals():
    rng = np.random.default_rng(1)
    N, M, W, lengths, subst, freqs, pidx, fidx, rates, w = make_case(4, 2, rng)
    with pytest.raises(rd.RdamdError, match="index out of range"):
        rd.gradient_from_pair_sums(N, M, W, lengths, subst, freqs, [0, 2, 1, 0], fidx, rates, w)
    assert rd.lib.rdamd_errno() == 7
    assert rd.lib.rdamd_gradient_from_pair_sums(4, 4, 2, len(N), None, None, None, None, None, None, None, None, None, None,
                                                None, None, None, None) != 1
    assert rd.lib.rdamd_errno() == 64


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_block_exponential_against_closed_forms(tmp_path, flags):
    exe = str(tmp_path / "param_gradient_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + INCLUDES + [SRC, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("param gradient OK"), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[-1]) > 1000
