"""tests/subst_ref.py, the restatement of the substitution mapping, checked without a GPU against
things that are not restatements of it:

  J      exact enumeration over every assignment of states to the inner nodes of a 5- and a 6-tip
         tree (R = 2, K = 4 and K = 2), no recursion and no renormalisation, at 1e-12;
  E      E[i][j] = X[i][j] dlnL/dX[i][j]: with one rate matrix, sum_r X_r[i][j] dlnL/dX_r[i][j] =
         Q[i][j] dlnL/dQ[i][j] for the branch's own copy of Q.  The derivative is a central difference
         (step 1e-4) of the NumPy lnL with that one branch's matrices replaced by
         expm(rho_r tau (Q + h e_i e_j^T)), at 1e-6 relative;
  A - D  the four identities of the header at 1e-11 of the sums' companions (all terms of A, B and
         D are non-negative; C has the negative diagonal of X, its companion takes |X[i][i]|)."""
import itertools
import math

import numpy as np
import pytest
from scipy.linalg import expm

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import grad_ref
import subst_ref

FIVE = "((a:0.21,b:0.09):0.13,c:0.4,(d:0.05,e:0.33):0.27);"
SIX = "((a:0.21,b:0.09):0.13,(c:0.4,f:0.02):0.6,(d:0.05,e:0.33):0.27);"


def make_case(tree, rl, K, R, S, rng, sets=1, pidx=None, brl_set=None):
    """a rooted tree with random UNREST matrices, 0/1 code vectors with ambiguity and pattern weights"""
    ops, pmi, brl = tree.generate_operations(rl)
    pmi, brl = [int(m) for m in pmi], np.array(brl, dtype=np.float64)
    for at, value in (brl_set or {}).items():
        brl[at] = value
    pidx = [0] * R if pidx is None else pidx
    subst = [rng.uniform(0.1, 1.5, K * K - K) for _ in range(sets)]
    freqs = [rng.dirichlet(np.ones(K) * 4) for _ in range(sets)]
    rates = np.array(rd.compute_gamma_cats(0.7, R)) if R > 1 else np.ones(1)
    w = rng.dirichlet(np.ones(R) * 3)
    weights = rng.integers(0, 4, S).astype(np.float64)
    weights[0] = 2
    q = [brlen_ref.build_q(subst[m], freqs[m]) for m in range(sets)]
    qs = [q[m] for m in pidx]
    pmat = subst_ref.pmatrices_from_q(pmi, brl, qs, rates)
    tipvec = {i: np.array([[(c >> j) & 1 for j in range(K)] for c in rng.integers(1, 2 ** K, S)], dtype=np.float64)
              for i in range(tree.tip_count())}
    lengths = grad_ref.branch_lengths(ops, pmi, brl)
    return dict(ops=ops, pmi=pmi, brl=brl, tips=tree.tip_count(), subst=subst, freqs=freqs, rates=rates, w=w, weights=weights,
                qs=qs, pidx=pidx, pis=[freqs[m] for m in pidx], pmat=pmat, tipvec=tipvec, lengths=lengths, K=K, R=R, S=S)


def maps_of(case):
    cmat = subst_ref.count_matrices(case["lengths"], case["qs"], case["rates"])
    return subst_ref.site_maps(case["ops"], case["tips"], case["tipvec"], case["pmat"], cmat, case["pis"], case["w"])


def enumerate_joint(case):
    """J[n][2][S][K][K] by brute force: every assignment of states to the inner nodes, per rate"""
    ops, tips, K, R, S = case["ops"], case["tips"], case["K"], case["R"], case["S"]
    n = len(ops)
    inner = [o.parent_clv_index for o in ops]
    J = np.zeros((n, 2, S, K, K))
    total = np.zeros(S)
    for r in range(R):
        for states in itertools.product(range(K), repeat=n):
            at = dict(zip(inner, states))
            root = ops[-1].parent_clv_index
            prob = np.full(S, case["w"][r] * case["pis"][r][at[root]])
            for o in ops:
                i = at[o.parent_clv_index]
                for child, m in brlen_ref.children_of(o):
                    row = case["pmat"][m][r][i]
                    prob = prob * (row[at[child]] if child >= tips else case["tipvec"][child] @ row)
            total += prob
            for k in range(n):
                o = ops[n - 1 - k]
                i = at[o.parent_clv_index]
                for c, (child, m) in enumerate(brlen_ref.children_of(o)):
                    if child >= tips:
                        J[k, c, :, i, at[child]] += prob
                    else:   # the tip's end state is any state its code allows, in proportion
                        row = case["pmat"][m][r][i] * case["tipvec"][child]
                        J[k, c, :, i, :] += prob[:, None] * row / row.sum(axis=1, keepdims=True)
    return J / total[None, None, :, None, None]


@pytest.mark.parametrize("newick,K", [(FIVE, 4), (SIX, 4), (FIVE, 2), (SIX, 2)], ids=["5-K4", "6-K4", "5-K2", "6-K2"])
def test_joint_equals_the_exact_enumeration(newick, K):
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(10 * K + tree.tip_count())
    case = make_case(tree, tree.root_location(1).with_ratio(0.3), K, 2, 9, rng)
    J, _ = maps_of(case)
    want = enumerate_joint(case)
    print("%d tips K %d: largest |J - J_enum| %.3e" % (tree.tip_count(), K, np.abs(J - want).max()))
    assert np.abs(J - want).max() <= 1e-12
    assert np.abs(J.sum(axis=(3, 4)) - 1.0).max() <= 1e-12


def ten(rng, K=4, R=4, S=41, **kw):
    newick, _ = synth.random_tree(10, rng)
    tree = rd.Tree.from_newick(newick)
    return make_case(tree, tree.root_location(5).with_ratio(0.3), K, R, S, rng, **kw)


def test_typed_counts_are_x_times_the_derivative_in_x():
    rng = np.random.default_rng(3)
    case = ten(rng, S=23)
    ops, n, K, R = case["ops"], len(case["ops"]), 4, 4
    N, _, _ = grad_ref.pair_sums(ops, case["tips"], case["tipvec"], case["pmat"], case["pis"], case["w"], case["weights"])
    typed, _, _, _ = subst_ref.typed_counts(N, case["lengths"], case["qs"], case["rates"])
    q, h, worst = case["qs"][0], 1e-4, 0.0

    def site_lnls(pmat):
        return np.log(subst_ref.site_likelihoods(ops, case["tips"], case["tipvec"], pmat, case["pis"], case["w"]))

    for k, c in ((0, 0), (0, 1), (3, 0), (n - 1, 1)):   # both root branches, an inner one, a tip branch
        m = brlen_ref.children_of(ops[n - 1 - k])[c][1]
        tau = case["lengths"][k][c]
        for i in range(K):
            for j in range(K):
                if i == j:
                    continue
                f = []
                for sign in (1.0, -1.0):
                    moved = q.copy()
                    moved[i, j] += sign * h
                    pm = dict(case["pmat"])
                    pm[m] = np.array([expm(case["rates"][r] * tau * moved) for r in range(R)])
                    f.append(site_lnls(pm))
                cd = math.fsum(case["weights"] * (f[0] - f[1])) / (2 * h)
                worst = max(worst, abs(typed[k, c, i, j] - q[i, j] * cd) / abs(typed[k, c, i, j]))
    print("largest |E - X dlnL/dX| / E %.3e" % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("K,R,sets", [(4, 4, 1), (4, 4, 2), (2, 4, 1), (4, 1, 1), (4, 3, 1)])
def test_identities(K, R, sets):
    rng = np.random.default_rng(100 * K + 10 * R + sets)
    pidx = [0, 1, 1, 0][:R] if sets == 2 else None
    case = ten(rng, K=K, R=R, sets=sets, pidx=pidx, brl_set={2: 0.0, 7: 3.0})
    ops, n = case["ops"], len(case["ops"])
    weights, total = case["weights"], case["weights"].sum()
    N, _, _ = grad_ref.pair_sums(ops, case["tips"], case["tipvec"], case["pmat"], case["pis"], case["w"], weights)
    typed, comp, diag, diag_comp = subst_ref.typed_counts(N, case["lengths"], case["qs"], case["rates"])
    J, cnt = maps_of(case)
    d1, _, _, _ = brlen_ref.branch_derivatives(ops, case["tips"], case["tipvec"], case["pmat"], case["qs"], case["pis"],
                                               case["w"], case["rates"], weights)
    off = ~np.eye(K, dtype=bool)
    worst = [0.0] * 4
    for k in range(n):
        for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
            tau = case["lengths"][k][c]
            e_sum = typed[k, c][off].sum()
            a = abs((weights * cnt[k, c]).sum() - e_sum)
            assert a <= 1e-11 * max(e_sum, 1e-300) or (tau == 0.0 and a == 0.0)
            b = np.abs(np.einsum("s,sij->ij", weights, J[k, c]) - (N[k, c] * case["pmat"][m]).sum(axis=0)).max()
            assert b <= 1e-11 * total
            cc = abs(tau * d1[k, c] - (e_sum + diag[k, c]))
            assert cc <= 1e-11 * (e_sum + diag_comp[k, c]) or (tau == 0.0 and cc == 0.0)
            d = abs(np.diag(typed[k, c]).sum() - tau * total)
            assert d <= 1e-11 * tau * total
            if tau > 0:
                worst = [max(x, y) for x, y in zip(worst, (a / e_sum, b / total, cc / (e_sum + diag_comp[k, c]), d / (tau * total)))]
    print("K %d R %d sets %d: A %.3e B %.3e C %.3e D %.3e (relative to the companions)" % ((K, R, sets) + tuple(worst)))
    assert 0.0 in case["lengths"] and 3.0 in case["lengths"]
