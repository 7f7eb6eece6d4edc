"""The NumPy restatement of the pair sums and of the gradient assembled from them
(tests/grad_ref.py) against central differences of the CPU oracle's lnL, without a GPU: 10.tree /
10.fasta compressed to weighted patterns, UNREST + four categories, one inner and one tip-adjacent
root; all 12 substitution rates, 4 frequencies (K independent numbers, as set_frequencies takes
them), 4 category rates and 4 category weights.

The bound is test_brlen_reference.py's for a first central difference of the same lnL at the same
step (1e-5): 1e-4 max(1, |g|).  Differences are formed per site and summed with fsum, as there.
The identities I1 and I3 of the header hold to 1e-12 of the total weight."""
import math

import numpy as np
import pytest

import brlen_ref
import grad_ref
from oracle_lib import ORC_MAP_NT
from test_brlen_reference import STEP, SUBST, diff1, inner_root, setup, tip_adjacent_root  # noqa: F401  (setup: fixture)


def persite(o, tree, ops):
    o.update_clvs(ops)
    total, sites = o.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)
    assert abs(math.fsum(sites) - total) <= 1e-12 * abs(total)
    return sites


@pytest.mark.parametrize("where", ["inner", "tip"])
def test_gradient_equals_central_differences(setup, where):
    tree, seqs, weights, o, freqs, rates, w = setup
    rl = (inner_root(tree) if where == "inner" else tip_adjacent_root(tree)).with_ratio(0.37)
    ops, pmi, brl = tree.generate_operations(rl)
    pmi, brl = list(pmi), np.array(brl, dtype=np.float64)
    if where == "tip":
        assert min(ops[-1].child1_clv_index, ops[-1].child2_clv_index) < tree.tip_count()
    subst = np.array(SUBST)
    setters = {"subst": lambda v: o.set_subst_params(0, v), "freqs": lambda v: o.set_frequencies(0, v),
               "rates": o.set_category_rates, "weights": o.set_category_weights}
    values = {"subst": subst, "freqs": freqs, "rates": rates, "weights": w}

    def evaluate():
        o.update_prob_matrices(pmi, brl)
        return persite(o, tree, ops)

    try:
        evaluate()
        N, M, W = grad_ref.pair_sums(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, ORC_MAP_NT, 4),
                                     brlen_ref.pmatrices(o, ops), [freqs] * 4, w, weights)
        total = float(np.sum(weights))
        # I1, I3
        pm = brlen_ref.pmatrices(o, ops)
        n = len(ops)
        worst = 0.0
        for k in range(n):
            for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
                worst = max(worst, abs((N[k, c] * pm[m]).sum() - total))
        i3a, i3b = abs((M * freqs[None, :]).sum() - total), abs((w * W).sum() - total)
        print("%s root: I1 %.3e, I3 %.3e %.3e of total weight %g" % (where, worst / total, i3a / total, i3b / total, total))
        assert worst <= 1e-12 * total and i3a <= 1e-12 * total and i3b <= 1e-12 * total
        assert N.min() >= 0 and M.min() >= 0 and W.min() >= 0

        lengths = grad_ref.branch_lengths(ops, pmi, brl)
        (d_subst, d_freqs, d_rates, d_weights), _ = grad_ref.gradient(N, M, W, lengths, [subst], [freqs], [0] * 4, [0] * 4,
                                                                      rates, w)
        got = {"subst": d_subst[0], "freqs": d_freqs[0], "rates": d_rates, "weights": d_weights}
        for name in ("subst", "freqs", "rates", "weights"):
            x, worst = values[name], 0.0
            for i in range(len(x)):
                f = []
                for sign in (1.0, -1.0):
                    v = np.array(x, dtype=np.float64)
                    v[i] += sign * STEP
                    setters[name](v)
                    f.append(evaluate())
                setters[name](x)
                cd = diff1(f[0], f[1], STEP)
                worst = max(worst, abs(got[name][i] - cd) / max(1.0, abs(got[name][i])))
            print("%s root: %s: largest scaled error %.3e over %d parameters (largest |g| %.3e)" % (
                where, name, worst, len(x), np.abs(got[name]).max()))
            assert worst <= 1e-4
    finally:
        for name in values:
            setters[name](values[name])
