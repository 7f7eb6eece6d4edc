"""The NumPy restatement of the pair sums and of the gradient assembled from them
(tests/grad_ref.py) at 20 states against central differences of the CPU oracle's lnL, without a GPU:
test_brlen_reference_k20.py's case (a 6-tip tree, 12 weighted columns of amino acids with one unknown
cell, an UNREST model with 380 random rates and Dirichlet frequencies) with four rate categories of
unequal weight, one inner and one tip-adjacent root.  It is the reference
tests/test_gpu_k20_pair_sums.py holds the 20-state pair-sum consumer to.

Differenced: all 20 frequencies (K independent numbers, as set_frequencies takes them), the 4
category rates, the 4 category weights, and 40 of the 380 substitution rates drawn with a fixed seed
plus the first and the last.  Step and bound are test_grad_reference.py's: 1e-5 and
1e-4 max(1, |g|), differences formed per site and summed with fsum; the identities I1 and I3 hold to
1e-12 of the total weight."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import grad_ref
import util
from oracle_lib import OraclePartition
from test_brlen_reference import STEP, diff1, inner_root, tip_adjacent_root
from test_brlen_reference_k20 import AA, AA_MAP
from test_grad_reference import persite

R = 4


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(620)
    newick, _ = synth.random_tree(6, rng)
    tree = rd.Tree.from_newick(newick)
    labels = [tree.tip_label(i) for i in range(6)]
    seqs = {l: "".join(rng.choice(list(AA), size=12)) for l in labels}
    seqs[labels[2]] = seqs[labels[2]][:5] + "X" + seqs[labels[2]][6:]   # one unknown cell
    weights = rng.integers(1, 6, 12).astype(np.uint32)
    o = OraclePartition.for_tree(tree, 20, 12, R, rd.ATTRIB_NONREV)
    util.load_tips(o, tree, seqs, AA_MAP, weights)
    subst = rng.uniform(0.1, 1.5, 380)
    freqs = rng.dirichlet(np.ones(20) * 4)
    rates = np.array(rd.compute_gamma_cats(0.8, R))
    w = np.array([0.1, 0.2, 0.3, 0.4])
    o.set_subst_params(0, subst)
    o.set_frequencies(0, freqs)
    o.set_category_rates(rates)
    o.set_category_weights(w)
    return tree, seqs, weights, o, subst, freqs, rates, w


@pytest.mark.parametrize("where", ["inner", "tip"])
def test_gradient_equals_central_differences_at_20_states(setup, where):
    tree, seqs, weights, o, subst, freqs, rates, w = setup
    rl = (inner_root(tree) if where == "inner" else tip_adjacent_root(tree)).with_ratio(0.37)
    ops, pmi, brl = tree.generate_operations(rl)
    pmi, brl = list(pmi), np.array(brl, dtype=np.float64)
    if where == "tip":
        assert min(ops[-1].child1_clv_index, ops[-1].child2_clv_index) < tree.tip_count()
    setters = {"subst": lambda v: o.set_subst_params(0, v), "freqs": lambda v: o.set_frequencies(0, v),
               "rates": o.set_category_rates, "weights": o.set_category_weights}
    values = {"subst": subst, "freqs": freqs, "rates": rates, "weights": w}
    drawn = sorted(set([0, 379]) | set(np.random.default_rng(2020).choice(380, 40, replace=False).tolist()))
    assert len(drawn) >= 40 and drawn[0] == 0 and drawn[-1] == 379
    which = {"subst": drawn, "freqs": range(20), "rates": range(R), "weights": range(R)}

    def evaluate():
        o.update_prob_matrices(pmi, brl)
        return persite(o, tree, ops)

    try:
        evaluate()
        pm = brlen_ref.pmatrices(o, ops)
        q = brlen_ref.build_q(subst, freqs)
        assert np.abs(q - q.T).max() > 1e-2   # (UNREST: N^T would show)
        N, M, W = grad_ref.pair_sums(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, AA_MAP, 20), pm,
                                     [freqs] * R, w, weights)
        assert N.shape == (5, 2, R, 20, 20) and M.shape == (R, 20) and W.shape == (R,)
        total, n = float(np.sum(weights)), len(ops)
        worst = max(abs((N[k, c] * pm[m]).sum() - total) for k in range(n)
                    for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])))
        i3a, i3b = abs((M * freqs[None, :]).sum() - total), abs((w * W).sum() - total)
        print("20 states, %s root: I1 %.3e, I3 %.3e %.3e of total weight %g" % (where, worst / total, i3a / total,
                                                                                  i3b / total, total))
        assert worst <= 1e-12 * total and i3a <= 1e-12 * total and i3b <= 1e-12 * total
        assert N.min() >= 0 and M.min() >= 0 and W.min() >= 0

        lengths = grad_ref.branch_lengths(ops, pmi, brl)
        (d_subst, d_freqs, d_rates, d_weights), _ = grad_ref.gradient(N, M, W, lengths, [subst], [freqs], [0] * R, [0] * R,
                                                                      rates, w)
        got = {"subst": d_subst[0], "freqs": d_freqs[0], "rates": d_rates, "weights": d_weights}
        for name in ("subst", "freqs", "rates", "weights"):
            x, worst = values[name], 0.0
            for i in which[name]:
                f = []
                for sign in (1.0, -1.0):
                    v = np.array(x, dtype=np.float64)
                    v[i] += sign * STEP
                    setters[name](v)
                    f.append(evaluate())
                setters[name](x)
                cd = diff1(f[0], f[1], STEP)
                worst = max(worst, abs(got[name][i] - cd) / max(1.0, abs(got[name][i])))
            print("20 states, %s root: %s: largest scaled error %.3e over %d parameters (largest |g| %.3e)" % (
                where, name, worst, len(which[name]), np.abs(got[name]).max()))
            assert worst <= 1e-4
    finally:
        for name in values:
            setters[name](values[name])
