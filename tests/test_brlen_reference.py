"""The NumPy restatement of the branch-length derivatives (tests/brlen_ref.py) against central
differences of the CPU oracle's lnL, without a GPU: 10.tree / 10.fasta compressed to weighted
patterns, UNREST + four gamma categories, one inner and one tip-adjacent root.

Tolerances are those of the trial the definitions were checked with (step 1e-5): first derivatives
within 1e-4 max(1, |d1|), second derivatives within 2e-2 max(1, |d2|).  The same first-derivative
bound serves the identity d lnL / d alpha = T (d1 of the root child that gets alpha T - d1 of the
other): it is a central difference of the same lnL with the same step, in a variable whose unit
is T branch-length units."""
import math
import os

import numpy as np
import pytest

import root_digger_amd as rd
import brlen_ref
import util
from oracle_lib import OraclePartition, ORC_MAP_NT

STEP = 1e-5
SUBST = [.34, .42, .24, .74, .16, .88, .75, .54, .20, .06, .08, .41]


@pytest.fixture(scope="module")
def setup():
    tree = rd.Tree.from_file(os.path.join(util.DATA, "10.tree"))
    seqs, weights = util.compress(util.read_fasta(os.path.join(util.DATA, "10.fasta")))
    assert weights.max() > 1
    S = len(weights)
    o = OraclePartition.for_tree(tree, 4, S, 4, rd.ATTRIB_NONREV)
    util.load_tips(o, tree, seqs, ORC_MAP_NT, weights)
    freqs = np.array(o.empirical_frequencies())
    rates = np.array(rd.compute_gamma_cats(0.8, 4))
    w = np.array([0.1, 0.2, 0.3, 0.4])
    o.set_subst_params(0, SUBST)
    o.set_frequencies(0, freqs)
    o.set_category_rates(rates)
    o.set_category_weights(w)
    return tree, seqs, weights, o, freqs, rates, w


def lnl_at(o, tree, ops, pmi, brl):
    """the oracle's per-site terms of lnL (their sum is its lnL): differences are formed per site and
    summed exactly, so the rounding of a total of 1e4 (2e-12, 0.2 in a second difference with step 1e-5)
    does not enter"""
    o.update_prob_matrices(pmi, brl)
    o.update_clvs(ops)
    total, persite = o.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)
    assert abs(math.fsum(persite) - total) <= 1e-12 * abs(total)
    return persite


def diff1(fu, fd, step):
    return math.fsum(fu - fd) / (2 * step)


def diff2(fu, f, fd, step):
    return math.fsum((fu - f) + (fd - f)) / step ** 2


def tip_adjacent_root(tree):
    for rl in tree.roots():
        if len(tree.side_tips(rl)) == 1 or len(tree.side_tips(rl)) == tree.tip_count() - 1:
            return rl
    raise AssertionError("no tip branch")


def inner_root(tree):
    for rl in tree.roots():
        if 2 <= len(tree.side_tips(rl)) <= tree.tip_count() - 2:
            return rl
    raise AssertionError("no inner branch")


@pytest.mark.parametrize("where", ["inner", "tip"])
def test_restatement_equals_central_differences(setup, where):
    tree, seqs, weights, o, freqs, rates, w = setup
    rl = (inner_root(tree) if where == "inner" else tip_adjacent_root(tree)).with_ratio(0.37)
    ops, pmi, brl = tree.generate_operations(rl)
    pmi, brl = list(pmi), np.array(brl, dtype=np.float64)
    n = len(ops)
    if where == "tip":
        assert min(ops[-1].child1_clv_index, ops[-1].child2_clv_index) < tree.tip_count()
    base = lnl_at(o, tree, ops, pmi, brl)
    pmat = brlen_ref.pmatrices(o, ops)
    q = brlen_ref.build_q(SUBST, freqs)
    assert np.abs(q - o.get_qmatrix(0)).max() < 1e-14
    d1, d2, _, _ = brlen_ref.branch_derivatives(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, ORC_MAP_NT, 4),
                                                pmat, [q] * 4, [freqs] * 4, w, rates, weights)
    place = {m: i for i, m in enumerate(pmi)}
    worst1 = worst2 = 0.0
    for k in range(n):
        for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
            up, down = brl.copy(), brl.copy()
            up[place[m]] += STEP
            down[place[m]] -= STEP
            fu, fd = lnl_at(o, tree, ops, pmi, up), lnl_at(o, tree, ops, pmi, down)
            e1 = abs(d1[k, c] - diff1(fu, fd, STEP)) / max(1.0, abs(d1[k, c]))
            e2 = abs(d2[k, c] - diff2(fu, base, fd, STEP)) / max(1.0, abs(d2[k, c]))
            worst1, worst2 = max(worst1, e1), max(worst2, e2)
    print("%s root: largest scaled error d1 %.3e, d2 %.3e over %d branches" % (where, worst1, worst2, 2 * n))
    assert worst1 <= 1e-4
    assert worst2 <= 2e-2

    # d lnL / d alpha = T (d1 of the root child that gets alpha T - d1 of the other)
    lengths = [brl[place[m]] for _, m in brlen_ref.children_of(ops[-1])]
    T = lengths[0] + lengths[1]
    near = 0 if abs(lengths[0] - 0.37 * T) < abs(lengths[1] - 0.37 * T) else 1
    assert abs(lengths[near] - 0.37 * T) < 1e-12 * max(1.0, T)
    want = T * (d1[0, near] - d1[0, 1 - near])
    f = []
    for alpha in (0.37 + STEP, 0.37 - STEP):
        ops_a, pmi_a, brl_a = tree.generate_operations(rl.with_ratio(alpha))
        f.append(lnl_at(o, tree, ops_a, pmi_a, brl_a))
    got = diff1(f[0], f[1], STEP)
    print("%s root: d lnL / d alpha %.9f, central difference %.9f" % (where, want, got))
    assert abs(want - got) <= 1e-4 * max(1.0, abs(want))
