"""The NumPy restatement of the branch-length derivatives (tests/brlen_ref.py) at 20 states against
central differences of the CPU oracle's lnL, without a GPU: a 6-tip tree, 12 weighted columns of
amino acids, an UNREST model with 380 random rates, Dirichlet frequencies and two rate categories,
one inner and one tip-adjacent root.  It is the reference tests/test_gpu_k20_brlen.py holds the
20-state derivative consumer to.

Step and tolerances are those of tests/test_brlen_reference.py (step 1e-5): first derivatives within
1e-4 max(1, |d1|), second derivatives within 2e-2 max(1, |d2|), and the first-derivative bound for
the identity d lnL / d alpha = T (d1 of the root child that gets alpha T - d1 of the other)."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import util
from oracle_lib import OraclePartition
from test_brlen_reference import STEP, lnl_at, diff1, diff2, tip_adjacent_root, inner_root

AA = synth.AA
AA_MAP = util.make_map(AA, {"-": (1 << 20) - 1, "X": (1 << 20) - 1})


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(620)
    newick, _ = synth.random_tree(6, rng)
    tree = rd.Tree.from_newick(newick)
    labels = [tree.tip_label(i) for i in range(6)]
    seqs = {l: "".join(rng.choice(list(AA), size=12)) for l in labels}
    seqs[labels[2]] = seqs[labels[2]][:5] + "X" + seqs[labels[2]][6:]   # one unknown cell
    weights = rng.integers(1, 6, 12).astype(np.uint32)
    o = OraclePartition.for_tree(tree, 20, 12, 2, rd.ATTRIB_NONREV)
    util.load_tips(o, tree, seqs, AA_MAP, weights)
    subst = rng.uniform(0.1, 1.5, 380)
    freqs = rng.dirichlet(np.ones(20) * 4)
    rates = np.array(rd.compute_gamma_cats(0.8, 2))
    w = np.array([0.35, 0.65])
    o.set_subst_params(0, subst)
    o.set_frequencies(0, freqs)
    o.set_category_rates(rates)
    o.set_category_weights(w)
    return tree, seqs, weights, o, subst, freqs, rates, w


@pytest.mark.parametrize("where", ["inner", "tip"])
def test_restatement_equals_central_differences_at_20_states(setup, where):
    tree, seqs, weights, o, subst, freqs, rates, w = setup
    rl = (inner_root(tree) if where == "inner" else tip_adjacent_root(tree)).with_ratio(0.37)
    ops, pmi, brl = tree.generate_operations(rl)
    pmi, brl = list(pmi), np.array(brl, dtype=np.float64)
    n = len(ops)
    assert n == 5
    if where == "tip":
        assert min(ops[-1].child1_clv_index, ops[-1].child2_clv_index) < tree.tip_count()
    base = lnl_at(o, tree, ops, pmi, brl)
    pmat = brlen_ref.pmatrices(o, ops)
    q = brlen_ref.build_q(subst, freqs)
    assert np.abs(q - o.get_qmatrix(0)).max() < 1e-14
    assert np.abs(q - q.T).max() > 1e-2   # (UNREST: a transposed product would show)
    d1, d2, _, _ = brlen_ref.branch_derivatives(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, AA_MAP, 20),
                                                pmat, [q] * 2, [freqs] * 2, w, rates, weights)
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
    print("20 states, %s root: largest scaled error d1 %.3e, d2 %.3e over %d branches" % (where, worst1, worst2, 2 * n))
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
    print("20 states, %s root: d lnL / d alpha %.9f, central difference %.9f" % (where, want, got))
    assert abs(want - got) <= 1e-4 * max(1.0, abs(want))
