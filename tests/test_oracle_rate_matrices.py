"""Pins the CPU oracle (oracle/rd_oracle.c) where a partition holds SEVERAL rate matrices and every
rate category names its own: params_indices for the P-matrices, freqs_indices -- a different vector --
for the root frequencies.  The GPU tests of tests/test_gpu_rate_matrices.py take the oracle as their
reference there, so it is compared first with the restatement of tests/util.py: Q per matrix as
synth.build_q builds it, scipy.linalg.expm per (branch, category), plain Felsenstein pruning per
category in NumPy (no rescaling: seven tips) and
    lnL = sum_s w_s log sum_r omega_r pi[fidx[r]] . root[s][r].
Limits as in tests/test_oracle_golden.py against SciPy: P 1e-13 absolute, lnL 1e-10 relative.
Runs without a GPU."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
from oracle_lib import OraclePartition, ORC_MAP_NT, orc_gamma_cats
import util
from util import restated_pmatrices, restated_site_lnls

P_TOL = 1e-13
TOL = 1e-10          # relative, per-site lnL and the total
R = 4


@pytest.mark.parametrize("K,M,pidx,fidx", [(4, 3, [2, 0, 2, 1], [1, 1, 0, 2]),
                                           (2, 2, [1, 0, 1, 1], [0, 1, 1, 0]),
                                           (5, 3, [2, 0, 2, 1], [1, 1, 0, 2])])
def test_per_category_indices_against_scipy_pruning(K, M, pidx, fidx):
    rng = np.random.default_rng(700 + K)
    newick, _ = synth.random_tree(7, rng)
    tree = rd.Tree.from_newick(newick)
    labels = [tree.tip_label(i) for i in range(7)]
    S = 40
    if K == 4:
        alphabet, odd, cmap = "ACGT", "RYKMSWBDHVN-", ORC_MAP_NT
    elif K == 2:
        alphabet, odd = "01", "-?"
        cmap = util.make_map(alphabet, {"-": 3, "?": 3})
    else:
        alphabet, odd = synth.AA[:5], "XB-"
        cmap = util.make_map(alphabet, {"X": 31, "-": 31, "B": 0b00110})
    seqs = util.odd_cells(rng, {l: "".join(rng.choice(list(alphabet), size=S)) for l in labels}, odd)
    assert 0.1 < np.mean([ch in odd for s in seqs.values() for ch in s]) < 0.3
    pattern_weights = rng.integers(1, 4, size=S).astype(np.uint32)
    subst, freqs = util.mixture_params(rng, K, M)
    rates, cat_weights = orc_gamma_cats(0.7, R), rng.dirichlet(np.ones(R) * 3)

    b = tree.branch_count()
    part = OraclePartition(7, b, K, S, M, b, R, b)
    util.load_tips(part, tree, seqs, cmap, pattern_weights)
    util.set_mixture((part,), subst, freqs, rates, cat_weights)
    rl = tree.root_location(3).with_ratio(0.3)
    ops, pmi, brl = tree.generate_operations(rl)

    def oracle(p_indices, f_indices):
        part.update_prob_matrices(pmi, brl, p_indices)
        part.update_clvs(ops)
        return part.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), f_indices, persite=True)

    # what an oracle that ignored one of the two vectors, or took one for the other, would return
    zero = [0] * R
    others = [oracle(zero, zero)[0], oracle(pidx, zero)[0], oracle(zero, fidx)[0], oracle(pidx, pidx)[0],
              oracle(fidx, fidx)[0], oracle(fidx, pidx)[0]]
    got, got_sites = oracle(pidx, fidx)
    assert all(util.rel_err(got, x) > 1e-6 for x in others), (got, others)

    want_p = restated_pmatrices(subst, freqs, pidx, rates, brl)
    pmat_of = {}
    for k, m in enumerate(pmi):
        have = part.get_pmatrix(int(m))
        assert np.max(np.abs(have - want_p[k])) <= P_TOL, (int(m), brl[k])
        pmat_of[int(m)] = want_p[k]
    want_sites = restated_site_lnls(tree, ops, pmat_of, seqs, cmap, K, freqs, fidx, cat_weights, pattern_weights)
    assert part.get_scaler(tree.root_scaler_index()).max() == 0
    worst = np.max(np.abs(got_sites - want_sites) / np.abs(want_sites))
    print("K %d: P %.2e, per-site lnL %.2e, total %.2e" % (K, np.max(np.abs(np.array(
        [part.get_pmatrix(int(m)) for m in pmi]) - want_p)), worst, util.rel_err(got, want_sites.sum())))
    assert worst <= TOL
    assert util.rel_err(got, float(np.sum(want_sites))) <= TOL
    part.destroy()


def test_twenty_state_pmatrices_per_category():
    """20 states through P only: three branches, four categories over three rate matrices"""
    K, M, pidx = 20, 3, [2, 0, 2, 1]
    rng = np.random.default_rng(720)
    subst, freqs = util.mixture_params(rng, K, M)
    rates = orc_gamma_cats(0.7, R)
    part = OraclePartition(3, 3, K, 1, M, 3, R, 3)
    util.set_mixture((part,), subst, freqs, rates, [0.25] * R)
    lengths = [1e-6, 0.37, 25.0]
    part.update_prob_matrices([2, 0, 1], lengths, pidx)
    want = restated_pmatrices(subst, freqs, pidx, rates, lengths)
    for k, m in enumerate((2, 0, 1)):
        have = part.get_pmatrix(m)
        assert np.max(np.abs(have - want[k])) <= P_TOL, m
        # the categories that share a rate matrix still differ by their rate, and those that do not share
        # one differ by more than the rates explain
        assert np.max(np.abs(have[0] - have[2])) > 1e-9 or lengths[k] < 1e-5
    part.update_prob_matrices([2, 0, 1], lengths, [0] * R)
    assert np.max(np.abs(part.get_pmatrix(0) - want[1])) > 1e-3
    part.destroy()
