"""Pins the CPU oracle (oracle/rd_oracle.c) at the state counts the library promises and the suite did
not reach: 3, 7, 21 states, 45 and 46 (either side of what the device's P-matrix kernel fits into
64 KB of LDS), 61 and 64 (codon models; at 64 the all-ones mask is ~0 and a state sits in bit 63).
tests/test_gpu_state_counts.py takes the oracle as its reference there, so it is compared first with
the restatement of tests/util.py: scipy.linalg.expm per (branch, category) and plain pruning in NumPy.

Every alignment fills the table of state masks a non-DNA partition holds -- 64, or 2^K - 1 --:
the plain states, the all-ones mask, pairs and random subsets, several with the highest state's bit
(util.full_table_map), and every one of them stands in a cell.
Limits as in tests/test_oracle_rate_matrices.py: P 1e-13 absolute, lnL 1e-10 relative.
Runs without a GPU."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
from oracle_lib import OraclePartition, orc_gamma_cats
import util

P_TOL = 1e-13
TOL = 1e-10          # relative, per-site lnL and the total
R = 3
STATE_COUNTS = [3, 7, 21, 45, 46, 61, 64]


@pytest.mark.parametrize("K", STATE_COUNTS)
def test_full_code_table_against_scipy_pruning(K):
    rng = np.random.default_rng(1400 + K)
    newick, _ = synth.random_tree(7, rng)
    tree = rd.Tree.from_newick(newick)
    labels = [tree.tip_label(i) for i in range(7)]
    S = 40
    plain, odd, cmap = util.full_table_map(rng, K)
    rl = tree.root_location(3).with_ratio(0.3)
    ops, pmi, brl = tree.generate_operations(rl)
    seqs = util.odd_cells(rng, {l: "".join(rng.choice(list(plain), size=S)) for l in labels}, odd)
    seqs = util.place_characters(rng, seqs, plain, odd, util.tip_tip_pair(tree, ops), late=min(len(odd) // 2, 16))

    # the cells hold every mask of the map, the table is full, and the highest state's bit is in several
    codes, table = util.tip_codes(seqs, cmap)
    masks = {int(cmap[ord(ch)]) for ch in plain + odd}
    assert set(table) == masks and len(table) == min(64, 2 ** K - 1)
    full = (1 << K) - 1
    assert full in table and all(0 < m <= full for m in table)
    assert (full == 0xFFFFFFFFFFFFFFFF) == (K == 64)
    assert sum(1 for m in table if m >> (K - 1) and m & (m - 1)) >= 3
    assert 0.05 < np.mean([ch in odd for s in seqs.values() for ch in s]) < 0.4

    pattern_weights = rng.integers(1, 4, size=S).astype(np.uint32)
    subst, freqs = util.mixture_params(rng, K, 1)
    rates, cat_weights = orc_gamma_cats(0.7, R), rng.dirichlet(np.ones(R) * 3)
    assert np.ptp(cat_weights) > 0.05

    b = tree.branch_count()
    part = OraclePartition(7, b, K, S, 1, b, R, b)
    util.load_tips(part, tree, seqs, cmap, pattern_weights)
    util.set_mixture((part,), subst, freqs, rates, cat_weights)
    part.update_prob_matrices(pmi, brl)
    part.update_clvs(ops)
    got, got_sites = part.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)

    zero = [0] * R
    want_p = util.restated_pmatrices(subst, freqs, zero, rates, brl)
    have_p = np.array([part.get_pmatrix(int(m)) for m in pmi])
    pmat_of = {int(m): want_p[k] for k, m in enumerate(pmi)}
    want_sites = util.restated_site_lnls(tree, ops, pmat_of, seqs, cmap, K, freqs, zero, cat_weights, pattern_weights)
    assert part.get_scaler(tree.root_scaler_index()).max() == 0
    worst = np.max(np.abs(got_sites - want_sites) / np.abs(want_sites))
    print("K %d: P %.2e, per-site lnL %.2e, total %.2e" % (K, np.max(np.abs(have_p - want_p)), worst,
                                                          util.rel_err(got, want_sites.sum())))
    assert np.max(np.abs(have_p - want_p)) <= P_TOL
    assert worst <= TOL
    assert util.rel_err(got, float(np.sum(want_sites))) <= TOL
    part.destroy()


@pytest.mark.parametrize("K", STATE_COUNTS)
def test_pmatrices_at_the_branch_lengths_of_the_device_test(K):
    """0, 1e-8, 1e-6, 0.37 and 25 with two gamma categories against SciPy: what
    tests/test_gpu_state_counts.py's P-matrix cases lean on"""
    rng = np.random.default_rng(1500 + K)
    subst, freqs = util.mixture_params(rng, K, 1)
    rates = orc_gamma_cats(0.6, 2)
    lengths = [0.0, 1e-8, 1e-6, 0.37, 25.0]
    part = OraclePartition(3, 3, K, 1, 1, 5, 2, 3)
    util.set_mixture((part,), subst, freqs, rates, [0.5, 0.5])
    part.update_prob_matrices([4, 0, 3, 1, 2], lengths)
    want = util.restated_pmatrices(subst, freqs, [0, 0], rates, lengths)
    have = np.array([part.get_pmatrix(m) for m in (4, 0, 3, 1, 2)])
    print("K %d: P %.2e" % (K, np.max(np.abs(have - want))))
    assert np.max(np.abs(have - want)) <= P_TOL
    part.destroy()
