"""Model.site_lnls / Model.site_patterns (rdamd_model_site_lnls): the unweighted per-pattern
log-likelihoods of a list of roots, each at its own parameters, against the CPU oracle's
per-site output; and what the call must leave untouched."""
import os

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
from oracle_lib import OraclePartition, ORC_MAP_NT
import util

pytestmark = pytest.mark.gpu
LNL_TOL = 1e-11   # the parity suite's (tests/test_gpu_configs.py)


def random_param_sets(rng, n, states, cats=1, partitions=1):
    """n parameter sets in the checkpoint's layout (unnormalised frequencies, as the optimiser
    leaves them)"""
    return [[{"subst_rates": rng.uniform(0.05, 1.0, states * states - states).tolist(),
              "freqs": rng.uniform(0.2, 1.0, states).tolist(),
              "gamma_alpha": [float(rng.uniform(0.3, 3.0))], "gamma_weights": []}
             for _ in range(partitions)] for _ in range(n)]


def oracle_rows(tree, seqs, cmap, states, cats, rls, param_sets):
    """the oracle's per-site lnL (unit pattern weights) of every root at its parameters, applied
    as model_t::set_model_params applies them: normalised frequencies, MEDIAN gamma rates"""
    sites = len(next(iter(seqs.values())))
    o = OraclePartition.for_tree(tree, states, sites, cats)
    util.load_tips(o, tree, seqs, cmap)
    rows = []
    for rl, pp in zip(rls, param_sets):
        f = np.asarray(pp["freqs"], dtype=np.float64)
        o.set_subst_params(0, pp["subst_rates"])
        o.set_frequencies(0, (f / f.sum()).tolist())
        if cats > 1:
            o.set_category_rates(rd.compute_gamma_cats(pp["gamma_alpha"][0], cats, rd.GAMMA_RATES_MEDIAN))
        ops, pmi, brl = tree.generate_operations(rl)
        o.update_prob_matrices(pmi, brl)
        o.update_clvs(ops)
        rows.append(o.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)[1])
    return np.array(rows)


def assert_rows(got, want, what):
    """LNL_TOL relative on every entry.  A site lnL is log(L): where |lnL| < 1 the bound is taken on
    the likelihood L itself, LNL_TOL relative in L = LNL_TOL absolute in lnL -- a column of gaps has
    L = 1 and lnL = 0 exactly, and what both sides compute there (-2e-15) is the rounding of L alone,
    of which no relative statement in lnL can be made."""
    err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))
    print("%s: %d x %d entries, largest relative error %.3e" % (what, got.shape[0], got.shape[1], err))
    assert got.shape == want.shape
    assert err < LNL_TOL


def check_single_partition(make_tree, seqs, cmap, orc_map, states, cats, root_ids, seed):
    """oracle parity with per-root parameters, weights . row against compute_lh, and the state the
    call leaves behind"""
    tree, t2 = make_tree(), make_tree()
    packed, weights = util.compress(seqs)
    m = rd.Model(tree, packed, states=states, cmap=cmap, rate_cats=cats, weights=weights, seed=3)
    m.initialize_partitions()
    w, pattern_of = m.site_patterns()
    assert np.array_equal(w, weights) and len(pattern_of) == int(weights.sum())
    assert np.array_equal(np.bincount(pattern_of, minlength=len(w)), w)
    rng = np.random.default_rng(seed)
    rls = [tree.root_location(i).with_ratio(float(rng.uniform(0.05, 0.95))) for i in root_ids]
    sets = random_param_sets(rng, len(rls), states, cats)

    home = tree.root_location(root_ids[0]).with_ratio(0.4)
    lh_before = m.compute_lh(home)
    root_before = m.compute_lh_root(home)
    freqs_before = m.partition_frequencies(0)

    got = m.site_lnls(rls, sets)
    assert_rows(got, oracle_rows(t2, packed, orc_map, states, cats, rls, [s[0] for s in sets]),
                "%d states, %d categories, own parameters" % (states, cats))
    # nothing moved: parameters, the rooting and its conditional likelihoods, the next evaluation
    assert np.array_equal(m.partition_frequencies(0), freqs_before)
    assert m.compute_lh_root(home) == root_before
    assert m.compute_lh(home) == lh_before
    # the model's current parameters (NULL), and the totals compute_lh gives at the same point
    cur = m.site_lnls(rls)
    for rl, row in zip(rls, cur):
        assert util.rel_err(float(np.dot(weights.astype(np.float64), row)), m.compute_lh(rl)) < LNL_TOL
    # ... and at a root's own parameters, set through the model's setters
    for k in (0, len(rls) - 1):
        pp = sets[k][0]
        f = np.asarray(pp["freqs"])
        m.set_subst_rates(pp["subst_rates"])
        m.set_freqs((f / f.sum()).tolist())
        m.set_gamma_alpha(pp["gamma_alpha"][0])
        assert util.rel_err(float(np.dot(weights.astype(np.float64), got[k])), m.compute_lh(rls[k])) < LNL_TOL
    return got, weights


@pytest.mark.parametrize("cats", [1, 4])
def test_site_lnls_ten_taxa_all_roots(cats):
    path = os.path.join(util.DATA, "10.tree")
    seqs = util.read_fasta(os.path.join(util.DATA, "10.fasta"))
    got, weights = check_single_partition(lambda: rd.Tree.from_file(path), seqs, rd.MAP_NT, ORC_MAP_NT, 4, cats,
                                          list(range(17)), 11 + cats)
    assert got.shape == (17, 991) and int(weights.sum()) == 1000


def test_site_lnls_hundred_taxa_five_parameter_sets():
    w = synth.workload(100, 2000, 4, 4, 77)
    check_single_partition(lambda: rd.Tree.from_newick(w["newick"]), w["seqs"], rd.MAP_NT, ORC_MAP_NT, 4, 4,
                           [0, 41, 97, 150, 196], 5)


def test_site_lnls_twenty_states():
    w = synth.workload(12, 300, 20, 4, 78)
    cmap = util.make_map(w["alphabet"])
    check_single_partition(lambda: rd.Tree.from_newick(w["newick"]), w["seqs"], cmap, cmap, 20, 4, [0, 7, 13, 20], 6)


def test_site_lnls_two_partitions(tmp_path):
    phy, tre = os.path.join(util.DATA, "101.phy"), os.path.join(util.DATA, "101.tree")
    lines = ["UNREST+G4, first = 1-300", "UNREST, second = 301-700, 900-1000"]
    pf = tmp_path / "parts.txt"
    pf.write_text("\n".join(lines) + "\n")
    tree, t2 = rd.Tree.from_file(tre), rd.Tree.from_file(tre)
    m = rd.Model.from_partition_file(tree, phy, str(pf), seed=3)
    m.initialize_partitions()
    weights, pattern_of = m.site_patterns()
    compressed, w_file, po_file = rd.msa_pattern_probe(phy, lines)
    assert np.array_equal(weights, w_file) and np.array_equal(pattern_of, po_file)
    assert len(pattern_of) == 300 + 400 + 101
    names = list(util.read_phylip(phy))
    sizes = [n for n, _ in rd.msa_partition_probe(phy, lines)]
    assert sum(sizes) == len(weights)

    rng = np.random.default_rng(9)
    rls = [tree.root_location(i).with_ratio(float(rng.uniform(0.1, 0.9))) for i in (0, 11, 57, 120, 198)]
    sets = random_param_sets(rng, len(rls), 4, partitions=2)
    home = tree.root_location(11).with_ratio(0.3)
    lh_before, root_before = m.compute_lh(home), m.compute_lh_root(home)
    freqs_before = [m.partition_frequencies(p) for p in range(2)]
    got = m.site_lnls(rls, sets)
    at = 0
    for p, (size, cats) in enumerate(zip(sizes, (4, 1))):
        seqs = {k: s[at:at + size] for k, s in zip(names, compressed)}
        want = oracle_rows(t2, seqs, ORC_MAP_NT, 4, cats, rls, [s[p] for s in sets])
        assert_rows(got[:, at:at + size], want, "partition %d of two" % p)
        at += size
    for p in range(2):
        assert np.array_equal(m.partition_frequencies(p), freqs_before[p])
    assert m.compute_lh_root(home) == root_before
    assert m.compute_lh(home) == lh_before
    for rl, row in zip(rls, m.site_lnls(rls)):
        assert util.rel_err(float(np.dot(weights.astype(np.float64), row)), m.compute_lh(rl)) < LNL_TOL


def test_site_sharded_model_refuses_with_its_own_error():
    tree = rd.Tree.from_file(os.path.join(util.DATA, "10.tree"))
    m = rd.Model.from_file_block(tree, os.path.join(util.DATA, "10.fasta"), 0, 2)
    m.set_lnl_reducer(lambda values, n: None)
    m.initialize_partitions()
    for call in (m.site_patterns, lambda: m.site_lnls([tree.root_location(0)])):
        with pytest.raises(rd.RdamdError, match="site group"):
            call()
        assert rd.lib.rdamd_errno() == 61
