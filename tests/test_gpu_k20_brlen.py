"""Branch-length derivatives and optimised lengths for protein data: the derivative consumer of the
20-state pre-order walk on the matrix cores (csrc/kernels_preorder_k20.hip) through
rdamd_branch_length_derivatives, Partition.branch_length_derivatives, Model.branch_derivatives and
Model.optimize_branch_lengths -- and the 4-state and binary partitions through the same call.

The reference is tests/brlen_ref.py (NumPy, every vector renormalised per site; held to central
differences of the CPU oracle at 20 states by tests/test_brlen_reference_k20.py), fed the device's
own P-matrices: exp(Qt) is not under test.  The acceptance rule is tests/test_gpu_brlen.py's:
|d - d_ref| <= 1e-11 A, A the absolute-value companion of the sum (its docstring says why); 1e-9 A
against a host matrix exponential, that file's and test_gpu_ancestral.py's figure for the model.
Models are UNREST (380 random rates, Dirichlet frequencies, unequal category weights: a symmetric
model would hide a Q / Q^T mix-up), pattern weights are unequal, 1 to 5."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import util
from test_gpu_k20_ancestral import protein_partition, AA, AA_MAP, ODD
from test_gpu_ancestral import traverse, caterpillar, random_columns, expm
from test_gpu_brlen import make_partition as dna_partition, model_partition, tip_root, inner_root, TOL
from test_brlen_reference import STEP

pytestmark = pytest.mark.gpu

WORST = {"d1": 0.0, "d2": 0.0}   # the largest |d - d_ref| / A of the module, printed by every comparison


def weighted(p, rng):
    weights = rng.integers(1, 6, p.sites).astype(np.uint32)
    p.set_pattern_weights(weights)
    return weights


def rates_of(R):
    return np.array(rd.compute_gamma_cats(0.7, R)) if R > 1 else np.ones(1)   # (protein_partition's)


def restate(p, tree, ops, seqs, freqs, w, weights, pidx=None, fidx=None):
    R = len(w)
    pidx = [0] * R if pidx is None else pidx
    fidx = pidx if fidx is None else fidx
    qs = [brlen_ref.build_q(p.subst_params(m), freqs[m]) for m in pidx]
    assert np.abs(qs[0] - qs[0].T).max() > 1e-2
    return brlen_ref.branch_derivatives(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, AA_MAP, 20),
                                        brlen_ref.pmatrices(p, ops), qs, [freqs[m] for m in fidx], w, rates_of(R), weights)


def assert_close(what, got, want, tol=TOL):
    """got = (d1, d2), want = (d1, d2, A1, A2): each figure printed, then |d - d_ref| <= tol A"""
    for name, d, ref, A in (("d1", got[0], want[0], want[2]), ("d2", got[1], want[1], want[3])):
        ratio = np.abs(d - ref) / A
        if tol == TOL:
            WORST[name] = max(WORST[name], float(ratio.max()))
        print("%s %s: largest |d - d_ref| / A %.3e (largest |d| %.3e); worst so far d1 %.3e, d2 %.3e" % (
            what, name, ratio.max(), np.abs(ref).max(), WORST["d1"], WORST["d2"]))
        assert np.all(np.isfinite(d))
        assert np.all(np.abs(d - ref) <= tol * A)


def tip_branches(ops, tips):
    n = len(ops)
    return [(k, c) for k in range(n) for c, (child, _) in enumerate(brlen_ref.children_of(ops[n - 1 - k])) if child < tips]


# ---- 1. lane map and both stages of the sum -------------------------------------------------
@pytest.fixture(scope="module")
def thirteen():
    rng = np.random.default_rng(1319)
    newick, _ = synth.random_tree(13, rng)
    labels = ["t%04d" % i for i in range(13)]
    return newick, random_columns(rng, labels, 33, AA, ODD)


# (S = 17 and 33: two and three workgroups; R = 5 and 8: the 512-thread instantiation)
@pytest.mark.parametrize("S,R", [(S, R) for S in (1, 15, 16, 17, 33) for R in (1, 2, 3, 4, 5, 8)])
def test_lane_map_and_both_stages_of_the_sum(thirteen, S, R):
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(1000 * S + R)
    p, freqs, w = protein_partition(tree, seqs, R, rng)
    weights = weighted(p, rng)
    for where, rl in (("inner", inner_root(tree)), ("tip", tip_root(tree))):
        ops = traverse(p, tree, rl.with_ratio(0.6))
        if where == "tip":
            assert min(ops[-1].child1_clv_index, ops[-1].child2_clv_index) < 13
        got = p.branch_length_derivatives(ops)
        assert got[0].shape == (12, 2) and got[1].shape == (12, 2)
        want = restate(p, tree, ops, seqs, freqs, w, weights)
        assert_close("S %d R %d %s root" % (S, R, where), got, want)
        tb = tip_branches(ops, 13)
        assert len(tb) == 13
        for k, c in tb:   # tip children have branches too
            assert got[0][k, c] != 0.0 and abs(got[0][k, c] - want[0][k, c]) <= TOL * want[2][k, c]


# ---- 2. parameter and frequency indices -----------------------------------------------------
def test_rate_matrix_and_frequency_set_per_category(thirteen):
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:17] for l, s in all_seqs.items()}
    rng = np.random.default_rng(202)
    p, freqs, w = protein_partition(tree, seqs, 3, rng, rate_matrices=2)
    weights = weighted(p, rng)
    rl = inner_root(tree).with_ratio(0.6)
    mixed, plain = [1, 0, 1], [0, 0, 0]
    found = {}
    for pidx, fidx in ((mixed, mixed), (plain, mixed), (mixed, plain), (plain, plain)):
        ops, pmi, brl = tree.generate_operations(rl)
        p.update_prob_matrices(pmi, brl, pidx)
        p.update_clvs(ops)
        got = p.branch_length_derivatives(ops, pidx, fidx)
        assert_close("params %s freqs %s" % (pidx, fidx), got, restate(p, tree, ops, seqs, freqs, w, weights, pidx, fidx))
        found[(tuple(pidx), tuple(fidx))] = got[0]
    key = lambda a, b: (tuple(a), tuple(b))
    by_params = np.abs(found[key(mixed, mixed)] - found[key(plain, mixed)]).max()
    by_freqs = np.abs(found[key(mixed, mixed)] - found[key(mixed, plain)]).max()
    print("d1 moves by %.3e with the rate-matrix indices, by %.3e with the frequency indices" % (by_params, by_freqs))
    assert by_params > 1e-3 and by_freqs > 1e-3


# ---- 3. parents from slots, registers and pi ------------------------------------------------
def test_balanced_tree_reads_parents_from_slots_registers_and_pi():
    rng = np.random.default_rng(1619)
    tree = rd.Tree.from_newick(util.balanced_newick(16, rng))
    seqs = random_columns(rng, ["t%d" % i for i in range(16)], 17, AA, ODD)
    p, freqs, w = protein_partition(tree, seqs, 4, rng)
    weights = weighted(p, rng)
    ops = traverse(p, tree, tree.root_location(5).with_ratio(0.4))
    assert rd.ancestral_workspace_slots(ops, 16) >= 2
    got = p.branch_length_derivatives(ops)
    assert_close("balanced, 16 tips, %d slots" % rd.ancestral_workspace_slots(ops, 16), got,
                 restate(p, tree, ops, seqs, freqs, w, weights))


# ---- 4. depth -------------------------------------------------------------------------------
@pytest.mark.parametrize("deep_first", [True, False])
def test_deep_tree_under_the_rescale_rule(deep_first):
    rng = np.random.default_rng(1900 + deep_first)
    newick, labels = caterpillar(299, deep_first, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 300
    seqs = {l: "".join(rng.choice(list(AA), size=17)) for l in labels}
    p, freqs, w = protein_partition(tree, seqs, 2, rng)
    weights = weighted(p, rng)
    ops = traverse(p, tree, tree.root_location("t299").with_ratio(0.5))   # the whole spine below one child
    assert len(ops) == 299
    assert p.get_scaler(tree.root_scaler_index()).max() > 0   # the rule fires
    got = p.branch_length_derivatives(ops)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert_close("deep child first %s" % deep_first, got, restate(p, tree, ops, seqs, freqs, w, weights))


# ---- 5. repeatability, read-only ------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_the_partition_is_only_read(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(5)
    p, _, _ = protein_partition(tree, seqs, 4, rng)
    weighted(p, rng)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    inner = [o.parent_clv_index for o in ops]
    clvs = [p.get_clv(i) for i in inner]
    scalers = [p.get_scaler(o.parent_scaler_index) for o in ops if o.parent_scaler_index >= 0]
    pm = p.get_pmatrix(ops[0].child1_matrix_index)
    lnl = p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    a = p.branch_length_derivatives(ops)
    assert rd.branch_last_ms() > 0
    b = p.branch_length_derivatives(ops)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    d1, none = p.branch_length_derivatives(ops, second=False)   # d2_out = NULL: the second product is skipped
    assert none is None and d1.tobytes() == a[0].tobytes()
    assert rd.branch_last_ms() > 0
    assert all(np.array_equal(p.get_clv(i), c) for i, c in zip(inner, clvs))
    assert all(np.array_equal(p.get_scaler(o.parent_scaler_index), s)
               for o, s in zip([o for o in ops if o.parent_scaler_index >= 0], scalers))
    assert np.array_equal(p.get_pmatrix(ops[0].child1_matrix_index), pm)
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl


# ---- 6. 4-state and binary partitions through the new call ----------------------------------
@pytest.mark.parametrize("states,R", [(4, 4), (4, 3), (2, 4), (2, 1)])
def test_dna_and_binary_partitions_have_the_old_bits(states, R):
    rng = np.random.default_rng(60 + 10 * states + R)
    newick, _ = synth.random_tree(13, rng)
    tree = rd.Tree.from_newick(newick)
    labels = ["t%04d" % i for i in range(13)]
    if states == 4:
        cmap, seqs = rd.MAP_NT, random_columns(rng, labels, 300, "ACGT", "RYKMSWBDHVN-")
    else:
        cmap, seqs = rd.MAP_BIN, random_columns(rng, labels, 300, "01", "-")
    p = dna_partition(tree, seqs, cmap, states, R, rng)[0]
    weighted(p, rng)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    old = p.branch_derivatives(ops)
    new = p.branch_length_derivatives(ops)
    assert np.abs(old[0]).max() > 0
    assert new[0].tobytes() == old[0].tobytes() and new[1].tobytes() == old[1].tobytes()
    assert p.branch_length_derivatives(ops, second=False)[0].tobytes() == old[0].tobytes()


# ---- 7. refusals ----------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable(thirteen):
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:17] for l, s in all_seqs.items()}
    rng = np.random.default_rng(7)
    good, _, _ = protein_partition(tree, seqs, 4, rng)
    rl = tree.root_location(7).with_ratio(0.6)
    ops = traverse(good, tree, rl)

    def valid_call():
        d1, d2 = good.branch_length_derivatives(ops)
        assert np.all(np.isfinite(d1)) and np.all(np.isfinite(d2)) and np.abs(d1).min() > 0
        assert rd.branch_last_ms() > 0

    def refused(errno, match, call, *args, **kw):
        with pytest.raises(rd.RdamdError, match=match):
            call(*args, **kw)
        assert rd.lib.rdamd_errno() == errno and rd.branch_last_ms() == 0
        assert b"rdamd_branch_length_derivatives:" in rd.lib.rdamd_errmsg()
        valid_call()

    valid_call()
    b = tree.branch_count()
    sparse = rd.Partition(13, b, 20, 17, 1, b, 4, b, rd.ATTRIB_NONREV | rd.ATTRIB_SPARSE_CLVS)
    util.load_tips(sparse, tree, seqs, AA_MAP)
    refused(63, "SPARSE_CLVS", sparse.branch_length_derivatives, traverse(sparse, tree, rl))
    # 20 states in the plain CLV layout: 16 rate categories
    p16 = rd.Partition(13, b, 20, 17, 1, b, 16, b, rd.ATTRIB_NONREV)
    util.load_tips(p16, tree, seqs, AA_MAP)
    p16.set_category_rates(rd.compute_gamma_cats(1.0, 16))
    refused(63, "16 rate categories", p16.branch_length_derivatives, traverse(p16, tree, rl))
    # 5 states
    p5 = rd.Partition(13, b, 5, 17, 1, b, 2, b, rd.ATTRIB_NONREV)
    util.load_tips(p5, tree, {l: "".join(AA[AA.index(ch) % 5] if ch in AA else "-" for ch in s) for l, s in seqs.items()},
                   util.make_map(AA[:5], {"-": 31}))
    refused(63, "5-state", p5.branch_length_derivatives, traverse(p5, tree, rl))
    # a list that does not end in the root operation
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    refused(64, "root operation", good.branch_length_derivatives, shuffled)
    # a rate matrix and a frequency set the partition does not have
    refused(7, "params", good.branch_length_derivatives, ops, params_indices=[0, 1, 0, 0], freqs_indices=[0, 0, 0, 0])
    refused(7, "freqs", good.branch_length_derivatives, ops, freqs_indices=[0, 0, 1, 0])
    # the old entry point still refuses the 20-state partition
    with pytest.raises(rd.RdamdError, match="20-state"):
        good.branch_derivatives(ops)
    assert rd.lib.rdamd_errno() == 63 and rd.branch_last_ms() == 0
    valid_call()
    assert np.isfinite(util.compute_lh(sparse, tree, rl)) and np.isfinite(util.compute_lh(p16, tree, rl))


# ---- 8. the model ---------------------------------------------------------------------------
def protein_model_restatement(tree, seqs, cmap, cats, ops, lengths, pp):
    """the parameters as model_t::set_model_params applies them (normalised frequencies, MEDIAN gamma
    rates, equal category weights), P-matrices by a host matrix exponential at lengths[k][c]"""
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    q = brlen_ref.build_q(pp["subst_rates"], f)
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], cats, rd.GAMMA_RATES_MEDIAN))
    n = len(ops)
    pmat = {m: np.stack([expm(q * r * lengths[k, c]) for r in rates])
            for k in range(n) for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k]))}
    S = len(next(iter(seqs.values())))
    return brlen_ref.branch_derivatives(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, cmap, 20), pmat,
                                        [q] * cats, [f] * cats, np.full(cats, 1.0 / cats), rates, np.ones(S))


@pytest.fixture(scope="module")
def protein_workload():
    wl = synth.workload(9, 120, 20, 4, 19)   # (every amino acid occurs: the model starts from empirical frequencies)
    rng = np.random.default_rng(8)
    pp = {"subst_rates": rng.uniform(0.1, 1.5, 380).tolist(), "freqs": rng.dirichlet(np.ones(20) * 4).tolist(),
          "gamma_alpha": [0.6], "gamma_weights": []}
    return wl, util.make_map(wl["alphabet"]), pp


def test_model_derivatives_and_the_root_identity_protein(protein_workload):
    wl, cmap, pp = protein_workload
    tree, t2 = rd.Tree.from_newick(wl["newick"]), rd.Tree.from_newick(wl["newick"])
    m = rd.Model(tree, wl["seqs"], states=20, cmap=cmap, rate_cats=4, seed=3)
    m.initialize_partitions()
    home = tree.root_location(0).with_ratio(0.4)
    lh_before, root_before = m.compute_lh(home), m.compute_lh_root(home)
    rl = tree.root_location(3).with_ratio(0.27)
    node_clv, node_parent, node_children, lengths, d1, d2, lnl = m.branch_derivatives(rl, [pp])
    # parameters, rooting and the CLVs of that rooting are as before
    assert m.compute_lh_root(home) == root_before
    assert m.compute_lh(home) == lh_before
    ops, pmi, brl = t2.generate_operations(rl)
    n = len(ops)
    want_clv, want_parent, want_children = rd.ancestral_nodes(ops)
    assert np.array_equal(node_clv, want_clv) and np.array_equal(node_parent, want_parent)
    assert np.array_equal(node_children, want_children)
    place = {int(mi): i for i, mi in enumerate(pmi)}
    sched = np.array([[brl[place[mi]] for _, mi in brlen_ref.children_of(ops[n - 1 - k])] for k in range(n)])
    assert np.array_equal(lengths, sched)
    assert d1.shape == (8, 2) and np.isfinite(lnl)
    assert_close("protein model, 9 taxa, host expm", (d1, d2),
                 protein_model_restatement(t2, wl["seqs"], cmap, 4, ops, lengths, pp), tol=1e-9)

    # d lnL / d alpha = T (d1 of the root child that gets alpha T - d1 of the other), the model's own parameters
    _, _, _, own_len, own_d1, _, own_lnl = m.branch_derivatives(rl)
    assert np.abs(own_d1 - d1).max() > 1e-3
    T = own_len[0, 0] + own_len[0, 1]
    near = 0 if abs(own_len[0, 0] - 0.27 * T) < abs(own_len[0, 1] - 0.27 * T) else 1
    assert abs(own_len[0, near] - 0.27 * T) < 1e-12 * max(1.0, T)
    want = T * (own_d1[0, near] - own_d1[0, 1 - near])
    got = (m.compute_lh(rl.with_ratio(0.27 + STEP)) - m.compute_lh(rl.with_ratio(0.27 - STEP))) / (2 * STEP)
    print("protein model: d lnL / d alpha %.9f, central difference of compute_lh %.9f; lnL %.6f" % (want, got, own_lnl))
    assert abs(want - got) <= 1e-4 * max(1.0, abs(want))
    assert util.rel_err(own_lnl, m.compute_lh(rl)) < 1e-10


def test_model_optimises_protein_branch_lengths(protein_workload):
    wl, cmap, pp = protein_workload
    atol, lo, hi = 1e-8, 1e-6, 100.0
    rng = np.random.default_rng(19)
    own = rd.Tree.from_newick(wl["newick"])
    split = sorted(own.side_tips(own.root_location(3)))
    rest = sorted(set(own.tip_label(i) for i in range(9)) - set(split))
    # the workload's tree with every length multiplied by a factor from [0.5, 2]
    ops, pmi, brl = own.generate_operations(util.find_root(own, split, rest, 0.27))
    n = len(ops)
    place = {int(mi): i for i, mi in enumerate(pmi)}
    lengths = np.array([[brl[place[mi]] for _, mi in brlen_ref.children_of(ops[n - 1 - k])] for k in range(n)])
    scaled = own.newick_branch_lengths(rd.ancestral_nodes(ops)[0], lengths * rng.uniform(0.5, 2.0, lengths.shape))
    tree, t2 = rd.Tree.from_newick(scaled), rd.Tree.from_newick(scaled)
    m = rd.Model(tree, wl["seqs"], states=20, cmap=cmap, rate_cats=4, seed=3)
    m.initialize_partitions()
    rl = util.find_root(tree, split, rest, 0.27)
    home = tree.root_location(0).with_ratio(0.4)
    lh_home, root_home = m.compute_lh(home), m.compute_lh_root(home)
    r = m.optimize_branch_lengths(rl, [pp], lo, hi, atol, 200)
    x = r["lengths"]
    print("protein model: lnL %.9f -> %.9f, %d iterations, %d evaluations, converged %s" % (
        r["lnl_before"], r["lnl_after"], r["iterations"], r["evaluations"], r["converged"]))
    assert r["converged"]
    assert x.min() >= lo and x.max() <= hi
    assert r["lnl_after"] >= r["lnl_before"]
    # nothing was applied: the model is bit for bit what it was
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home
    ops2, _, _ = t2.generate_operations(util.find_root(t2, split, rest, 0.27))
    d1, d2, _, _ = protein_model_restatement(t2, wl["seqs"], cmap, 4, ops2, x, pp)
    gain = brlen_ref.predicted_gain(x, d1, d2, lo, hi)
    print("protein model: predicted gain left %.3e" % gain)
    assert gain < 2 * atol   # (the factor 2: the difference between device and restatement derivatives)


def test_model_dna_through_the_new_call_has_the_old_bits():
    """the model's evaluation goes through rdamd_branch_length_derivatives now: for a 4-state model it
    returns what rdamd_branch_derivatives returns for a partition set up as the model sets its own
    (frequencies that sum to exactly 1, so that the model's normalisation changes no bit)"""
    tree, t2 = rd.Tree.from_file(util.DATA + "/10.tree"), rd.Tree.from_file(util.DATA + "/10.tree")
    packed, weights = util.compress(util.read_fasta(util.DATA + "/10.fasta"))
    m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
    m.initialize_partitions()
    rng = np.random.default_rng(11)
    pp = {"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": [0.125, 0.375, 0.25, 0.25],
          "gamma_alpha": [0.6], "gamma_weights": []}
    rl = tree.root_location(3).with_ratio(0.27)
    _, _, _, _, d1, d2, lnl = m.branch_derivatives(rl, [pp])
    ops, pmi, brl = t2.generate_operations(rl)
    p, f, _, _ = model_partition(t2, packed, weights, 4, pp)
    assert f.tolist() == pp["freqs"]
    p.update_prob_matrices(pmi, brl)
    p.update_clvs(ops)
    old = p.branch_derivatives(ops)
    assert np.abs(old[0]).max() > 0
    assert d1.tobytes() == old[0].tobytes() and d2.tobytes() == old[1].tobytes()
    assert util.rel_err(lnl, p.compute_root_loglikelihood(t2.root_clv_index(), t2.root_scaler_index())) < 1e-10


# ---- 9. error 65 ----------------------------------------------------------------------------
def test_a_site_without_likelihood_is_error_65(thirteen):
    """a frequency that is exactly 0 and a column fixed in that state: Q has a zero column there, so
    P keeps the state to itself, t = pi (.) (P L) is the zero vector at the root and below, f0 = 0"""
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:17] for l, s in all_seqs.items()}
    # (a column with that state in any tip has no likelihood under such a model: only column 4 holds it)
    seqs = {l: s.replace(AA[6], AA[7]) for l, s in seqs.items()}
    fixed = {l: s[:4] + AA[6] + s[5:] for l, s in seqs.items()}
    rng = np.random.default_rng(65)
    p, freqs, w = protein_partition(tree, fixed, 2, rng)
    f = np.array(freqs[0])
    f[6] = 0.0
    f /= f.sum()
    p.set_frequencies(0, f)
    rl = inner_root(tree).with_ratio(0.6)
    ops = traverse(p, tree, rl)
    with pytest.raises(rd.RdamdError, match="1 of 17 sites"):
        p.branch_length_derivatives(ops)
    assert rd.lib.rdamd_errno() == 65 and rd.branch_last_ms() == 0
    assert b"rdamd_branch_length_derivatives:" in rd.lib.rdamd_errmsg()
    # the other columns are fine: without that column the same model gives derivatives
    q, _, _ = protein_partition(tree, seqs, 2, np.random.default_rng(65))
    q.set_frequencies(0, f)
    d1, d2 = q.branch_length_derivatives(traverse(q, tree, rl))
    assert np.all(np.isfinite(d1)) and np.all(np.isfinite(d2)) and rd.branch_last_ms() > 0
