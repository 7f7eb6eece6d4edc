"""Pair sums for protein data: the pair-sum consumer of the 20-state pre-order walk on the matrix cores
(csrc/kernels_preorder_k20.hip) through rdamd_pair_sums, Partition.pair_sums, Model.gradient and
Model.substitutions -- and the 4-state and binary partitions through the same call.

The restatement is tests/grad_ref.py (NumPy, every vector renormalised per site; held to central
differences of the CPU oracle at 20 states by tests/test_grad_reference_k20.py), fed the device's own
P-matrices: exp(Qt) is not under test.  Every term of N, M and W is non-negative, so a sum is its own
absolute-value companion and the bound is test_gpu_pair_sums.py's: |x - x_ref| <= 1e-11 x_ref entry by
entry, which also makes an entry that is exactly 0 in the restatement exactly 0 on the device.
Models are UNREST (380 random rates, Dirichlet frequencies, unequal category weights: a symmetric
model would hide N^T), pattern weights are unequal, 1 to 5."""
import math

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import grad_ref
import subst_ref
import util
from test_gpu_k20_ancestral import protein_partition, AA, AA_MAP, ODD
from test_gpu_ancestral import traverse, caterpillar, random_columns
from test_gpu_brlen import make_partition as dna_partition, tip_root, inner_root, TOL
from test_gpu_k20_brlen import weighted, tip_branches, protein_workload  # noqa: F401  (protein_workload: fixture)
from test_gpu_pair_sums import assert_identities

pytestmark = pytest.mark.gpu

WORST = {"N": 0.0, "M": 0.0, "W": 0.0}   # the largest |x - x_ref| / x_ref of the module, printed by every comparison


def restate(p, tree, ops, seqs, freqs, w, weights, fidx=None, smallest=None):
    fidx = [0] * len(w) if fidx is None else fidx
    return grad_ref.pair_sums(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, AA_MAP, 20),
                              brlen_ref.pmatrices(p, ops), [freqs[m] for m in fidx], w, weights, smallest)


def assert_close(what, got, want):
    """got, want = (N, M, W): each figure printed, then |x - x_ref| <= 1e-11 x_ref (0 where x_ref is 0)"""
    for name, x, ref in zip(("N", "M", "W"), got, want):
        assert x.shape == ref.shape and np.all(np.isfinite(x))
        ratio = np.abs(x - ref) / np.where(ref > 0, ref, 1.0)
        WORST[name] = max(WORST[name], float(ratio.max()))
        print("%s %s: largest |x - x_ref| / x_ref %.3e (largest x %.3e, %d of %d entries are 0); worst so far N %.3e, M %.3e, "
              "W %.3e" % (what, name, ratio.max(), ref.max(), (ref == 0).sum(), ref.size, WORST["N"], WORST["M"], WORST["W"]))
        assert np.all(np.abs(x - ref) <= TOL * ref)


# ---- 1. lane map and both stages of the sum -------------------------------------------------
@pytest.fixture(scope="module")
def thirteen():
    rng = np.random.default_rng(1320)
    newick, _ = synth.random_tree(13, rng)
    labels = ["t%04d" % i for i in range(13)]
    return newick, random_columns(rng, labels, 33, AA, ODD)


# (S = 17 and 33: two and three tiles; R = 5 and 8: the 512-thread instantiation)
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
        got = p.pair_sums(ops)
        assert got[0].shape == (12, 2, R, 20, 20) and got[1].shape == (R, 20) and got[2].shape == (R,)
        want = restate(p, tree, ops, seqs, freqs, w, weights)
        what = "S %d R %d %s root" % (S, R, where)
        assert_close(what, got, want)
        tb = tip_branches(ops, 13)
        assert len(tb) == 13
        for k, c in tb:   # tip children have pair sums too
            assert got[0][k, c].max() > 0 and np.all(np.abs(got[0][k, c] - want[0][k, c]) <= TOL * want[0][k, c])
        assert_identities(what, p, ops, got, w, [freqs[0]] * R, weights)


# ---- 2. frequency indices -------------------------------------------------------------------
def test_frequency_set_per_category(thirteen):
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:17] for l, s in all_seqs.items()}
    rng = np.random.default_rng(202)
    p, freqs, w = protein_partition(tree, seqs, 3, rng, rate_matrices=2)
    weights = weighted(p, rng)
    rl = inner_root(tree).with_ratio(0.6)
    mixed, plain = [1, 0, 1], [0, 0, 0]
    ops, pmi, brl = tree.generate_operations(rl)
    p.update_prob_matrices(pmi, brl, mixed)
    p.update_clvs(ops)
    got = p.pair_sums(ops, mixed)
    assert_close("freqs %s" % mixed, got, restate(p, tree, ops, seqs, freqs, w, weights, mixed))
    assert_identities("freqs %s" % mixed, p, ops, got, w, [freqs[m] for m in mixed], weights)
    other = p.pair_sums(ops, plain)
    assert_close("freqs %s" % plain, other, restate(p, tree, ops, seqs, freqs, w, weights, plain))
    moved = np.abs(other[0] - got[0]).max()
    print("N moves by %.3e with the frequency indices" % moved)
    assert moved > 1e-3


# ---- 3. parents from slots, registers and pi ------------------------------------------------
def test_balanced_tree_reads_parents_from_slots_registers_and_pi():
    rng = np.random.default_rng(1619)
    tree = rd.Tree.from_newick(util.balanced_newick(16, rng))
    seqs = random_columns(rng, ["t%d" % i for i in range(16)], 17, AA, ODD)
    p, freqs, w = protein_partition(tree, seqs, 4, rng)
    weights = weighted(p, rng)
    ops = traverse(p, tree, tree.root_location(5).with_ratio(0.4))
    assert rd.ancestral_workspace_slots(ops, 16) >= 2
    assert_close("balanced, 16 tips, %d slots" % rd.ancestral_workspace_slots(ops, 16), p.pair_sums(ops),
                 restate(p, tree, ops, seqs, freqs, w, weights))


# ---- 4. passes ------------------------------------------------------------------------------
def test_passes_give_the_bytes_of_one_pass(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(33)
    R = 3
    p, _, _ = protein_partition(tree, seqs, R, rng)   # S = 33: three tiles
    weighted(p, rng)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    row_bytes = 8 * (len(ops) * 2 * R * 400 + R * 21)   # one tile's partial sums
    whole = p.pair_sums(ops, workspace_bytes=4 * row_bytes)   # one pass
    assert rd.pair_sums_last_ms() > 0 and whole[0].max() > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, p.pair_sums(ops)))
    for bound in (row_bytes + 8, row_bytes - 8, 1, 2 * row_bytes):
        cut = p.pair_sums(ops, workspace_bytes=bound)
        assert rd.pair_sums_last_ms() > 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, cut)), bound


# ---- 5. I2 on the device --------------------------------------------------------------------
def test_contraction_with_q_p_is_the_branch_derivative(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(44)
    R = 4
    p, freqs, w = protein_partition(tree, seqs, R, rng)
    weights = weighted(p, rng)
    rates = np.array(rd.compute_gamma_cats(0.7, R))   # (protein_partition's)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    N, M, W = p.pair_sums(ops)
    d1, _ = p.branch_length_derivatives(ops)
    q = brlen_ref.build_q(p.subst_params(0), freqs[0])
    pm = brlen_ref.pmatrices(p, ops)
    n, worst = len(ops), 0.0
    for k in range(n):
        for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
            got = sum(rates[r] * (N[k, c, r] * (q @ pm[m][r])).sum() for r in range(R))
            bound = sum(rates[r] * (N[k, c, r] * np.abs(q @ pm[m][r])).sum() for r in range(R))
            worst = max(worst, abs(got - d1[k, c]) / bound)
            assert abs(got - d1[k, c]) <= 1e-10 * bound
    print("I2, largest |contraction - d1| / bound %.3e" % worst)
    assert_identities("R 4", p, ops, (N, M, W), w, [freqs[0]] * R, weights)


# ---- 6. depth -------------------------------------------------------------------------------
@pytest.mark.parametrize("deep_first", [True, False])
def test_deep_tree_under_the_rescale_rule(deep_first):
    """the rates are reset to alpha 20 for the reason in test_gpu_pair_sums.py's docstring; the two
    conditions on the inputs are asserted from the restatement alone"""
    rng = np.random.default_rng(1900 + deep_first)
    newick, labels = caterpillar(299, deep_first, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 300
    seqs = {l: "".join(rng.choice(list(AA), size=17)) for l in labels}
    R = 2
    p, freqs, w = protein_partition(tree, seqs, R, rng)
    p.set_category_rates(rd.compute_gamma_cats(20.0, R))
    weights = weighted(p, rng)
    ops = traverse(p, tree, tree.root_location("t299").with_ratio(0.5))   # the whole spine below one child
    assert len(ops) == 299
    assert p.get_scaler(tree.root_scaler_index()).max() > 0   # the rule fires
    got = p.pair_sums(ops)
    smallest = []
    want = restate(p, tree, ops, seqs, freqs, w, weights, smallest=smallest)
    print("deep child first %s: smallest entry of a vector relative to its site's largest 2^%.1f" % (
        deep_first, np.log2(min(smallest))))
    assert min(smallest) >= 2.0 ** -500
    assert_close("deep child first %s" % deep_first, got, want)


# ---- 7. determinism, read-only --------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_the_partition_is_only_read(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(5)
    p, _, _ = protein_partition(tree, seqs, 4, rng)
    weighted(p, rng)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    root_clv = p.get_clv(tree.root_clv_index())
    pm = p.get_pmatrix(ops[0].child1_matrix_index)
    lnl = p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    a = p.pair_sums(ops)
    assert rd.pair_sums_last_ms() > 0
    b = p.pair_sums(ops)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    pair = np.zeros_like(a[0])   # root_out and cat_out may be left out
    fi = np.zeros(4, dtype=np.uint32)
    assert rd.lib.rdamd_pair_sums(p.handle, rd.api._op_array(ops), len(ops), rd.api._uptr(fi), 0, rd.api._dptr(pair), None,
                                  None) == 1
    assert pair.tobytes() == a[0].tobytes()
    assert np.array_equal(p.get_clv(tree.root_clv_index()), root_clv)
    assert np.array_equal(p.get_pmatrix(ops[0].child1_matrix_index), pm)
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl


# ---- 8. 4-state and binary partitions through the new call ----------------------------------
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
    old = p.branch_pair_sums(ops)
    new = p.pair_sums(ops)
    assert old[0].max() > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(old, new))


# ---- 9. refusals ----------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable(thirteen):
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:17] for l, s in all_seqs.items()}
    rng = np.random.default_rng(7)
    good, _, _ = protein_partition(tree, seqs, 4, rng)
    rl = tree.root_location(7).with_ratio(0.6)
    ops = traverse(good, tree, rl)

    def valid_call():
        N, M, W = good.pair_sums(ops)
        assert all(np.all(np.isfinite(v)) for v in (N, M, W)) and N.max() > 0
        assert rd.pair_sums_last_ms() > 0

    def refused(errno, match, call, *args, **kw):
        with pytest.raises(rd.RdamdError, match=match):
            call(*args, **kw)
        assert rd.lib.rdamd_errno() == errno and rd.pair_sums_last_ms() == 0
        assert b"rdamd_pair_sums:" in rd.lib.rdamd_errmsg()
        valid_call()

    valid_call()
    b = tree.branch_count()
    sparse = rd.Partition(13, b, 20, 17, 1, b, 4, b, rd.ATTRIB_NONREV | rd.ATTRIB_SPARSE_CLVS)
    util.load_tips(sparse, tree, seqs, AA_MAP)
    refused(63, "SPARSE_CLVS", sparse.pair_sums, traverse(sparse, tree, rl))
    # 20 states in the plain CLV layout: 16 rate categories
    p16 = rd.Partition(13, b, 20, 17, 1, b, 16, b, rd.ATTRIB_NONREV)
    util.load_tips(p16, tree, seqs, AA_MAP)
    p16.set_category_rates(rd.compute_gamma_cats(1.0, 16))
    refused(63, "16 rate categories", p16.pair_sums, traverse(p16, tree, rl))
    # a list that does not end in the root operation
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    refused(64, "root operation", good.pair_sums, shuffled)
    # NULL pair_out
    fi = np.zeros(4, dtype=np.uint32)
    assert rd.lib.rdamd_pair_sums(good.handle, rd.api._op_array(ops), len(ops), rd.api._uptr(fi), 0, None, None, None) != 1
    assert rd.lib.rdamd_errno() == 67 and rd.pair_sums_last_ms() == 0 and b"rdamd_pair_sums:" in rd.lib.rdamd_errmsg()
    valid_call()
    # the old entry point still refuses the 20-state partition
    with pytest.raises(rd.RdamdError, match="20-state"):
        good.branch_pair_sums(ops)
    assert rd.lib.rdamd_errno() == 63 and rd.pair_sums_last_ms() == 0
    valid_call()
    assert np.isfinite(util.compute_lh(sparse, tree, rl)) and np.isfinite(util.compute_lh(p16, tree, rl))


def test_a_site_without_likelihood_is_error_65(thirteen):
    """test_gpu_k20_brlen.py's construction: a frequency that is exactly 0 and a column fixed in that state"""
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:17] for l, s in all_seqs.items()}
    seqs = {l: s.replace(AA[6], AA[7]) for l, s in seqs.items()}
    fixed = {l: s[:4] + AA[6] + s[5:] for l, s in seqs.items()}
    rng = np.random.default_rng(65)
    p, freqs, w = protein_partition(tree, fixed, 2, rng)
    f = np.array(freqs[0])
    f[6] = 0.0
    f /= f.sum()
    p.set_frequencies(0, f)
    rl = inner_root(tree).with_ratio(0.6)
    with pytest.raises(rd.RdamdError, match="1 of 17 sites"):
        p.pair_sums(traverse(p, tree, rl))
    assert rd.lib.rdamd_errno() == 65 and rd.pair_sums_last_ms() == 0
    assert b"rdamd_pair_sums:" in rd.lib.rdamd_errmsg()
    # the other columns are fine: without that column the same model gives sums
    q, _, _ = protein_partition(tree, seqs, 2, np.random.default_rng(65))
    q.set_frequencies(0, f)
    N, M, W = q.pair_sums(traverse(q, tree, rl))
    assert np.all(np.isfinite(N)) and N.max() > 0 and rd.pair_sums_last_ms() > 0


# ---- 10. the model --------------------------------------------------------------------------
def protein_model(wl, cmap):
    tree = rd.Tree.from_newick(wl["newick"])
    m = rd.Model(tree, wl["seqs"], states=20, cmap=cmap, rate_cats=4, seed=3)
    m.initialize_partitions()
    return tree, m


def test_model_gradient_protein(protein_workload):
    """Model.gradient against central differences of Model.site_lnls (it takes protein models), formed
    per pattern and summed with fsum as check_model_gradient forms them: step 1e-5, bound
    1e-4 max(1, |g|); alpha, all 20 frequencies, 40 of the 380 rates drawn with a fixed seed, the first
    and the last among them.  Then the same gradient against grad_ref.gradient fed the device's sums."""
    wl, cmap, pp = protein_workload
    tree, m = protein_model(wl, cmap)
    home = tree.root_location(0).with_ratio(0.4)
    rl = tree.root_location(3).with_ratio(0.27)
    step = 1e-5
    lh_home, root_home = m.compute_lh(home), m.compute_lh_root(home)
    before = m.partition_frequencies(0)
    weights = m.site_patterns()[0].astype(np.float64)
    grad, lnl = m.gradient(rl, [pp])
    base = m.site_lnls([rl], [[pp]])[0]
    assert util.rel_err(lnl, math.fsum(weights * base)) < 1e-10
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home
    assert np.array_equal(m.partition_frequencies(0), before)
    assert len(grad) == 1 and len(grad[0]["subst_rates"]) == 380 and len(grad[0]["gamma_weights"]) == 0
    drawn = sorted(set([0, 379]) | set(np.random.default_rng(380).choice(380, 40, replace=False).tolist()))
    assert len(drawn) >= 40
    for key, which in (("gamma_alpha", [0]), ("freqs", range(20)), ("subst_rates", drawn)):
        worst = 0.0
        for i in which:
            f = []
            for sign in (1.0, -1.0):
                moved = {k: list(v) for k, v in pp.items()}
                moved[key][i] += sign * step
                f.append(m.site_lnls([rl], [[moved]])[0])
            cd = math.fsum(weights * (f[0] - f[1])) / (2 * step)
            g = grad[0][key][i]
            worst = max(worst, abs(g - cd) / max(1.0, abs(g)))
        print("protein model %s: largest scaled error %.3e over %d parameters (largest |g| %.3e)" % (
            key, worst, len(list(which)), np.abs(grad[0][key]).max()))
        assert worst <= 1e-4
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home

    # a partition set up as the model sets its own: the device's sums, the restatement's assembly
    t2 = rd.Tree.from_newick(wl["newick"])
    S = len(next(iter(wl["seqs"].values())))
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], 4, rd.GAMMA_RATES_MEDIAN))
    w = np.full(4, 0.25)
    p = rd.Partition.for_tree(t2, 20, S, 4, rd.ATTRIB_NONREV)
    util.load_tips(p, t2, wl["seqs"], cmap)
    p.set_subst_params(0, pp["subst_rates"])
    p.set_frequencies(0, f)
    p.set_category_rates(rates)
    p.set_category_weights(w)
    sched = t2.generate_operations(rl)
    ops = traverse(p, t2, rl)
    N, M, W = p.pair_sums(ops)
    lengths = grad_ref.branch_lengths(*sched)
    (d_subst, d_pi, d_rho, _), (c_subst, c_pi, c_rho, _) = grad_ref.gradient(
        N, M, W, lengths, [np.array(pp["subst_rates"])], [f], [0] * 4, [0] * 4, rates, w)
    g = rd.gradient_from_pair_sums(N, M, W, lengths, [pp["subst_rates"]], [f], [0] * 4, [0] * 4, rates, w)
    for name, a, b, C in zip(("subst", "freqs", "rates"), g, (d_subst, d_pi, d_rho), (c_subst, c_pi, c_rho)):
        print("protein gradient %s: largest |g - g_ref| / C %.3e" % (name, (np.abs(a - b) / C).max()))
        assert np.all(np.abs(a - b) <= 10 * TOL * C)   # test_gpu_pair_sums.py's bound for this comparison
    # ... and the model's own substitution-rate entries are those (the rates enter as given)
    assert np.all(np.abs(grad[0]["subst_rates"] - d_subst[0]) <= 10 * TOL * c_subst[0])


def test_model_substitutions_protein(protein_workload):
    wl, cmap, pp = protein_workload
    tree, m = protein_model(wl, cmap)
    home = tree.root_location(0).with_ratio(0.4)
    rl = tree.root_location(3).with_ratio(0.27)
    lh_home, root_home = m.compute_lh(home), m.compute_lh_root(home)
    out = m.substitutions(rl, [pp], per_site=False)
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home
    assert not any(key in out for key in ("change", "count", "top_prob", "top_pair"))
    typed, lengths = out["typed"][0], out["lengths"]
    assert typed.shape == (8, 2, 20, 20) and np.all(np.isfinite(typed))
    off = ~np.eye(20, dtype=bool)
    assert typed[:, :, off].min() >= 0 and typed[:, :, off].max() > 0
    total = float(m.site_patterns()[0].sum())
    _, _, _, _, d1, _, _ = m.branch_derivatives(rl, [pp])
    # identity C needs the diagonal contraction, which the pair sums hold: the same evaluation on a partition
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], 4, rd.GAMMA_RATES_MEDIAN))
    t2 = rd.Tree.from_newick(wl["newick"])
    p = rd.Partition.for_tree(t2, 20, len(next(iter(wl["seqs"].values()))), 4, rd.ATTRIB_NONREV)
    util.load_tips(p, t2, wl["seqs"], cmap)
    p.set_subst_params(0, pp["subst_rates"])
    p.set_frequencies(0, f)
    p.set_category_rates(rates)
    p.set_category_weights(np.full(4, 0.25))
    N, _, _ = p.pair_sums(traverse(p, t2, rl))
    q = brlen_ref.build_q(pp["subst_rates"], f)
    ref_typed, comp, diag, diag_comp = subst_ref.typed_counts(N, lengths, [q] * 4, rates)
    assert np.all(np.abs(typed - ref_typed) <= 1e-11 * comp)   # (test_gpu_subst.py's bound for the model's typed counts)
    worst_c = worst_d = 0.0
    for k in range(8):
        for c in range(2):
            tau = lengths[k, c]
            dwell = np.trace(typed[k, c])
            assert abs(dwell - tau * total) <= 1e-11 * tau * total   # D (1e-11: that file's bound for sums over sites)
            e_sum = typed[k, c][off].sum()
            cc = abs(tau * d1[k, c] - (e_sum + diag[k, c]))
            assert cc <= 1e-11 * (e_sum + diag_comp[k, c])           # C
            if tau > 0:
                worst_d = max(worst_d, abs(dwell - tau * total) / (tau * total))
                worst_c = max(worst_c, cc / (e_sum + diag_comp[k, c]))
    print("protein model: identity C %.3e, D %.3e of the companions" % (worst_c, worst_d))
    with pytest.raises(rd.RdamdError, match="partition 0"):
        m.substitutions(rl, [pp], per_site=True)
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home


def test_model_substitutions_dna_without_per_site_has_the_typed_bytes():
    tree = rd.Tree.from_file(util.DATA + "/10.tree")
    packed, weights = util.compress(util.read_fasta(util.DATA + "/10.fasta"))
    m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
    m.initialize_partitions()
    rng = np.random.default_rng(11)
    pp = {"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": [0.125, 0.375, 0.25, 0.25],
          "gamma_alpha": [0.6], "gamma_weights": []}
    rl = tree.root_location(3).with_ratio(0.27)
    full = m.substitutions(rl, [pp])
    bare = m.substitutions(rl, [pp], per_site=False)
    assert "count" in full and "count" not in bare and full["typed"][0].max() > 0
    assert bare["typed"][0].tobytes() == full["typed"][0].tobytes() and bare["lnl"] == full["lnl"]
    assert bare["lengths"].tobytes() == full["lengths"].tobytes()
