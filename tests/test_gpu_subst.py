"""Substitutions mapped onto branches: the pre-order walk of csrc/kernels_preorder.hip with its
substitution consumer, through rdamd_branch_substitutions and Model.substitutions.

The restatement is tests/subst_ref.py (NumPy/SciPy, every vector renormalised per site; checked by
test_subst_reference.py against exact enumeration and finite differences).  J, change and top_prob
are posteriors in [0, 1], held to 1e-12 absolute; n_s to 1e-11 of its absolute-value companion,
which is n_s itself (no term is negative): the project's figures for posteriors and pair sums.  On
the 600-tip caterpillar both are 5e-11, test_gpu_ancestral.py's figure for deep trees.

top_pair must equal the restatement's wherever the restatement's best and second-best pairs i != j
are more than 1e-9 apart, and also where every off-diagonal entry of the restatement is exactly 0
(a branch of length 0: the tie rule decides, code 1).  The share of (branch, site) pairs compared
in neither way is asserted to be at most 1 %.

One case of the issue's list cannot be built: "R = 4 with a 17-code table".  The pre-order pass
takes 4-state partitions only (binary data is embedded in four states), four states have 2^4 - 1
non-empty masks, and the partition's table has 16 entries: a character whose mask names a fifth
state is refused by rdamd_set_tip_states (asserted below).  The lane-per-site walk is reached by a
category count other than 1, 2, 4, 8 -- R = 3 and R = 5 here, 4-state and binary, one and two
workgroups -- or by 2^26 (site, rate) pairs, which no test of a few seconds holds."""
import itertools

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import grad_ref
import subst_ref
import util
from test_gpu_ancestral import caterpillar, random_columns
from test_gpu_brlen import MSA, TREE, make_partition, model_partition

pytestmark = pytest.mark.gpu

TOL_J, TOL_N, TOL_DEEP, GAP = 1e-12, 1e-11, 5e-11, 1e-9


def traverse(p, tree, rl, pidx=None, zero=()):
    """update_prob_matrices + update_clvs at root rl -> (ops, lengths[n][2]); zero: places in the
    schedule's list whose branch gets length 0"""
    ops, pmi, brl = tree.generate_operations(rl)
    brl = np.array(brl, dtype=np.float64)
    for at in zero:
        brl[at] = 0.0
    p.update_prob_matrices(pmi, brl, pidx)
    p.update_clvs(ops)
    return ops, grad_ref.branch_lengths(ops, [int(m) for m in pmi], brl)


def restate(p, tree, ops, lengths, seqs, cmap, K, subst, freqs, rates, w, pidx=None, fidx=None):
    R = len(w)
    pidx = [0] * R if pidx is None else pidx
    fidx = pidx if fidx is None else fidx
    qs = [brlen_ref.build_q(subst[m], freqs[m]) for m in pidx]
    cmat = subst_ref.count_matrices(lengths, qs, rates)
    return subst_ref.site_maps(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, cmap, K), brlen_ref.pmatrices(p, ops),
                               cmat, [freqs[m] for m in fidx], w)


def assert_close(what, got, J, cnt, tol_j=TOL_J, tol_n=TOL_N):
    """got: the dict of Partition.branch_substitutions (with joint); J, cnt: the restatement.  Each
    figure printed, then asserted."""
    change, top_pair, top_prob, gap = subst_ref.summaries(J)
    assert got["joint"].shape == J.shape and got["count"].shape == cnt.shape
    for v in got.values():
        assert np.all(np.isfinite(v))
    K = J.shape[-1]
    off = ~np.eye(K, dtype=bool)
    all_zero = np.all(J[..., off] == 0.0, axis=-1)
    compared = (gap > GAP) | all_zero
    left_out = 1.0 - compared.mean()
    figures = (np.abs(got["joint"] - J).max(), np.abs(got["change"] - change).max(), np.abs(got["top_prob"] - top_prob).max(),
               (np.abs(got["count"] - cnt) / np.where(cnt > 0, cnt, 1.0)).max())
    print("%s: largest |J - J_ref| %.3e, |change - ref| %.3e, |top_prob - ref| %.3e, |n - n_ref| / n_ref %.3e; top pairs "
          "left out %.4f %%, largest n %.3e" % ((what,) + figures + (100 * left_out, cnt.max())))
    assert figures[0] <= tol_j and figures[1] <= tol_j and figures[2] <= tol_j
    assert np.all(np.abs(got["count"] - cnt) <= tol_n * cnt)
    assert left_out <= 0.01
    assert np.array_equal(got["top_pair"][compared], top_pair[compared])
    assert np.abs(got["joint"].sum(axis=(3, 4)) - 1.0).max() <= 1e-12


# ---- 1. the lane maps on a 40-tip tree -----------------------------------------------------------
@pytest.fixture(scope="module")
def forty():
    """a 40-tip random tree and 257 columns with ambiguity codes; column 5 (column 0 of a one-column
    alignment is kept) is all gaps"""
    rng = np.random.default_rng(40)
    newick, _ = synth.random_tree(40, rng)
    labels = ["t%04d" % i for i in range(40)]
    nt = random_columns(rng, labels, 257, "ACGT", "RYKMSWBDHVN-")
    binary = random_columns(rng, labels, 257, "01", "-")
    for seqs in (nt, binary):
        for l in labels:
            seqs[l] = seqs[l][:5] + "-" + seqs[l][6:]
    return newick, nt, binary


def forty_case(forty, K, R, S, seed, rate_matrices=1, pidx=None):
    newick, nt, binary = forty
    tree = rd.Tree.from_newick(newick)
    cmap, all_seqs = (rd.MAP_NT, nt) if K == 4 else (rd.MAP_BIN, binary)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(seed)
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, cmap, K, R, rng, rate_matrices=rate_matrices)
    assert weights.max() > 1
    ops, lengths = traverse(p, tree, tree.root_location(21).with_ratio(0.6), pidx, zero=(7,))
    assert (lengths == 0.0).sum() == 1
    return p, tree, ops, lengths, seqs, cmap, subst, freqs, rates, w, weights


# fast walk: a (site, rate) pair per lane; 70 and 257 sites leave a partial last workgroup and a partial wave at every R
@pytest.mark.parametrize("S", [1, 70, 257])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_fast_walk_equals_the_restatement(forty, R, S):
    p, tree, ops, lengths, seqs, cmap, subst, freqs, rates, w, weights = forty_case(forty, 4, R, S, 1000 * S + R)
    got = p.branch_substitutions(ops, lengths, joint=True)
    assert rd.branch_substitutions_last_ms() > 0
    assert got["joint"].shape == (39, 2, S, 4, 4) and got["top_pair"].dtype == np.uint8
    J, cnt = restate(p, tree, ops, lengths, seqs, cmap, 4, subst, freqs, rates, w)
    assert_close("fast walk R %d S %d" % (R, S), got, J, cnt)


# lane-per-site walk: any other category count
@pytest.mark.parametrize("K,R,S", [(4, 3, 257), (4, 5, 70), (2, 3, 257), (4, 3, 1)])
def test_generic_walk_equals_the_restatement(forty, K, R, S):
    p, tree, ops, lengths, seqs, cmap, subst, freqs, rates, w, weights = forty_case(forty, K, R, S, 77 * S + R + K)
    got = p.branch_substitutions(ops, lengths, joint=True)
    assert got["joint"].shape == (39, 2, S, K, K)
    J, cnt = restate(p, tree, ops, lengths, seqs, cmap, K, subst, freqs, rates, w)
    assert_close("generic walk K %d R %d S %d" % (K, R, S), got, J, cnt)


@pytest.mark.parametrize("R,S", [(4, 70), (1, 257)])
def test_binary_data_gets_two_by_two_joints(forty, R, S):
    p, tree, ops, lengths, seqs, cmap, subst, freqs, rates, w, weights = forty_case(forty, 2, R, S, 5 * S + R)
    got = p.branch_substitutions(ops, lengths, joint=True)
    assert got["joint"].shape == (39, 2, S, 2, 2) and set(np.unique(got["top_pair"])) <= {1, 2}
    J, cnt = restate(p, tree, ops, lengths, seqs, cmap, 2, subst, freqs, rates, w)
    assert_close("binary R %d S %d" % (R, S), got, J, cnt)


def test_two_rate_matrices_with_their_own_indices_per_category(forty):
    pidx, fidx = [0, 1, 1, 0], [1, 1, 0, 0]
    p, tree, ops, lengths, seqs, cmap, subst, freqs, rates, w, weights = forty_case(forty, 4, 4, 70, 12, 2, pidx)
    got = p.branch_substitutions(ops, lengths, pidx, fidx, joint=True)
    J, cnt = restate(p, tree, ops, lengths, seqs, cmap, 4, subst, freqs, rates, w, pidx, fidx)
    assert_close("two rate matrices", got, J, cnt)
    other = p.branch_substitutions(ops, lengths, [0, 0, 0, 0], [0, 0, 0, 0])
    assert np.abs(other["count"] - got["count"]).max() > 1e-4   # the indices matter


def test_a_four_state_table_has_no_seventeenth_code(forty):
    newick, nt, _ = forty
    tree = rd.Tree.from_newick(newick)
    p = rd.Partition.for_tree(tree, 4, 20, 4, rd.ATTRIB_NONREV)
    # all 15 non-empty masks of four states, and one more character: its mask, 16, names a fifth state
    cmap = util.make_map("ACGT", {ch: m for ch, m in zip("abcdefghijkl", range(5, 17))})
    with pytest.raises(rd.RdamdError):
        p.set_tip_states(0, cmap, "ACGTabcdefghijklACGT"[:20])
    assert rd.lib.rdamd_errno() in (4, 5)


# ---- 2. the planner's keeps ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["caterpillar", "balanced"])
def test_register_slot_and_discard_keeps(shape):
    rng = np.random.default_rng(32)
    if shape == "caterpillar":
        newick, labels = caterpillar(31, True, rng)
        root = "t31"
    else:
        newick, labels = util.balanced_newick(32, rng), ["t%d" % i for i in range(32)]
        root = 9
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 32
    seqs = random_columns(rng, labels, 70, "ACGT", "RYN-")
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng)
    ops, lengths = traverse(p, tree, tree.root_location(root).with_ratio(0.4))
    slots = rd.ancestral_workspace_slots(ops, 32)
    # a caterpillar keeps every outer vector in registers; a balanced tree parks vectors in slots; tips are discarded
    assert slots == 0 if shape == "caterpillar" else slots >= 2
    got = p.branch_substitutions(ops, lengths, joint=True)
    J, cnt = restate(p, tree, ops, lengths, seqs, rd.MAP_NT, 4, subst, freqs, rates, w)
    assert_close(shape, got, J, cnt)


# ---- 3. depth ------------------------------------------------------------------------------------
def test_deep_caterpillar_under_the_rescale_rule():
    rng = np.random.default_rng(600)
    newick, labels = caterpillar(599, True, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 600
    seqs = {l: "".join(rng.choice(list("ACGT"), size=33)) for l in labels}
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng)
    ops, lengths = traverse(p, tree, tree.root_location("t599").with_ratio(0.5))
    assert len(ops) == 599
    assert p.get_scaler(tree.root_scaler_index()).max() > 0   # the rule fires
    got = p.branch_substitutions(ops, lengths, joint=True)
    J, cnt = restate(p, tree, ops, lengths, seqs, rd.MAP_NT, 4, subst, freqs, rates, w)
    assert_close("600-tip caterpillar", got, J, cnt, TOL_DEEP, TOL_DEEP)


# ---- 4. identities on the device's own outputs ----------------------------------------------------
@pytest.mark.parametrize("R", [4, 3])
def test_identities_tie_the_walks_consumers_together(forty, R):
    p, tree, ops, lengths, seqs, cmap, subst, freqs, rates, w, weights = forty_case(forty, 4, R, 257, 50 + R)
    got = p.branch_substitutions(ops, lengths, joint=True)
    N, _, _ = p.branch_pair_sums(ops)
    d1, _ = p.branch_derivatives(ops)
    typed = rd.substitution_counts(N, lengths, subst, freqs, [0] * R, rates)
    q = brlen_ref.build_q(subst[0], freqs[0])
    _, comp, diag, diag_comp = subst_ref.typed_counts(N, lengths, [q] * R, rates)
    pm = brlen_ref.pmatrices(p, ops)
    n, total = len(ops), float(weights.sum())
    off = ~np.eye(4, dtype=bool)
    worst = [0.0, 0.0, 0.0]
    for k in range(n):
        for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
            e_sum = typed[k, c][off].sum()
            a = abs((weights * got["count"][k, c]).sum() - e_sum)
            b = np.abs(np.einsum("s,sij->ij", weights.astype(np.float64), got["joint"][k, c]) - (N[k, c] * pm[m]).sum(axis=0)).max()
            cc = abs(lengths[k, c] * d1[k, c] - (e_sum + diag[k, c]))
            assert a <= 1e-11 * e_sum and b <= 1e-11 * total and cc <= 1e-11 * (e_sum + diag_comp[k, c])
            if lengths[k, c] > 0:
                worst = [max(x, y) for x, y in zip(worst, (a / e_sum, b / total, cc / (e_sum + diag_comp[k, c])))]
    print("R %d: identity A %.3e, B %.3e, C %.3e of the companions" % ((R,) + tuple(worst)))


# ---- 5. NULL outputs, determinism, read-only ------------------------------------------------------
def ten(R, seed, S=41):
    rng = np.random.default_rng(seed)
    tree = rd.Tree.from_file(TREE)
    seqs = random_columns(rng, list(util.read_fasta(MSA)), S, "ACGT", "RYKMSWBDHVN-")
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    ops, lengths = traverse(p, tree, tree.root_location(3).with_ratio(0.4))
    return p, tree, ops, lengths, seqs


@pytest.mark.parametrize("R", [4, 3])
def test_every_combination_of_null_outputs(R):
    p, tree, ops, lengths, _ = ten(R, 8)
    whole = p.branch_substitutions(ops, lengths, joint=True)
    keys = ("change", "count", "top_pair", "top_prob", "joint")
    fi = np.zeros(R, dtype=np.uint32)
    arr, n = rd.api._op_array(ops), len(ops)
    for wanted in itertools.product((False, True), repeat=5):
        out = {k: np.full_like(whole[k], 7) for k in keys}
        ptr = [(rd.api._dptr(out[k]) if k != "top_pair" else out[k].ctypes.data_as(rd.api._pub)) if use else None
               for k, use in zip(keys, wanted)]
        assert rd.lib.rdamd_branch_substitutions(p.handle, arr, n, rd.api._uptr(fi), rd.api._uptr(fi), rd.api._dptr(lengths),
                                                 *ptr) == 1, wanted
        for k, use in zip(keys, wanted):
            assert out[k].tobytes() == (whole[k] if use else np.full_like(whole[k], 7)).tobytes(), (wanted, k)


@pytest.mark.parametrize("R", [4, 3])
def test_two_calls_give_equal_bits_and_the_partition_is_only_read(R):
    p, tree, ops, lengths, _ = ten(R, 9, 300)
    root_clv = p.get_clv(tree.root_clv_index())
    pm = p.get_pmatrix(ops[0].child1_matrix_index)
    lnl = p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    a = p.branch_substitutions(ops, lengths, joint=True)
    assert rd.branch_substitutions_last_ms() > 0
    b = p.branch_substitutions(ops, lengths, joint=True)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert np.array_equal(p.get_clv(tree.root_clv_index()), root_clv)
    assert np.array_equal(p.get_pmatrix(ops[0].child1_matrix_index), pm)
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl


# ---- 6. refusals ---------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable():
    good, tree, ops, lengths, seqs = ten(4, 4)

    def valid_call():
        out = good.branch_substitutions(ops, lengths)
        assert all(np.all(np.isfinite(v)) for v in out.values()) and out["count"].max() > 0
        assert rd.branch_substitutions_last_ms() > 0

    def refused(code):
        assert rd.lib.rdamd_errno() == code and rd.branch_substitutions_last_ms() == 0
        valid_call()

    valid_call()
    w20 = synth.workload(10, 40, 20, 4, 78)
    t20 = rd.Tree.from_newick(w20["newick"])
    p20 = rd.Partition.for_tree(t20, 20, 40, 4, rd.ATTRIB_NONREV)
    util.load_tips(p20, t20, w20["seqs"], util.make_map(w20["alphabet"]))
    p20.set_subst_params(0, np.linspace(0.1, 1.9, 380))
    p20.set_frequencies(0, [0.05] * 20)
    p20.set_category_rates(rd.compute_gamma_cats(1.0, 4))
    ops20, lengths20 = traverse(p20, t20, t20.root_location(2))
    with pytest.raises(rd.RdamdError, match="rdamd_branch_substitutions: 20-state"):
        p20.branch_substitutions(ops20, lengths20)
    refused(63)
    rng = np.random.default_rng(4)
    sparse, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng, rd.ATTRIB_SPARSE_CLVS)
    sparse_ops, _ = traverse(sparse, tree, tree.root_location(3).with_ratio(0.4))
    with pytest.raises(rd.RdamdError, match="rdamd_branch_substitutions: .*SPARSE_CLVS"):
        sparse.branch_substitutions(sparse_ops, lengths)
    refused(63)
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    with pytest.raises(rd.RdamdError, match="root operation"):
        good.branch_substitutions(shuffled, lengths)
    refused(64)
    for bad in (-1e-3, np.inf, np.nan):
        wrong = lengths.copy()
        wrong[2, 1] = bad
        with pytest.raises(rd.RdamdError, match="negative or not finite"):
            good.branch_substitutions(ops, wrong)
        refused(64)
    fi = np.zeros(4, dtype=np.uint32)
    assert rd.lib.rdamd_branch_substitutions(good.handle, rd.api._op_array(ops), len(ops), rd.api._uptr(fi), rd.api._uptr(fi),
                                             None, None, None, None, None, None) != 1
    refused(64)
    with pytest.raises(rd.RdamdError, match="params index out of range"):
        good.branch_substitutions(ops, lengths, [0, 0, 1, 0], [0, 0, 0, 0])
    refused(7)
    with pytest.raises(rd.RdamdError, match="freqs index out of range"):
        good.branch_substitutions(ops, lengths, [0, 0, 0, 0], [0, 5, 0, 0])
    refused(7)
    # a column no history explains: two tips that differ, joined by two branches of length 0
    a, b = util.tip_tip_pair(tree, ops)
    dead = dict(seqs)
    dead[a], dead[b] = "A" + dead[a][1:], "C" + dead[a][1:]   # (the same everywhere else)
    p, _, _, _, _, _ = make_partition(tree, dead, rd.MAP_NT, 4, 4, rng)
    sched, pmi, brl = tree.generate_operations(tree.root_location(3).with_ratio(0.4))
    pair_op = next(o for o in sched if {o.child1_clv_index, o.child2_clv_index} == {tree.tip_index(a), tree.tip_index(b)})
    zero = [i for i, m in enumerate(pmi) if int(m) in (pair_op.child1_matrix_index, pair_op.child2_matrix_index)]
    dead_ops, dead_lengths = traverse(p, tree, tree.root_location(3).with_ratio(0.4), zero=zero)
    assert (dead_lengths == 0.0).sum() == 2
    with pytest.raises(rd.RdamdError, match="1 of 41 sites have a likelihood that is 0 or not finite"):
        p.branch_substitutions(dead_ops, dead_lengths)
    refused(65)


# ---- 7. the model --------------------------------------------------------------------------------
def test_site_group_model_is_refused():
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file_block(rd.Tree.from_file(TREE), MSA, 0, 2)
    m.set_lnl_reducer(lambda values, n: None)
    m.initialize_partitions()
    pp = {"subst_rates": [0.5] * 12, "freqs": [0.25] * 4, "gamma_alpha": [1.0], "gamma_weights": []}
    with pytest.raises(rd.RdamdError, match="site group"):
        m.substitutions(tree.root_location(0), [pp])
    assert rd.lib.rdamd_errno() == 61


def test_model_substitutions_equal_the_partitions_and_leave_the_model_as_it_was():
    packed, weights = util.compress(util.read_fasta(MSA))
    tree, t2 = rd.Tree.from_file(TREE), rd.Tree.from_file(TREE)
    m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
    m.initialize_partitions()
    rng = np.random.default_rng(5)
    pp = {"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
          "gamma_alpha": [0.6], "gamma_weights": []}
    rl, home = tree.root_location(3).with_ratio(0.27), tree.root_location(0).with_ratio(0.4)
    lh_home, root_home = m.compute_lh(home), m.compute_lh_root(home)
    freqs_before = m.partition_frequencies(0)
    out = m.substitutions(rl, [pp])
    # parameters, rooting and CLVs are bit for bit what they were
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home
    assert np.array_equal(m.partition_frequencies(0), freqs_before)
    again = m.substitutions(rl, [pp])
    assert all(np.asarray(out[k]).tobytes() == np.asarray(again[k]).tobytes() for k in out if k != "typed")
    assert out["typed"][0].tobytes() == again["typed"][0].tobytes()
    # the same through a partition set up as the model sets its own up
    p, f, rates, w = model_partition(t2, packed, weights, 4, pp)
    ops, lengths = traverse(p, t2, t2.root_location(3).with_ratio(0.27))
    clv, parent, children = rd.ancestral_nodes(ops)
    assert np.array_equal(out["node_clv"], clv) and np.array_equal(out["node_parent"], parent)
    assert np.array_equal(out["node_children"], children) and np.array_equal(out["lengths"], lengths)
    site = p.branch_substitutions(ops, lengths)
    for key in ("change", "top_prob"):
        assert np.abs(out[key] - site[key]).max() <= 1e-12
    assert np.all(np.abs(out["count"] - site["count"]) <= 1e-11 * site["count"])
    assert (out["top_pair"] != site["top_pair"]).mean() <= 0.01
    N, _, _ = p.branch_pair_sums(ops)
    typed = rd.substitution_counts(N, lengths, [pp["subst_rates"]], [f], [0] * 4, rates)
    assert len(out["typed"]) == 1 and out["typed"][0].shape == (9, 2, 4, 4)
    assert np.all(np.abs(out["typed"][0] - typed) <= 1e-11 * typed)
    assert util.rel_err(out["lnl"], p.compute_root_loglikelihood(t2.root_clv_index(), t2.root_scaler_index())) < 1e-12
    # identity A across the model's own outputs
    off = ~np.eye(4, dtype=bool)
    e_sum = out["typed"][0][:, :, off].sum(axis=2)
    assert np.all(np.abs((out["count"] * weights).sum(axis=2) - e_sum) <= 1e-11 * e_sum)
