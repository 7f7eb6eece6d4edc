"""Ancestral sequences for protein data: the 20-state pre-order walk on the matrix cores
(csrc/kernels_preorder_k20.hip) through rdamd_ancestral_sequences, Partition.ancestral_sequences
and Model.ancestral_sequences -- and the 4-state and binary partitions through the same call.

The references are the NumPy restatements of tests/test_gpu_ancestral.py (K-generic): the exact
enumeration over all assignments of the inner nodes, and the recursion of
include/root_digger_amd.h.  They are fed the device's own P-matrices (exp(Qt) is not under test).
Models are UNREST with 380 random rates in [0.1, 1.5], Dirichlet frequencies and unequal category
weights: a symmetric model would hide a P / P^T mix-up in the transposed product.
Tolerances: 1e-12 on posteriors (the figure test_gpu_ancestral.py holds the 4-state pass to), 5e-11
on the deep caterpillar (that file's figure for its deep case), 1e-9 against a host matrix
exponential (that file's figure for the model)."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import util
from test_gpu_ancestral import (recursion, enumeration, caterpillar, tip_vectors, children_of, device_pmatrices,
                                check_nodes, expm, make_partition, traverse, random_columns)
from test_gpu_state_counts import full_table_case

pytestmark = pytest.mark.gpu

AA = synth.AA
AA_MAP = util.make_map(AA, {"-": (1 << 20) - 1, "X": (1 << 20) - 1, "B": (1 << 2) | (1 << 3), "Z": (1 << 5) | (1 << 6),
                            "J": (1 << 9) | (1 << 10)})
ODD = "XBZJ-"


def protein_partition(tree, seqs, R, rng, rate_matrices=1, cmap=AA_MAP):
    """a 20-state partition under random UNREST models -> (partition, freqs[rate_matrices][20], category weights)"""
    S = len(next(iter(seqs.values())))
    b = tree.branch_count()
    p = rd.Partition(tree.tip_count(), b, 20, S, rate_matrices, b, R, b, rd.ATTRIB_NONREV)
    util.load_tips(p, tree, seqs, cmap)
    freqs = []
    for m in range(rate_matrices):
        p.set_subst_params(m, rng.uniform(0.1, 1.5, 380))
        freqs.append(rng.dirichlet(np.ones(20) * 4))
        p.set_frequencies(m, freqs[-1])
    p.set_category_rates(np.array(rd.compute_gamma_cats(0.7, R)) if R > 1 else np.ones(1))
    w = rng.dirichlet(np.ones(R) * 3)
    p.set_category_weights(w)
    return p, freqs, w


def check_state_and_prob(state, prob, post):
    """the arg-max outputs are the table's own, bit for bit, the first of equals"""
    assert state.dtype == np.uint8 and state.shape == post.shape[:2] and prob.shape == post.shape[:2]
    assert np.array_equal(state, post.argmax(axis=2))
    assert prob.tobytes() == post.max(axis=2).tobytes()


# ---- 1. exact enumeration -------------------------------------------------------------------
FOUR = "((a:0.21,b:0.09):0.13,c:0.4,d:0.33);"


@pytest.mark.parametrize("R", [1, 4])
def test_posteriors_equal_the_exact_enumeration(R):
    rng = np.random.default_rng(2000 + R)
    tree = rd.Tree.from_newick(FOUR)
    seqs = random_columns(rng, "abcd", 17, AA, ODD)
    seqs = {l: s[:11] + "-" + s[12:] for l, s in seqs.items()}       # one column of gaps only
    p, freqs, w = protein_partition(tree, seqs, R, rng)
    ops = traverse(p, tree, tree.root_location(3).with_ratio(0.3))
    assert len(ops) == 3                                               # 20^3 = 8 000 assignments
    state, prob, post = p.ancestral_sequences(ops, posteriors=True)
    want, _ = enumeration(ops, 4, tip_vectors(tree, seqs, AA_MAP, 20), device_pmatrices(p, ops), freqs[0], w)
    print("enumeration, R %d: post %.3e, rows %.3e, gaps at the root %.3e" % (
        R, np.abs(post - want).max(), np.abs(post.sum(axis=2) - 1).max(), np.abs(post[0, 11] - freqs[0]).max()))
    assert post.shape == (3, 17, 20)
    assert np.abs(post - want).max() < 1e-12
    assert np.abs(post.sum(axis=2) - 1).max() < 1e-14
    assert np.abs(post[0, 11] - freqs[0]).max() < 1e-14
    check_state_and_prob(state, prob, post)


# ---- 2. lane map and slots ------------------------------------------------------------------
@pytest.fixture(scope="module")
def thirteen():
    rng = np.random.default_rng(13)
    newick, _ = synth.random_tree(13, rng)
    labels = ["t%04d" % i for i in range(13)]
    return newick, random_columns(rng, labels, 17, AA, ODD)


# (R = 5 and 8: the 512-thread instantiation)
@pytest.mark.parametrize("S,R", [(S, R) for S in (1, 15, 16, 17) for R in (1, 2, 3, 4, 5, 8)])
def test_shapes_around_the_lane_map(thirteen, S, R):
    newick, all_seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(1000 * S + R)
    p, freqs, w = protein_partition(tree, seqs, R, rng)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    state, prob, post = p.ancestral_sequences(ops, posteriors=True)
    want, _, _ = recursion(ops, 13, tip_vectors(tree, seqs, AA_MAP, 20), device_pmatrices(p, ops), freqs[0], w, normalise=True)
    print("S %d, R %d: post %.3e" % (S, R, np.abs(post - want).max()))
    assert post.shape == (12, S, 20)
    assert np.abs(post - want).max() < 1e-12
    check_state_and_prob(state, prob, post)


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 8])
def test_three_tiles_and_a_full_code_table(R):
    """S = 33: two full tiles and one site, all 64 codes of the table and the late codes in the cells"""
    case = full_table_case(20, R, 13, 3300 + R, plain=AA)
    p, tree, rng = case["g"], case["tree"], case["rng"]
    freqs, w = rng.dirichlet(np.ones(20) * 4), rng.dirichlet(np.ones(R) * 3)
    p.set_subst_params(0, rng.uniform(0.1, 1.5, 380))
    p.set_frequencies(0, freqs)
    p.set_category_weights(w)
    ops = traverse(p, tree, case["rl"])
    state, prob, post = p.ancestral_sequences(ops, posteriors=True)
    want, _, _ = recursion(ops, 13, tip_vectors(tree, case["seqs"], case["cmap"], 20), device_pmatrices(p, ops), freqs, w,
                           normalise=True)
    print("S 33, R %d, 64 codes: post %.3e" % (R, np.abs(post - want).max()))
    assert post.shape == (12, 33, 20) and len(case["table"]) == 64
    assert np.abs(post - want).max() < 1e-12
    check_state_and_prob(state, prob, post)


def test_balanced_tree_reads_parents_from_slots_registers_and_pi():
    rng = np.random.default_rng(16)
    tree = rd.Tree.from_newick(util.balanced_newick(16, rng))
    seqs = random_columns(rng, ["t%d" % i for i in range(16)], 17, AA, ODD)
    p, freqs, w = protein_partition(tree, seqs, 4, rng)
    ops = traverse(p, tree, tree.root_location(5).with_ratio(0.4))
    assert rd.ancestral_workspace_slots(ops, 16) >= 2
    state, prob, post = p.ancestral_sequences(ops, posteriors=True)
    want, _, _ = recursion(ops, 16, tip_vectors(tree, seqs, AA_MAP, 20), device_pmatrices(p, ops), freqs[0], w, normalise=True)
    print("balanced, 16 tips, %d slots: post %.3e" % (rd.ancestral_workspace_slots(ops, 16), np.abs(post - want).max()))
    assert np.abs(post - want).max() < 1e-12
    check_state_and_prob(state, prob, post)


# ---- 3. per-category frequency sets ---------------------------------------------------------
def test_frequency_set_per_category(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(303)
    p, freqs, w = protein_partition(tree, seqs, 3, rng, rate_matrices=2)
    fidx = [1, 0, 1]
    ops, pmi, brl = tree.generate_operations(tree.root_location(7).with_ratio(0.6))
    p.update_prob_matrices(pmi, brl, fidx)
    p.update_clvs(ops)
    _, _, post = p.ancestral_sequences(ops, freqs_indices=fidx, posteriors=True)
    _, _, same = p.ancestral_sequences(ops, freqs_indices=[0, 0, 0], posteriors=True)
    # the restatement with a frequency vector per category: U_root = pi of the category's set
    pmat, tipvec = device_pmatrices(p, ops), tip_vectors(tree, seqs, AA_MAP, 20)
    n, S, R = len(ops), 17, 3
    L, PL = {}, {}
    for o in ops:
        for c, m in children_of(o):
            v = np.broadcast_to(tipvec[c][:, None, :], (S, R, 20)) if c < 13 else L[c]
            PL[c] = np.einsum("rij,srj->sri", pmat[m], v)
        L[o.parent_clv_index] = PL[o.child1_clv_index] * PL[o.child2_clv_index]
    index_of = {ops[n - 1 - k].parent_clv_index: k for k in range(n)}
    U = {ops[-1].parent_clv_index: np.broadcast_to(np.stack([freqs[i] for i in fidx])[None], (S, R, 20))}
    want = np.zeros((n, S, 20))
    for k in range(n):
        o = ops[n - 1 - k]
        up = U[o.parent_clv_index]
        q = (w[None, :, None] * up * L[o.parent_clv_index]).sum(axis=1)
        want[k] = q / q.sum(axis=1, keepdims=True)
        (a, ma), (b, mb) = children_of(o)
        for c, m, sibling in ((a, ma, b), (b, mb, a)):
            if c >= 13:
                U[c] = np.einsum("sri,rij->srj", up * PL[sibling], pmat[m])
    print("frequency sets [1, 0, 1]: post %.3e, against [0, 0, 0] %.3e" % (np.abs(post - want).max(), np.abs(post - same).max()))
    assert np.abs(post - want).max() < 1e-12
    assert np.abs(post - same).max() > 1e-4


# ---- 4. depth -------------------------------------------------------------------------------
@pytest.mark.parametrize("deep_first", [True, False])
def test_deep_tree_needs_and_gets_the_rescale_rule(deep_first):
    rng = np.random.default_rng(300 + deep_first)
    newick, labels = caterpillar(299, deep_first, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 300
    seqs = {l: "".join(rng.choice(list(AA), size=17)) for l in labels}
    p, freqs, w = protein_partition(tree, seqs, 2, rng)
    ops = traverse(p, tree, tree.root_location("t299").with_ratio(0.5))   # the whole spine below one child
    assert len(ops) == 299
    state, prob, post = p.ancestral_sequences(ops, posteriors=True)
    tipvec, pmat = tip_vectors(tree, seqs, AA_MAP, 20), device_pmatrices(p, ops)
    # the case needs the rule: without any rescaling every column's root CLV is exactly zero
    with np.errstate(invalid="ignore", divide="ignore"):
        _, root_plain, _ = recursion(ops, 300, tipvec, pmat, freqs[0], w)
    assert np.all(root_plain == 0.0)
    want, _, _ = recursion(ops, 300, tipvec, pmat, freqs[0], w, normalise=True)
    assert np.all(np.isfinite(post))
    print("deep child first %s: largest difference %.3e" % (deep_first, np.abs(post - want).max()))
    assert np.abs(post - want).max() < 5e-11
    check_state_and_prob(state, prob, post)


# ---- 5. own consistency ---------------------------------------------------------------------
def test_two_calls_give_equal_bytes_and_the_partition_is_only_read(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    p, _, _ = protein_partition(tree, seqs, 4, np.random.default_rng(5))
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    inner = [o.parent_clv_index for o in ops]
    clvs = [p.get_clv(i) for i in inner]
    scalers = [p.get_scaler(o.parent_scaler_index) for o in ops if o.parent_scaler_index >= 0]
    lnl = p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    a = p.ancestral_sequences(ops, posteriors=True)
    b = p.ancestral_sequences(ops, posteriors=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    check_state_and_prob(*a)
    # without the table: the same states and probabilities
    state, prob = p.ancestral_sequences(ops)
    assert state.tobytes() == a[0].tobytes() and prob.tobytes() == a[1].tobytes()
    assert rd.ancestral_sequences_last_ms() > 0
    assert all(np.array_equal(p.get_clv(i), c) for i, c in zip(inner, clvs))
    assert all(np.array_equal(p.get_scaler(o.parent_scaler_index), s)
               for o, s in zip([o for o in ops if o.parent_scaler_index >= 0], scalers))
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl


# ---- 6. 4-state and binary partitions through the new call ----------------------------------
@pytest.mark.parametrize("states,R", [(4, 4), (4, 3), (2, 4), (2, 1)])
def test_dna_and_binary_partitions_through_the_new_call(states, R):
    rng = np.random.default_rng(60 + 10 * states + R)
    newick, _ = synth.random_tree(13, rng)
    tree = rd.Tree.from_newick(newick)
    labels = ["t%04d" % i for i in range(13)]
    if states == 4:
        cmap, seqs = rd.MAP_NT, random_columns(rng, labels, 37, "ACGT", "RYKMSWBDHVN-")
    else:
        cmap, seqs = rd.MAP_BIN, random_columns(rng, labels, 37, "01", "-")
    p, _, _, _ = make_partition(tree, seqs, cmap, states, R, rng)
    ops = traverse(p, tree, tree.root_location(7).with_ratio(0.6))
    old = p.marginal_ancestral(ops)
    state, prob, post = p.ancestral_sequences(ops, posteriors=True)
    assert post.shape == (12, 37, states) and post.tobytes() == old.tobytes()
    check_state_and_prob(state, prob, post)


# ---- 7. refusals ----------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable(thirteen):
    newick, seqs = thirteen
    tree = rd.Tree.from_newick(newick)
    rng = np.random.default_rng(7)
    good, _, _ = protein_partition(tree, seqs, 4, rng)
    rl = tree.root_location(7).with_ratio(0.6)
    ops = traverse(good, tree, rl)

    def valid_call():
        _, _, post = good.ancestral_sequences(ops, posteriors=True)
        assert np.abs(post.sum(axis=2) - 1).max() < 1e-14
        assert rd.ancestral_sequences_last_ms() > 0

    def refused(errno, match, call, *args, **kw):
        with pytest.raises(rd.RdamdError, match=match):
            call(*args, **kw)
        assert rd.lib.rdamd_errno() == errno and rd.ancestral_sequences_last_ms() == 0
        valid_call()

    valid_call()
    # sparse CLVs
    b = tree.branch_count()
    sparse = rd.Partition(13, b, 20, 17, 1, b, 4, b, rd.ATTRIB_NONREV | rd.ATTRIB_SPARSE_CLVS)
    util.load_tips(sparse, tree, seqs, AA_MAP)
    sparse_ops = traverse(sparse, tree, rl)
    refused(63, "SPARSE_CLVS", sparse.ancestral_sequences, sparse_ops)
    # 20 states in the plain CLV layout: 16 rate categories
    p16 = rd.Partition(13, b, 20, 17, 1, b, 16, b, rd.ATTRIB_NONREV)
    util.load_tips(p16, tree, seqs, AA_MAP)
    p16.set_category_rates(rd.compute_gamma_cats(1.0, 16))
    refused(63, "16 rate categories", p16.ancestral_sequences, traverse(p16, tree, rl))
    # 5 states
    p5 = rd.Partition(13, b, 5, 17, 1, b, 2, b, rd.ATTRIB_NONREV)
    util.load_tips(p5, tree, {l: "".join(AA[AA.index(ch) % 5] if ch in AA else "-" for ch in s) for l, s in seqs.items()},
                   util.make_map(AA[:5], {"-": 31}))
    refused(63, "5-state", p5.ancestral_sequences, traverse(p5, tree, rl))
    # a list that does not end in the root operation
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    refused(64, "root operation", good.ancestral_sequences, shuffled)
    # a frequency set the partition does not have
    refused(7, "freqs", good.ancestral_sequences, ops, freqs_indices=[0, 0, 1, 0])
    # the old entry point still refuses the 20-state partition
    with pytest.raises(rd.RdamdError, match="20-state"):
        good.marginal_ancestral(ops)
    assert rd.lib.rdamd_errno() == 63
    valid_call()
    assert np.isfinite(util.compute_lh(sparse, tree, rl)) and np.isfinite(util.compute_lh(p16, tree, rl))


# ---- 8. the model ---------------------------------------------------------------------------
def protein_restatement(tree, seqs, cmap, cats, rl, pp):
    """test_gpu_ancestral.model_restatement at 20 states: the parameters as model_t::set_model_params applies
    them (normalised frequencies, MEDIAN gamma rates, equal category weights), a host matrix exponential"""
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    q = synth.build_q(pp["subst_rates"], f)
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], cats, rd.GAMMA_RATES_MEDIAN))
    ops, pmi, brl = tree.generate_operations(rl)
    pmat = {m: np.stack([expm(q * r * t) for r in rates]) for m, t in zip(pmi, brl)}
    post, _, _ = recursion(ops, tree.tip_count(), tip_vectors(tree, seqs, cmap, 20), pmat, f, np.full(cats, 1.0 / cats))
    return ops, post


def test_model_ancestral_sequences_protein():
    wl = synth.workload(9, 120, 20, 4, 19)   # (every amino acid occurs: the model starts from empirical frequencies)
    cmap = util.make_map(wl["alphabet"])
    tree, t2 = rd.Tree.from_newick(wl["newick"]), rd.Tree.from_newick(wl["newick"])
    m = rd.Model(tree, wl["seqs"], states=20, cmap=cmap, rate_cats=4, seed=3)
    m.initialize_partitions()
    home = tree.root_location(0).with_ratio(0.4)
    lh_before, root_before = m.compute_lh(home), m.compute_lh_root(home)
    rng = np.random.default_rng(8)
    pp = {"subst_rates": rng.uniform(0.1, 1.5, 380).tolist(), "freqs": rng.dirichlet(np.ones(20) * 4).tolist(),
          "gamma_alpha": [0.6], "gamma_weights": []}
    rl = tree.root_location(3).with_ratio(0.27)
    node_clv, node_parent, node_children, state, prob, post = m.ancestral_sequences(rl, [pp], posteriors=True)
    ops, want = protein_restatement(t2, wl["seqs"], cmap, 4, rl, pp)
    print("protein model, 9 taxa: post %.3e" % np.abs(post - want).max())
    assert post.shape == (8, 120, 20)
    assert np.abs(post - want).max() < 1e-9
    check_state_and_prob(state, prob, post)
    check_nodes(t2, rl, ops, node_clv, node_parent, node_children)
    # parameters, rooting and the CLVs of that rooting are as before
    assert m.compute_lh_root(home) == root_before
    assert m.compute_lh(home) == lh_before
    # NULL parameters: the model's own (they are not the ones above)
    own = m.ancestral_sequences(rl, posteriors=True)
    assert len(own) == 6 and np.abs(own[5] - post).max() > 1e-3 and np.abs(own[5].sum(axis=2) - 1).max() < 1e-14
    assert len(m.ancestral_sequences(rl)) == 5


def test_model_dna_through_the_new_call_has_the_old_bits():
    tree = rd.Tree.from_file(util.DATA + "/10.tree")
    packed, weights = util.compress(util.read_fasta(util.DATA + "/10.fasta"))
    m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
    m.initialize_partitions()
    rl = tree.root_location(3).with_ratio(0.27)
    old = m.ancestral(rl)
    new = m.ancestral_sequences(rl, posteriors=True)
    assert all(np.array_equal(a, b) for a, b in zip(old[:3], new[:3]))
    assert new[5].tobytes() == old[3].tobytes()
    check_state_and_prob(new[3], new[4], new[5])
