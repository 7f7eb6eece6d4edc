"""The state-generic kernels between 3 and 64 states, and tables of state masks that are FULL.

include/root_digger_amd.h promises partitions of 2 to 64 states; the rest of the suite runs the
state-generic kernels (pmatrix_generic_kernel, tiptab_all_kernel, clv_generic_traversal_kernel, the
root reductions over K, the site-rate posteriors) at 5 states with 3 categories and at 20 with 16, and
never puts more than 22 distinct masks into a table of 64.  Here: 3, 7, 21 states, 45 and 46 (the
P-matrix kernel's 4 K^2 + K doubles of LDS pass 64 KB between them), 61 and 64 (codon models; at 64
the all-ones mask is ~0), every alignment with all 64 masks -- or 2^K - 1 -- in its cells
(util.full_table_map, util.place_characters), the highest codes at the two tips of a tip-tip step.

The reference is the CPU oracle, pinned at these sizes by tests/test_oracle_state_counts.py.
Tolerances are those of tests/test_gpu_parity.py: P 1e-13 absolute, non-negative, rows summing to 1
within 1e-12; CLVs rtol 1e-12, scalers bit-exact (compare_state); lnL 1e-11 relative."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
from oracle_lib import OraclePartition, ORC_MAP_NT
import util
from test_gpu_parity import compare_state, set_model, LNL_TOL, _oracle_eval
from test_gpu_root_children import _check_children

pytestmark = pytest.mark.gpu

STATE_COUNTS = [3, 7, 21, 45, 46, 61, 64]
S = 33          # one more than a multiple of 32
ODD20 = "".join(ch for ch in util.PRINTABLE if ch not in synth.AA)[:44]


def refused(errno, call, *args):
    """the call fails, with this error number"""
    with pytest.raises(rd.RdamdError):
        call(*args)
    assert rd.api._errno() == errno, (rd.api._errno(), errno)


def rate_model(rng, K, R):
    """(subst, freqs, rates, category weights) drawn as the oracle test draws them"""
    subst, freqs = util.mixture_params(rng, K, 1)
    rates = rd.compute_gamma_cats(0.7, R) if R > 1 else [1.0]
    weights = rng.dirichlet(np.ones(R) * 3)
    return subst[0], freqs[0], rates, weights


def partitions(tree, K, R, sites=S, attributes=0):
    """a device partition and an oracle one with room for the tree's own operation lists and for the
    all-directions schedule"""
    d = tree.generate_directional_operations()
    b = tree.branch_count()
    sizes = dict(tips=tree.tip_count(), clv_buffers=max(d["clv_buffers"], b), states=K, sites=sites, rate_matrices=1,
                 prob_matrices=max(d["prob_matrices"], b), rate_cats=R, scale_buffers=max(d["scale_buffers"], b))
    return rd.Partition(attributes=attributes, **sizes), OraclePartition(**sizes), d


def full_table_case(K, R, n, seed, plain=None, seqs=None, rooting=3):
    """tree of n tips, an alignment of S sites that fills the table of masks, both partitions loaded.
    -> dict"""
    rng = np.random.default_rng(seed)
    newick, _ = synth.random_tree(n, rng)
    tree = rd.Tree.from_newick(newick)
    labels = [tree.tip_label(i) for i in range(n)]
    used, odd, cmap = util.full_table_map(rng, K, plain)
    rl = tree.root_location(rooting).with_ratio(0.3)
    ops, pmi, brl = tree.generate_operations(rl)
    pair = util.tip_tip_pair(tree, ops)
    if seqs is None:
        seqs = {l: "".join(rng.choice(list(used), size=S)) for l in labels}
    seqs = util.odd_cells(rng, seqs, odd)
    late = min(len(odd) // 2, 22)
    seqs = util.place_characters(rng, seqs, used, odd, pair, late)
    # every mask of the table stands in a cell; the two tips of a tip-tip step carry the highest codes,
    # two of them at the same site
    codes, table = util.tip_codes(seqs, cmap)
    assert len(table) == min(64, 2 ** K - 1) and (1 << K) - 1 in table
    a, b = codes[pair[0]], codes[pair[1]]
    assert a.max() == len(table) - 1 and min(a[:late].min(), b[:late].min()) >= len(table) - late
    assert len(table) < 64 or min(a[:late].min(), b[:late].min()) >= 32
    g, o, d = partitions(tree, K, R)
    weights = rng.integers(1, 4, size=S).astype(np.uint32)
    util.load_tips(g, tree, seqs, cmap, weights)
    util.load_tips(o, tree, seqs, cmap, weights)
    subst, freqs, rates, cw = rate_model(rng, K, R)
    set_model((g, o), subst, freqs, rates, cw)
    return dict(rng=rng, newick=newick, tree=tree, seqs=seqs, cmap=cmap, g=g, o=o, d=d, rl=rl, subst=subst, freqs=freqs,
                rates=rates, cw=cw, pair=pair, table=table, used=used, odd=odd)


def check_pmatrices(g, o, indices):
    for m in indices:
        a, b = g.get_pmatrix(int(m)), o.get_pmatrix(int(m))
        assert np.max(np.abs(a - b)) < 1e-13, m
        assert np.all(a >= 0.0)
        assert np.allclose(a.sum(axis=2), 1.0, atol=1e-12)


def check_lnl(g, o, tree):
    """root lnL, single and per site"""
    a, pa = g.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)
    b, pb = o.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)
    assert np.isfinite(b) and b < 0
    assert util.rel_err(a, b) < LNL_TOL, (a, b)
    assert np.allclose(pa, pb, rtol=1e-12, atol=0.0)
    assert a == g.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    return a


# ---- 1. P-matrices and tip tables ---------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", STATE_COUNTS)
def test_prob_matrices_and_tip_tables(K, R):
    """every matrix at the branch lengths of test_gpu_parity.test_prob_matrices; then every row of two
    matrices' tip tables through one operation over two tips that between them show every code twice"""
    rng = np.random.default_rng(70 + K)
    nm = 37
    used, odd, cmap = util.full_table_map(rng, K)
    chars = used + odd
    sites = len(chars) + 1
    g = rd.Partition(5, 8, K, sites, 1, nm, R, 8)
    o = OraclePartition(5, 8, K, sites, 1, nm, R, 8)
    subst, freqs, rates, _ = rate_model(rng, K, R)
    set_model((g, o), subst, freqs, rates)
    idx = rng.permutation(nm).astype(np.uint32)
    bl = np.concatenate([[0.0, 1e-8, 1e-6, 25.0], rng.exponential(0.3, nm - 4)])
    g.update_prob_matrices(idx, bl)
    o.update_prob_matrices(idx, bl)
    check_pmatrices(g, o, range(nm))
    # (tip 1 shows the codes in the order the partition met them at tip 0, one step on; the last site
    # pairs the all-ones mask with itself)
    ones = odd[0]
    assert int(cmap[ord(ones)]) == (1 << K) - 1
    for p in (g, o):
        p.set_tip_states(0, cmap, chars + ones)
        p.set_tip_states(1, cmap, chars[1:] + chars[0] + ones)
    k = 4 + int(np.argmax(bl[4:]))      # (a branch of ordinary length and the one of 25)
    op = rd.Operation(5, 0, 0, int(idx[k]), rd.api.SCALE_BUFFER_NONE, 1, int(idx[3]), rd.api.SCALE_BUFFER_NONE)
    assert 0.1 < bl[k] < 5 and bl[3] == 25.0
    g.update_clvs([op])
    o.update_clvs([op])
    a, b = g.get_clv(5), o.get_clv(5)
    assert b.min() > 0.0
    assert np.allclose(a, b, rtol=1e-12, atol=0.0)
    assert np.array_equal(g.get_scaler(0), o.get_scaler(0))
    g.destroy()
    o.destroy()


# ---- 2. a full traversal with full code tables ----------------------------------------------------
@pytest.mark.parametrize("K,R,n", [(3, 3, 9), (7, 1, 11), (7, 3, 13), (21, 3, 10), (45, 1, 9), (46, 3, 12), (61, 3, 9),
                                   (64, 1, 13), (64, 3, 11)])
def test_full_traversal_with_a_full_code_table(K, R, n):
    c = full_table_case(K, R, n, 2000 + 10 * K + R)
    g, o, tree, rl, d = c["g"], c["o"], c["tree"], c["rl"], c["d"]
    ops, pmi, brl = tree.generate_operations(rl)
    for p in (g, o):
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
    check_pmatrices(g, o, pmi)
    compare_state(g, o, ops, tree)
    lnl = check_lnl(g, o, tree)

    # site-rate posteriors from the root CLV (the entry point takes every shape but the matrix-core layout)
    cat, mean = g.site_rate_posteriors(tree.root_clv_index(), tree.root_scaler_index())
    terms = np.asarray(c["cw"]) * (o.get_clv(tree.root_clv_index()) @ np.asarray(c["freqs"]))
    want_cat = terms / terms.sum(axis=1, keepdims=True)
    assert np.abs(cat - want_cat).max() < 1e-12 and np.abs(cat.sum(axis=1) - 1).max() < 1e-14
    assert np.abs(mean - want_cat @ np.asarray(c["rates"])).max() < 1e-12

    # what refuses this state count says so, with its documented number, and leaves the partition usable
    before = [g.get_clv(op.parent_clv_index) for op in ops]
    refused(40, g.schedule, ops, pmi, brl)
    refused(40, g.evaluate_batch, [], np.zeros((0, K * K - K)), np.zeros((0, K)))
    refused(50, g.evaluate_root_children, ops, pmi, brl, c["subst"], c["freqs"], c["rates"], c["cw"])
    refused(63, g.marginal_ancestral, ops)
    refused(63, g.branch_derivatives, ops)
    assert all(np.array_equal(g.get_clv(op.parent_clv_index), x) for op, x in zip(ops, before))
    assert util.compute_lh(g, tree, rl) == lnl

    # the one-launch root step takes its fallback (a P-matrix launch per position) and gives the three
    # calls' bits
    op, pmi2, _ = tree.generate_derivative_operations(rl)
    alphas = [0.3, 0.3 + 1e-8, 0.0, 1.0, 0.77]
    l1 = [rl.saved_brlen * a for a in alphas]
    l2 = [rl.saved_brlen * (1 - a) for a in alphas]
    g.profile_enable(True)
    g.profile_read()
    got = g.root_loglikelihood_fused(op, l1, l2)
    assert g.profile_read()["pmatrix"][1] == len(alphas)
    g.profile_enable(False)
    want = o.root_loglikelihood_fused(op, l1, l2)
    for a, b in zip(got, want):
        assert util.rel_err(a, b) < LNL_TOL
    assert util.rel_err(got[0], lnl) < 1e-13      # full == root-only (test/src/model.cpp:285-286)
    g.update_prob_matrices(pmi2, [l1[4], l2[4]])
    g.update_clvs([op])
    assert g.compute_root_loglikelihood(op.parent_clv_index, op.parent_scaler_index) == got[4]

    # move_root over every root position (compute_all_root_lh, src/model.cpp:1737-1746)
    util.compute_lh(g, tree, tree.root_location(0))
    util.compute_lh(o, tree, tree.root_location(0))
    t2 = rd.Tree.from_newick(c["newick"])
    t2.root_by(t2.root_location(0))
    for cand in tree.roots():
        util.move_root(g, tree, cand)
        a = util.compute_lh_root(g, tree, cand)
        util.move_root(o, t2, cand)
        b = util.compute_lh_root(o, t2, cand)
        assert util.rel_err(a, b) < LNL_TOL, (cand.edge if hasattr(cand, "edge") else None, a, b)

    # every root CLV of the all-directions schedule: the batched reduction and the single one
    for p in (g, o):
        p.update_prob_matrices(d["matrix_indices"], d["branch_lengths"])
        p.update_clvs(d["ops"])
    many = g.compute_root_loglikelihoods(d["root_clv"], d["root_scaler"])
    assert len(many) == tree.root_count()
    for rid in range(tree.root_count()):
        clv, sc = int(d["root_clv"][rid]), int(d["root_scaler"][rid])
        want = o.compute_root_loglikelihood(clv, sc)
        assert util.rel_err(many[rid], want) < LNL_TOL, rid
        assert util.rel_err(g.compute_root_loglikelihood(clv, sc), want) < LNL_TOL, rid
    g.destroy()
    o.destroy()


# ---- 3. rescaling at generic K ----------------------------------------------------------------------
@pytest.mark.parametrize("K,n", [(7, 150), (64, 64)])
def test_rescaling_on_a_deep_caterpillar(K, n):
    """a site loses about log2(K) binades per tip and more on long branches: the per-site 2^256 rule
    fires on the way up, and the scalers must be the oracle's bit for bit"""
    R = 3
    rng = np.random.default_rng(300 + K)
    used, odd, cmap = util.full_table_map(rng, K)
    names = ["q%03d" % i for i in range(n)]
    nw = names[0]
    for i in range(1, n - 2):
        nw = "(%s:0.8,%s:0.6)" % (nw, names[i])
    nw = "(%s:0.8,%s:0.6,%s:0.7);" % (nw, names[n - 2], names[n - 1])
    tree = rd.Tree.from_newick(nw)
    seqs = util.odd_cells(rng, {k: "".join(rng.choice(list(used), S)) for k in names}, odd, share=0.1)
    g, o = rd.Partition.for_tree(tree, K, S, R), OraclePartition.for_tree(tree, K, S, R)
    util.load_tips(g, tree, seqs, cmap)
    util.load_tips(o, tree, seqs, cmap)
    subst, freqs, rates, cw = rate_model(rng, K, R)
    set_model((g, o), subst, freqs, rates, cw)
    rl = tree.root_location(3).with_ratio(0.4)
    ops, pmi, brl = tree.generate_operations(rl)
    for p in (g, o):
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
    assert o.get_scaler(tree.root_scaler_index()).max() >= 1
    compare_state(g, o, ops, tree)
    check_lnl(g, o, tree)
    g.destroy()
    o.destroy()


# ---- 4. twenty states, 64 codes, on every 20-state route --------------------------------------------
def twenty(R, n, seed):
    w = synth.workload(n, S, 20, R, seed)
    c = full_table_case(20, R, n, seed, plain=synth.AA, seqs=w["seqs"])
    assert c["odd"] == ODD20 and len(c["table"]) == 64
    return c


@pytest.mark.parametrize("R,n", [(3, 11),      # the matrix-core traversal kernel
                                 (8, 9),       # its wide-workgroup variant
                                 (16, 13)])    # beyond it: the generic kernel
def test_twenty_states_full_table_traversal(R, n):
    c = twenty(R, n, 500 + R)
    g, o, tree, rl = c["g"], c["o"], c["tree"], c["rl"]
    ops, pmi, brl = tree.generate_operations(rl)
    for p in (g, o):
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
    check_pmatrices(g, o, pmi)
    compare_state(g, o, ops, tree)
    check_lnl(g, o, tree)
    g.destroy()
    o.destroy()


@pytest.mark.parametrize("R,n", [(1, 9), (4, 13), (5, 11)])
def test_twenty_states_full_table_fused_batch(R, n):
    """per-job parameters, rates and category weights; 33 sites leave the last tile ragged"""
    c = twenty(R, n, 520 + R)
    g, o, tree, rng = c["g"], c["o"], c["tree"], c["rng"]
    picks = rng.choice(tree.root_count(), size=5, replace=False)
    rls = [c["rl"]] + [tree.root_location(int(i)).with_ratio(float(rng.uniform(0.02, 0.98))) for i in picks]
    scheds = [g.schedule(*tree.generate_operations(rl)) for rl in rls]
    J = len(rls)
    subst = rng.uniform(1e-4, 1.0, (J, 380))
    freqs = rng.dirichlet(np.ones(20) * 10, J)
    rates = np.array([rd.compute_gamma_cats(a, R) if R > 1 else [1.0] for a in rng.uniform(0.3, 3.0, J)])
    cw = rng.dirichlet(np.ones(R) * 3, J)
    got = g.evaluate_batch(scheds, subst, freqs, rates, cw)
    for j, rl in enumerate(rls):
        want = _oracle_eval(o, tree, rl, subst[j], freqs[j], rates[j], cw[j])
        assert util.rel_err(got[j], want) < LNL_TOL, (j, got[j], want)
    assert np.array_equal(got, g.evaluate_batch(scheds, subst, freqs, rates, cw))
    g.destroy()
    o.destroy()


def test_twenty_states_full_table_root_children():
    c = twenty(4, 12, 540)
    g, o, tree = c["g"], c["o"], c["tree"]
    for rl in (c["rl"], tree.root_location(0).with_ratio(0.6), tree.root_location(tree.root_count() - 1).with_ratio(0.37)):
        _check_children(g, o, tree, rl, c["subst"], c["freqs"], c["rates"], c["cw"])
    g.destroy()
    o.destroy()


def test_twenty_states_full_table_site_lnls():
    """Model.site_lnls over the same alignment: per-pattern lnL of three roots at their own parameters,
    through the fixture of tests/test_gpu_site_lnls.py"""
    from test_gpu_site_lnls import check_single_partition
    c = twenty(3, 11, 560)
    c["g"].destroy()
    c["o"].destroy()
    check_single_partition(lambda: rd.Tree.from_newick(c["newick"]), c["seqs"], c["cmap"], c["cmap"], 20, 3, [3, 0, 12], 561)


# ---- 5. codes that arrive late, the table's end, refused calls -------------------------------------
def plain_case(K, R, n, seed, attributes=0, sites=S):
    """tree, a partition pair with plain tips only (K distinct masks), model set, the map of
    util.full_table_map at hand for what comes later"""
    rng = np.random.default_rng(seed)
    if K == 4:
        w = synth.workload(n, sites, 4, R, seed)
        tree = rd.Tree.from_newick(w["newick"])
        used, odd, cmap, ocmap, seqs = "ACGT", "RYKMSWBDHVN-", rd.MAP_NT, ORC_MAP_NT, w["seqs"]
    else:
        newick, _ = synth.random_tree(n, rng)
        tree = rd.Tree.from_newick(newick)
        used, odd, cmap = util.full_table_map(rng, K, synth.AA[:K])
        ocmap = cmap
        seqs = {tree.tip_label(i): "".join(rng.choice(list(used), size=sites)) for i in range(n)}
    g, o, _ = partitions(tree, K, R, sites, attributes)
    weights = rng.integers(1, 4, size=sites).astype(np.uint32)
    util.load_tips(g, tree, seqs, cmap, weights)
    util.load_tips(o, tree, seqs, ocmap, weights)
    subst, freqs, rates, cw = rate_model(rng, K, R)
    set_model((g, o), subst, freqs, rates, cw)
    return dict(rng=rng, tree=tree, seqs=seqs, cmap=cmap, ocmap=ocmap, g=g, o=o, used=used, odd=odd, subst=subst,
                freqs=freqs, rates=rates, cw=cw, weights=weights)


def with_characters(seq, chars, start):
    """seq with chars written over it from site `start` on"""
    return seq[:start] + chars + seq[start + len(chars):]


@pytest.mark.parametrize("K,R", [(20, 4), (5, 3)])
def test_codes_that_arrive_late(K, R):
    """Tip tables are built with the P-matrices, for the masks the partition knows then.  A sequence
    with new masks makes them stale; whatever reads them next rebuilds them first -- without any
    rdamd_update_prob_matrices in between but the two root matrices of a root-only step.

    A root-only step reads two CLVs and nothing else.  So the changed tip's characters reach
    (a) a traversal run again over matrices that were NOT refreshed (rdamd_update_clvs alone; the
        root-only steps at a root away from the tip follow it and read its CLVs), and
    (b) a root-only step on the changed tip's own branch, straight after the change.
    Every value is the oracle's for the same calls and differs from the value before the change."""
    c = plain_case(K, R, 10, 900 + K)
    g, o, tree, rng = c["g"], c["o"], c["tree"], c["rng"]
    tip = 4
    label = tree.tip_label(tip)
    inner = [rl for rl in tree.roots() if min(len(tree.side_tips(rl)), 10 - len(tree.side_tips(rl))) >= 3]
    far = inner[len(inner) // 2].with_ratio(0.35)
    near = next(rl for rl in tree.roots() if len(tree.side_tips(rl)) in (1, 9) and
                (label in tree.side_tips(rl)) == (len(tree.side_tips(rl)) == 1)).with_ratio(0.6)
    if K == 20:      # (compiled first: compiling roots the tree at its own location)
        rl_s = tree.root_location(5).with_ratio(0.45)
        sched = g.schedule(*tree.generate_operations(rl_s))
        params = ([c["subst"]], [c["freqs"]], [c["rates"]], [c["cw"]])
    far_ops, _, _ = tree.generate_operations(far)
    root_far = far_ops[len(far_ops) - 1]
    assert min(root_far.child1_clv_index, root_far.child2_clv_index) >= tree.tip_count()
    before = util.compute_lh(g, tree, far)
    assert util.rel_err(before, util.compute_lh(o, tree, far)) < LNL_TOL
    if K == 20:
        batch_before = g.evaluate_batch([sched], *params)[0]

    # (a) two masks the partition has not seen, at five sites of one tip
    odd = c["odd"]
    seq = with_characters(c["seqs"][label], odd[0] + odd[3] + odd[0] + odd[3] + odd[3], 7)
    g.set_tip_states(tip, c["cmap"], seq)
    o.set_tip_states(tip, c["cmap"], seq)
    for p in (g, o):
        p.update_clvs(far_ops)
    compare_state(g, o, far_ops, tree)
    after = check_lnl(g, o, tree)
    assert util.rel_err(after, before) > 1e-6
    a, b = util.compute_lh_root(g, tree, far), util.compute_lh_root(o, tree, far)
    assert util.rel_err(a, b) < LNL_TOL and util.rel_err(a, before) > 1e-6
    op, _, _ = tree.generate_derivative_operations(far)
    l1, l2 = [far.saved_brlen * x for x in (0.35, 0.8)], [far.saved_brlen * (1 - x) for x in (0.35, 0.8)]
    a, b = g.root_loglikelihood_fused(op, l1, l2), o.root_loglikelihood_fused(op, l1, l2)
    assert all(util.rel_err(x, y) < LNL_TOL for x, y in zip(a, b)) and util.rel_err(a[0], before) > 1e-6
    if K == 20:      # the SAME schedule: the evaluator builds its tables for the masks of now
        got = g.evaluate_batch([sched], *params)[0]
        o2 = OraclePartition.for_tree(tree, K, S, R)
        util.load_tips(o2, tree, dict(c["seqs"], **{label: seq}), c["cmap"], c["weights"])
        want = _oracle_eval(o2, tree, rl_s, c["subst"], c["freqs"], c["rates"], c["cw"])
        assert util.rel_err(got, want) < LNL_TOL, (got, want)
        assert util.rel_err(got, batch_before) > 1e-6
        o2.destroy()

    # (b) a full evaluation rooted on the tip's own branch, then two MORE new masks and the root-only step
    before = util.compute_lh(g, tree, near)
    assert util.rel_err(before, util.compute_lh(o, tree, near)) < LNL_TOL
    seq = with_characters(seq, odd[5] + odd[6] + odd[5], 20)
    g.set_tip_states(tip, c["cmap"], seq)
    o.set_tip_states(tip, c["cmap"], seq)
    # (the one-call root step FIRST: it is what meets the stale tables)
    op, _, _ = tree.generate_derivative_operations(near)
    l1, l2 = [near.saved_brlen * 0.25], [near.saved_brlen * 0.75]
    a, b = g.root_loglikelihood_fused(op, l1, l2), o.root_loglikelihood_fused(op, l1, l2)
    assert util.rel_err(a[0], b[0]) < LNL_TOL and util.rel_err(a[0], before) > 1e-6
    x, y = util.compute_lh_root(g, tree, near), util.compute_lh_root(o, tree, near)
    assert util.rel_err(x, y) < LNL_TOL and util.rel_err(x, before) > 1e-6
    # ... which is the full evaluation's value for that sequence
    near2 = near.with_ratio(0.25)
    assert util.rel_err(util.compute_lh(o, tree, near2), a[0]) < LNL_TOL
    g.destroy()
    o.destroy()


def snapshot(g, tree, rl):
    """everything a partition computes at rl, and the tips as it holds them: lnL, per-site values,
    every CLV and scaler"""
    ops, _, _ = tree.generate_operations(rl)
    lnl = util.compute_lh(g, tree, rl)
    _, persite = g.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index(), persite=True)
    out = [np.array([lnl]), persite] + [g.get_clv(i) for i in range(tree.tip_count())]
    for op in ops:
        out.append(g.get_clv(op.parent_clv_index))
        if op.parent_scaler_index >= 0:
            out.append(g.get_scaler(op.parent_scaler_index))
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("K,R", [(20, 4), (7, 3)])
def test_the_tables_end(K, R):
    """a 65th distinct mask is refused with error 5 and changes nothing; the same tip then takes a
    sequence within the 64"""
    c = full_table_case(K, R, 9, 1100 + K, plain=synth.AA[:K])
    g, o, tree, rl = c["g"], c["o"], c["tree"], c["rl"]
    assert len(c["table"]) == 64
    one_more = next(m for m in range(3, 1 << K) if m not in c["table"])
    extra = next(ch for ch in util.PRINTABLE if ch not in c["used"] + c["odd"])
    cmap = util.make_map(synth.AA[:K], dict({ch: int(c["cmap"][ord(ch)]) for ch in c["odd"]}, **{extra: one_more}))
    tip = tree.tip_index(c["pair"][0])
    label = tree.tip_label(tip)
    before = snapshot(g, tree, rl)
    want = util.compute_lh(o, tree, rl)
    assert util.rel_err(before[0][0], want) < LNL_TOL
    # (characters that differ from the tip's own in front of the one that is refused)
    seq = "".join(c["used"][(c["used"].index(ch) + 1) % len(c["used"])] if ch in c["used"] else c["used"][0]
                  for ch in c["seqs"][label])
    refused(5, g.set_tip_states, tip, cmap, with_characters(seq, extra, S - 2))
    assert same_bits(snapshot(g, tree, rl), before)
    seq = with_characters(seq, c["odd"][1] + c["odd"][-1], 3)
    g.set_tip_states(tip, cmap, seq)
    o.set_tip_states(tip, cmap, seq)
    a, b = util.compute_lh(g, tree, rl), util.compute_lh(o, tree, rl)
    assert util.rel_err(a, b) < LNL_TOL and util.rel_err(a, want) > 1e-6
    ops, _, _ = tree.generate_operations(rl)
    compare_state(g, o, ops, tree)
    g.destroy()
    o.destroy()


@pytest.mark.parametrize("K,R", [(4, 4), (20, 4), (5, 3)])
def test_a_refused_call_changes_nothing(K, R):
    """A sequence whose first characters differ from the tip's own -- outside DNA with a mask the table
    does not hold yet -- and whose last character has no entry in the map: error 4, and host and
    device stay as they were.  4 states run with site repeats: a schedule compiled after the refusal
    works its site classes out from the host's copy of the tips."""
    sites = 65
    c = plain_case(K, R, 12, 1200 + K, rd.ATTRIB_SITE_REPEATS if K == 4 else 0, sites)
    g, o, tree, used, odd = c["g"], c["o"], c["tree"], c["used"], c["odd"]
    rl = tree.root_location(4).with_ratio(0.45)
    tip, other = 2, 7
    label = tree.tip_label(tip)
    assert "~" not in used + odd and int(c["cmap"][ord("~")]) == 0
    before = snapshot(g, tree, rl)
    want = util.compute_lh(o, tree, rl)
    assert util.rel_err(before[0][0], want) < LNL_TOL
    if K == 4:
        args = tree.generate_operations(rl)
        job = ([c["subst"]], [c["freqs"]], [c["rates"]], [c["cw"]])
        batch_before = g.evaluate_batch([g.schedule(*args)], *job)[0]
        assert util.rel_err(batch_before, want) < LNL_TOL
    own = c["seqs"][label]
    bad = "".join(used[(used.index(ch) + 1) % len(used)] for ch in own[:40]) + odd[2] * 5 + own[45:sites - 1] + "~"
    assert len(bad) == sites and all(x != y for x, y in zip(bad[:45], own[:45]))
    refused(4, g.set_tip_states, tip, c["cmap"], bad)
    assert same_bits(snapshot(g, tree, rl), before)
    if K == 4:
        assert g.evaluate_batch([g.schedule(*args)], *job)[0] == batch_before
    # the same new mask, and no other, in a valid call at another tip: a table that had kept the mask
    # from the refused call would see nothing new here and send nothing to the device
    seq = with_characters(c["seqs"][tree.tip_label(other)], odd[2] * 5, 11)
    g.set_tip_states(other, c["cmap"], seq)
    o.set_tip_states(other, c["ocmap"], seq)
    a, b = util.compute_lh(g, tree, rl), util.compute_lh(o, tree, rl)
    assert util.rel_err(a, b) < LNL_TOL and util.rel_err(a, want) > 1e-6
    ops, _, _ = tree.generate_operations(rl)
    compare_state(g, o, ops, tree)
    if K == 4:
        assert util.rel_err(g.evaluate_batch([g.schedule(*args)], *job)[0], b) < LNL_TOL
    g.destroy()
    o.destroy()
