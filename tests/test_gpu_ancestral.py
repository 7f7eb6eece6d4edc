"""Marginal ancestral states and site rates at a chosen root: the pre-order walk of
csrc/kernels_preorder.hip with its posterior consumer, through rdamd_marginal_ancestral /
rdamd_site_rate_posteriors, Model.ancestral and `rd_amd --ancestral --site-rates`.

The restatements are NumPy, in this file: an exact enumeration over all assignments of the inner
nodes (no pruning recursion at all), and the recursion of include/root_digger_amd.h (inner CLVs up,
outer vectors down), plain and with every vector renormalised by its largest entry."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import util

pytestmark = pytest.mark.gpu

ROOT = util.ROOT
RD = os.path.join(ROOT, "root_digger_amd", "bin", "rd_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
MSA = os.path.join(util.DATA, "10.fasta")
TREE = os.path.join(util.DATA, "10.tree")


# ---- restatements ------------------------------------------------------------------------
def tip_vectors(tree, seqs, cmap, K):
    """clv index -> [S][K] 0/1 code vectors"""
    out = {}
    for label, seq in seqs.items():
        out[tree.tip_index(label)] = np.array([[(cmap[ord(ch)] >> j) & 1 for j in range(K)] for ch in seq], dtype=np.float64)
    return out


def children_of(o):
    return ((o.child1_clv_index, o.child1_matrix_index), (o.child2_clv_index, o.child2_matrix_index))


def recursion(ops, tips, tipvec, pmat, pi, w, normalise=False):
    """post[n_ops][S][K] in the order of rdamd_marginal_ancestral (node k: the parent of ops[n-1-k]), the
    root CLV [S][R][K], and cat[S][R] / (unnormalised) per-rate site likelihoods.  normalise: every inner
    CLV and every outer vector divided by its largest entry over rates and states, per site."""
    n, K, R = len(ops), len(pi), len(w)
    S = next(iter(tipvec.values())).shape[0]
    L, PL = {}, {}

    def norm(v):
        return v / v.max(axis=(1, 2), keepdims=True) if normalise else v

    def clv(i):
        return np.broadcast_to(tipvec[i][:, None, :], (S, R, K)) if i < tips else L[i]

    for o in ops:
        for c, m in children_of(o):
            PL[c] = np.einsum("rij,srj->sri", pmat[m], clv(c))
        L[o.parent_clv_index] = norm(PL[o.child1_clv_index] * PL[o.child2_clv_index])
    index_of = {ops[n - 1 - k].parent_clv_index: k for k in range(n)}
    root = ops[-1].parent_clv_index
    U = {root: np.broadcast_to(np.asarray(pi)[None, None, :], (S, R, K))}
    post = np.zeros((n, S, K))

    def emit(c):
        q = (np.asarray(w)[None, :, None] * U[c] * L[c]).sum(axis=1)
        post[index_of[c]] = q / q.sum(axis=1, keepdims=True)

    emit(root)
    for k in range(n):
        o = ops[n - 1 - k]
        up = U.pop(o.parent_clv_index)
        (a, ma), (b, mb) = children_of(o)
        for c, m, sibling in ((a, ma, b), (b, mb, a)):
            if c >= tips:
                U[c] = norm(np.einsum("sri,rij->srj", up * PL[sibling], pmat[m]))
                emit(c)
    site_rate = np.asarray(w)[None, :] * (L[root] * np.asarray(pi)[None, None, :]).sum(axis=2)
    return post, L[root], site_rate


def enumeration(ops, tips, tipvec, pmat, pi, w):
    """The same outputs from the joint probability summed over ALL assignments of the inner nodes."""
    n, K, R = len(ops), len(pi), len(w)
    S = next(iter(tipvec.values())).shape[0]
    index_of = {ops[n - 1 - k].parent_clv_index: k for k in range(n)}
    tipfac = {}
    for o in ops:
        for c, m in children_of(o):
            if c < tips:
                tipfac[c] = np.einsum("rij,sj->sri", pmat[m], tipvec[c])   # [S][R][state of the parent]
    marg = np.zeros((n, S, R, K))
    like = np.zeros((S, R))
    for x in itertools.product(range(K), repeat=n):
        pr = np.full((S, R), pi[x[0]])
        for k in range(n):
            for c, m in children_of(ops[n - 1 - k]):
                pr = pr * (tipfac[c][:, :, x[k]] if c < tips else pmat[m][None, :, x[k], x[index_of[c]]])
        like += pr
        for k in range(n):
            marg[k, :, :, x[k]] += pr
    post = (np.asarray(w)[None, None, :, None] * marg).sum(axis=2)
    return post / post.sum(axis=2, keepdims=True), np.asarray(w)[None, :] * like


def cat_and_mean(site_rate, rates):
    cat = site_rate / site_rate.sum(axis=1, keepdims=True)
    return cat, cat @ np.asarray(rates)


# ---- the device side ----------------------------------------------------------------------
def make_partition(tree, seqs, cmap, states, R, rng, attrs=0):
    S = len(next(iter(seqs.values())))
    p = rd.Partition.for_tree(tree, states, S, R, rd.ATTRIB_NONREV | attrs)
    util.load_tips(p, tree, seqs, cmap)
    subst = rng.uniform(0.1, 1.5, states * states - states)          # UNREST: 12 free rates
    freqs = rng.dirichlet(np.ones(states) * 4)
    rates = np.array(rd.compute_gamma_cats(0.7, R)) if R > 1 else np.ones(1)
    w = rng.dirichlet(np.ones(R) * 3)                                  # unequal category weights
    p.set_subst_params(0, subst)
    p.set_frequencies(0, freqs)
    p.set_category_rates(rates)
    p.set_category_weights(w)
    return p, freqs, rates, w


def traverse(p, tree, rl):
    ops, pmi, brl = tree.generate_operations(rl)
    p.update_prob_matrices(pmi, brl)
    p.update_clvs(ops)
    return ops


def device_pmatrices(p, ops):
    """the device's own P-matrices: exp(Qt) is not under test here"""
    return {m: p.get_pmatrix(m) for o in ops for _, m in children_of(o)}


def random_columns(rng, labels, S, alphabet, odd):
    seqs = {l: "".join(rng.choice(list(alphabet), size=S)) for l in labels}
    for l in labels:   # ambiguity codes and gaps in a fifth of the cells
        s = list(seqs[l])
        for i in np.flatnonzero(rng.random(S) < 0.2):
            s[i] = odd[int(rng.integers(len(odd)))]
        seqs[l] = "".join(s)
    return seqs


# ---- 1. exact enumeration -------------------------------------------------------------------
FIVE = "((a:0.21,b:0.09):0.13,c:0.4,(d:0.05,e:0.33):0.27);"


@pytest.mark.parametrize("states,R", [(4, 4), (4, 1), (2, 4), (2, 1)])
def test_posteriors_equal_the_exact_enumeration(states, R):
    rng = np.random.default_rng(100 * states + R)
    tree = rd.Tree.from_newick(FIVE)
    labels = "abcde"
    if states == 4:
        cmap, seqs = rd.MAP_NT, random_columns(rng, labels, 37, "ACGT", "RYKMSWBDHVN-")
    else:
        cmap, seqs = rd.MAP_BIN, random_columns(rng, labels, 37, "01", "-")
    seqs = {l: s[:20] + "-" + s[21:] for l, s in seqs.items()}       # one column of gaps only
    p, pi, rates, w = make_partition(tree, seqs, cmap, states, R, rng)
    weights = rng.integers(1, 3, 37).astype(np.uint32)
    weights[[3, 20]] = 0
    weights[[7, 30]] = 3
    p.set_pattern_weights(weights)
    rl = tree.root_location(5).with_ratio(0.3)
    ops = traverse(p, tree, rl)
    assert len(ops) == 4
    post = p.marginal_ancestral(ops)
    cat, mean = p.site_rate_posteriors(tree.root_clv_index(), tree.root_scaler_index())

    tipvec = tip_vectors(tree, seqs, cmap, states)
    want, site_rate = enumeration(ops, 5, tipvec, device_pmatrices(p, ops), pi, w)
    want_cat, want_mean = cat_and_mean(site_rate, rates)
    print("states %d, R %d: post %.3e, rows %.3e, cat %.3e, mean %.3e" % (
        states, R, np.abs(post - want).max(), np.abs(post.sum(axis=2) - 1).max(), np.abs(cat - want_cat).max(),
        np.abs(mean - want_mean).max()))
    assert post.shape == (4, 37, states)
    assert np.abs(post - want).max() < 1e-12
    assert np.abs(post.sum(axis=2) - 1).max() < 1e-14
    assert np.abs(cat - want_cat).max() < 1e-12 and np.abs(cat.sum(axis=1) - 1).max() < 1e-14
    assert np.abs(mean - want_mean).max() < 1e-12
    # the column of gaps: the prior carried down the tree, the prior itself at the root
    assert np.abs(post[0, 20] - pi).max() < 1e-14
    # either output of the site-rate call may be left out
    fi = np.zeros(R, dtype=np.uint32)
    only = np.zeros(37)
    assert rd.lib.rdamd_site_rate_posteriors(p.handle, tree.root_clv_index(), -1, rd.api._uptr(fi), None, rd.api._dptr(only)) == 1
    assert np.array_equal(only, mean)


# ---- 2. shapes around the lane map ----------------------------------------------------------
@pytest.fixture(scope="module")
def thirty_three():
    rng = np.random.default_rng(33)
    newick, _ = synth.random_tree(33, rng)
    labels = ["t%04d" % i for i in range(33)]
    return newick, random_columns(rng, labels, 67, "ACGT", "RYN-")


@pytest.fixture(scope="module")
def thirty_three_wide(thirty_three):
    """the same tree with 300 columns: two workgroups of the lane-per-site walk"""
    labels = ["t%04d" % i for i in range(33)]
    return thirty_three[0], random_columns(np.random.default_rng(300), labels, 300, "ACGT", "RYN-")


# (300, 3): the generic walk in two workgroups, the second with 44 live lanes, parents from slots
@pytest.mark.parametrize("S,R", [(S, R) for S in (1, 15, 67) for R in (1, 2, 4, 8, 3)] + [(300, 3)])
def test_shapes_around_the_lane_map(thirty_three, thirty_three_wide, S, R):
    newick, all_seqs = thirty_three if S <= 67 else thirty_three_wide
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(1000 * S + R)
    p, pi, rates, w = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    rl = tree.root_location(17).with_ratio(0.6)
    ops = traverse(p, tree, rl)
    # parents come from the workspace as well as from registers
    assert rd.ancestral_workspace_slots(ops, 33) >= 1
    inner = [o.parent_clv_index for o in ops]
    before = [p.get_clv(i) for i in inner]
    lnl_before = p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    post = p.marginal_ancestral(ops)
    cat, mean = p.site_rate_posteriors(tree.root_clv_index(), tree.root_scaler_index())
    # the call writes nothing into the partition
    assert all(np.array_equal(p.get_clv(i), b) for i, b in zip(inner, before))
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl_before

    want, _, site_rate = recursion(ops, 33, tip_vectors(tree, seqs, rd.MAP_NT, 4), device_pmatrices(p, ops), pi, w)
    want_cat, want_mean = cat_and_mean(site_rate, rates)
    print("S %d, R %d: post %.3e, cat %.3e" % (S, R, np.abs(post - want).max(), np.abs(cat - want_cat).max()))
    assert post.shape == (32, S, 4)
    assert np.abs(post - want).max() < 1e-12
    assert np.abs(cat - want_cat).max() < 1e-12 and np.abs(mean - want_mean).max() < 1e-12


def test_two_calls_give_equal_bytes(thirty_three):
    newick, seqs = thirty_three
    tree = rd.Tree.from_newick(newick)
    p, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, np.random.default_rng(4))
    ops = traverse(p, tree, tree.root_location(17).with_ratio(0.6))
    a = p.marginal_ancestral(ops)
    b = p.marginal_ancestral(ops)
    assert a.shape == (32, 67, 4) and a.tobytes() == b.tobytes()


# ---- 3. depth -------------------------------------------------------------------------------
def caterpillar(n, deep_first, rng):
    """an n-tip caterpillar; the deep child is child 1 (deep_first) or child 2 of every spine node"""
    def length():
        return "%.6f" % rng.uniform(0.02, 0.3)
    spine = "(t0:%s,t1:%s)" % (length(), length())
    for i in range(2, n - 1):
        tip = "t%d:%s" % (i, length())
        deep = "%s:%s" % (spine, length())
        spine = "(%s,%s)" % ((deep, tip) if deep_first else (tip, deep))
    # unrooted at the top: the spine, and two tips
    return "(%s:%s,t%d:%s,t%d:%s);" % (spine, length(), n - 1, length(), n, length()), ["t%d" % i for i in range(n + 1)]


# (R = 3: the generic walk under the rule)
@pytest.mark.parametrize("deep_first,R", [pytest.param(True, 2, id="True"), pytest.param(False, 2, id="False"),
                                          pytest.param(True, 3, id="True-R3"), pytest.param(False, 3, id="False-R3")])
def test_deep_tree_needs_and_gets_the_rescale_rule(deep_first, R):
    rng = np.random.default_rng(800 + deep_first)
    newick, labels = caterpillar(799, deep_first, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 800
    seqs = {l: "".join(rng.choice(list("ACGT"), size=8)) for l in labels}
    p, pi, rates, w = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    # root on the branch of the last tip: the whole spine hangs below one child
    rl = tree.root_location("t799").with_ratio(0.5)
    ops = traverse(p, tree, rl)
    assert len(ops) == 799
    post = p.marginal_ancestral(ops)
    tipvec = tip_vectors(tree, seqs, rd.MAP_NT, 4)
    pmat = device_pmatrices(p, ops)
    # the case needs the rule: without any rescaling every column's root CLV is exactly zero
    with np.errstate(invalid="ignore", divide="ignore"):
        _, root_plain, _ = recursion(ops, 800, tipvec, pmat, pi, w)
    assert np.all(root_plain == 0.0)
    want, _, _ = recursion(ops, 800, tipvec, pmat, pi, w, normalise=True)
    assert np.all(np.isfinite(post))
    print("deep child first %s, R %d: largest difference %.3e" % (deep_first, R, np.abs(post - want).max()))
    assert np.abs(post - want).max() < 5e-11
    assert np.abs(post.sum(axis=2) - 1).max() < 1e-13


# ---- 4. refusals ----------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable():
    rng = np.random.default_rng(4)
    tree = rd.Tree.from_file(TREE)
    seqs = util.read_fasta(MSA)
    good, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng)
    rl = tree.root_location(3).with_ratio(0.4)
    ops = traverse(good, tree, rl)

    def valid_call():
        post = good.marginal_ancestral(ops)
        assert np.abs(post.sum(axis=2) - 1).max() < 1e-14
        assert rd.ancestral_last_ms() > 0

    valid_call()
    # 20 states
    w20 = synth.workload(10, 40, 20, 4, 78)
    t20 = rd.Tree.from_newick(w20["newick"])
    cmap = util.make_map(w20["alphabet"])
    p20 = rd.Partition.for_tree(t20, 20, 40, 4, rd.ATTRIB_NONREV)
    util.load_tips(p20, t20, w20["seqs"], cmap)
    p20.set_subst_params(0, np.linspace(0.1, 1.9, 380))
    p20.set_frequencies(0, [0.05] * 20)
    p20.set_category_rates(rd.compute_gamma_cats(1.0, 4))
    ops20 = traverse(p20, t20, t20.root_location(2))
    with pytest.raises(rd.RdamdError, match="20-state"):
        p20.marginal_ancestral(ops20)
    assert rd.lib.rdamd_errno() == 63 and rd.ancestral_last_ms() == 0
    valid_call()
    # sparse CLVs
    sparse, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng, rd.ATTRIB_SPARSE_CLVS)
    sparse_ops = traverse(sparse, tree, rl)
    with pytest.raises(rd.RdamdError, match="SPARSE_CLVS"):
        sparse.marginal_ancestral(sparse_ops)
    assert rd.lib.rdamd_errno() == 63
    valid_call()
    # a list that does not end in the root operation
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    with pytest.raises(rd.RdamdError, match="root operation"):
        good.marginal_ancestral(shuffled)
    assert rd.lib.rdamd_errno() == 64
    with pytest.raises(rd.RdamdError):
        rd.ancestral_nodes(shuffled)
    valid_call()
    # a model that sums over a site group
    m = rd.Model.from_file_block(rd.Tree.from_file(TREE), MSA, 0, 2)
    m.set_lnl_reducer(lambda values, n: None)
    m.initialize_partitions()
    with pytest.raises(rd.RdamdError, match="site group"):
        m.ancestral(tree.root_location(0))
    assert rd.lib.rdamd_errno() == 61
    valid_call()
    # ... and the partitions still evaluate (no HIP error was left behind)
    assert np.isfinite(util.compute_lh(p20, t20, t20.root_location(2)))
    assert np.isfinite(util.compute_lh(sparse, tree, rl))


# ---- 5. the model ---------------------------------------------------------------------------
def expm(a):
    """exp(a) by scaling and squaring of a Taylor series"""
    n = max(0, int(np.ceil(np.log2(max(np.abs(a).sum(axis=1).max(), 1e-300) / 0.125))))
    x, out, term = a / 2.0 ** n, np.eye(a.shape[0]), np.eye(a.shape[0])
    for k in range(1, 24):
        term = term @ x / k
        out = out + term
    for _ in range(n):
        out = out @ out
    return out


def model_restatement(tree, seqs, cmap, cats, rl, pp):
    """the parameters applied as model_t::set_model_params applies them (normalised frequencies, MEDIAN
    gamma rates, equal category weights), P-matrices by a host matrix exponential"""
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    q = synth.build_q(pp["subst_rates"], f)
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], cats, rd.GAMMA_RATES_MEDIAN)) if cats > 1 else np.ones(1)
    w = np.full(cats, 1.0 / cats)
    ops, pmi, brl = tree.generate_operations(rl)
    pmat = {m: np.stack([expm(q * r * t) for r in rates]) for m, t in zip(pmi, brl)}
    post, _, site_rate = recursion(ops, tree.tip_count(), tip_vectors(tree, seqs, cmap, 4), pmat, f, w)
    return (ops, post) + cat_and_mean(site_rate, rates)


def tips_below(clv, node_clv, node_children, tree):
    index = {int(c): k for k, c in enumerate(node_clv)}
    if clv not in index:
        return [tree.tip_label(clv)]
    a, b = node_children[index[clv]]
    return sorted(tips_below(int(a), node_clv, node_children, tree) + tips_below(int(b), node_clv, node_children, tree))


def check_nodes(tree, rl, ops, node_clv, node_parent, node_children):
    n = len(ops)
    assert list(node_clv) == [ops[n - 1 - k].parent_clv_index for k in range(n)] and node_parent[0] == -1
    for k in range(n):
        assert list(node_children[k]) == [ops[n - 1 - k].child1_clv_index, ops[n - 1 - k].child2_clv_index]
        for c in node_children[k]:
            if c >= tree.tip_count():
                assert node_parent[list(node_clv).index(c)] == k
    sides = [tips_below(int(c), node_clv, node_children, tree) for c in node_children[0]]
    assert tree.side_tips(rl) in sides
    assert sorted(sides[0] + sides[1]) == sorted(tree.tip_label(i) for i in range(tree.tip_count()))


def test_model_ancestral_ten_taxa():
    tree, t2 = rd.Tree.from_file(TREE), rd.Tree.from_file(TREE)
    packed, weights = util.compress(util.read_fasta(MSA))
    m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
    m.initialize_partitions()
    home = tree.root_location(0).with_ratio(0.4)
    lh_before, root_before = m.compute_lh(home), m.compute_lh_root(home)
    rng = np.random.default_rng(5)
    pp = {"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
          "gamma_alpha": [0.6], "gamma_weights": []}
    rl = tree.root_location(3).with_ratio(0.27)
    node_clv, node_parent, node_children, post, cat, mean = m.ancestral(rl, [pp])
    ops, want, want_cat, want_mean = model_restatement(t2, packed, rd.MAP_NT, 4, rl, pp)
    print("10 taxa: post %.3e, cat %.3e, mean %.3e" % (np.abs(post - want).max(), np.abs(cat - want_cat).max(),
                                                      np.abs(mean - want_mean).max()))
    assert post.shape == (9, len(weights), 4) and cat.shape == (len(weights), 4)
    assert np.abs(post - want).max() < 1e-9
    assert np.abs(cat - want_cat).max() < 1e-9 and np.abs(mean - want_mean).max() < 1e-9
    check_nodes(t2, rl, ops, node_clv, node_parent, node_children)
    # parameters, rooting and the CLVs of that rooting are as before
    assert m.compute_lh_root(home) == root_before
    assert m.compute_lh(home) == lh_before
    # NULL parameters: the model's own (they are not the ones above)
    post_own = m.ancestral(rl)[3]
    assert np.abs(post_own - post).max() > 1e-3 and np.abs(post_own.sum(axis=2) - 1).max() < 1e-14


def test_model_ancestral_two_partitions(tmp_path):
    phy, tre = os.path.join(util.DATA, "101.phy"), os.path.join(util.DATA, "101.tree")
    lines = ["UNREST+G4, first = 1-60", "UNREST, second = 61-100, 900-920"]
    pf = tmp_path / "parts.txt"
    pf.write_text("\n".join(lines) + "\n")
    tree, t2 = rd.Tree.from_file(tre), rd.Tree.from_file(tre)
    m = rd.Model.from_partition_file(tree, phy, str(pf), seed=3)
    m.initialize_partitions()
    compressed, _, _ = rd.msa_pattern_probe(phy, lines)
    names = list(util.read_phylip(phy))
    sizes = [n for n, _ in rd.msa_partition_probe(phy, lines)]
    assert [m.partition_shape(p)[0] for p in range(2)] == sizes and [m.partition_shape(p)[2] for p in range(2)] == [4, 1]
    home = tree.root_location(11).with_ratio(0.3)
    lh_before, root_before = m.compute_lh(home), m.compute_lh_root(home)
    rng = np.random.default_rng(9)
    sets = [{"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
             "gamma_alpha": [float(rng.uniform(0.3, 3.0))], "gamma_weights": []} for _ in range(2)]
    rl = tree.root_location(3).with_ratio(0.7)
    node_clv, node_parent, node_children, post, cat, mean = m.ancestral(rl, sets)
    assert post.shape == (100, sum(sizes), 4) and [c.shape for c in cat] == [(sizes[0], 4), (sizes[1], 1)]
    at = 0
    for p, (size, cats) in enumerate(zip(sizes, (4, 1))):
        seqs = {k: s[at:at + size] for k, s in zip(names, compressed)}
        ops, want, want_cat, want_mean = model_restatement(t2, seqs, rd.MAP_NT, cats, rl, sets[p])
        assert np.abs(post[:, at:at + size] - want).max() < 1e-9
        assert np.abs(cat[p] - want_cat).max() < 1e-9 and np.abs(mean[at:at + size] - want_mean).max() < 1e-9
        at += size
    check_nodes(t2, rl, ops, node_clv, node_parent, node_children)
    assert m.compute_lh_root(home) == root_before
    assert m.compute_lh(home) == lh_before


# ---- 6. the command line ----------------------------------------------------------------------
def _run(args):
    return subprocess.run([RD] + args, capture_output=True, text=True, timeout=600)


def test_rd_amd_ancestral_and_site_rates(tmp_path):
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--silent", "--rate-cats", "4",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(REF):
        common += ["--lbfgsb", REF]
    prefix, plain = str(tmp_path / "anc"), str(tmp_path / "plain")
    out = _run(common + ["--prefix", prefix, "--ancestral", "--site-rates"])
    assert out.returncode == 0, out.stdout + out.stderr
    records = rd.Checkpoint(prefix).read_results()
    best = max(range(len(records)), key=lambda i: (records[i][1], -i))   # the first maximum
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=4, seed=5)
    m.initialize_partitions()
    _, pattern_of = m.site_patterns()
    rl = tree.root_location(records[best][0]).with_ratio(records[best][2])
    node_clv, _, _, post, cat, mean = m.ancestral(rl, records[best][3])

    rows = [l.split("\t") for l in open(prefix + ".ancestral.tsv").read().splitlines()]
    assert rows[0] == ["node", "partition", "column", "state", "p_A", "p_C", "p_G", "p_T"]
    assert len(rows) - 1 == 9 * 1000
    for i, r in enumerate(rows[1:]):
        k, c = divmod(i, 1000)
        probs = [float(x) for x in r[4:]]
        assert r[0] == "N%d" % k and r[1] == "0" and int(r[2]) == c + 1
        assert abs(sum(probs) - 1.0) <= 5e-6
        assert r[4:] == ["%.6f" % v for v in post[k, pattern_of[c]]]
        if probs.count(max(probs)) == 1:
            assert r[3] == "ACGT"[probs.index(max(probs))]
    nw = open(prefix + ".ancestral.tree").read()
    named = rd.Tree.from_newick(nw)
    assert named.tip_count() == 10 and all(")N%d" % k in nw for k in range(9))
    tree.root_by(rl)
    assert nw == tree.newick_ancestral(node_clv)

    rates = [l.split("\t") for l in open(prefix + ".siterates.tsv").read().splitlines()]
    assert rates[0] == ["partition", "column", "mean_rate", "category", "p_1", "p_2", "p_3", "p_4"] and len(rates) == 1001
    for c, r in enumerate(rates[1:]):
        assert r[0] == "0" and int(r[1]) == c + 1
        assert r[2] == "%.6f" % mean[pattern_of[c]] and r[4:] == ["%.6f" % v for v in cat[pattern_of[c]]]
        probs = [float(x) for x in r[4:]]
        if probs.count(max(probs)) == 1:
            assert int(r[3]) == probs.index(max(probs)) + 1

    # the same run without the two options: every shared output byte for byte, nothing new
    out2 = _run(common + ["--prefix", plain])
    assert out2.returncode == 0, out2.stdout + out2.stderr
    assert out2.stdout == out.stdout
    made = sorted(f[len("anc"):] for f in os.listdir(tmp_path) if f.startswith("anc"))
    shared = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain"))
    assert sorted(set(made) - set(shared)) == [".ancestral.tree", ".ancestral.tsv", ".siterates.tsv"]
    for ext in shared:
        if ext != ".ckp":   # (the checkpoint's header holds the prefix)
            assert open(plain + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    assert ".lwr.tree" in shared and ".rooted.tree" in shared


@pytest.mark.parametrize("option", ["--ancestral", "--site-rates"])
@pytest.mark.parametrize("extra", [["--exhaustive", "--site-shards", "2"], ["--exhaustive", "--no-checkpoint"], []],
                         ids=["site-shards", "no-checkpoint", "heuristic"])
def test_rd_amd_refuses_ancestral_where_it_cannot_work(tmp_path, option, extra):
    prefix = str(tmp_path / "no")
    out = _run(["--msa", MSA, "--tree", TREE, "--silent", "--prefix", prefix, option] + extra)
    assert out.returncode != 0
    assert option in out.stdout + out.stderr
    assert not os.path.exists(prefix + ".ancestral.tsv") and not os.path.exists(prefix + ".siterates.tsv")
