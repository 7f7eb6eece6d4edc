"""Analytic branch-length derivatives and optimised lengths at a chosen root: the pre-order walk of
csrc/kernels_preorder.hip with its derivative consumer, through rdamd_branch_derivatives, Model.branch_derivatives, Model.optimize_branch_lengths and
`rd_amd --branch-lengths`.

The restatement is tests/brlen_ref.py (NumPy, every vector renormalised per site).  Device sums are
compared with it at |d - d_ref| <= 1e-11 A, A the absolute-value companion of the sum: the rounding
error of a sum of S <= 20 000 terms is a small multiple of 2^-53 S A, three or more orders below."""
import os
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import util
from test_gpu_ancestral import caterpillar, random_columns

pytestmark = pytest.mark.gpu

ROOT = util.ROOT
RD = os.path.join(ROOT, "root_digger_amd", "bin", "rd_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
MSA = os.path.join(util.DATA, "10.fasta")
TREE = os.path.join(util.DATA, "10.tree")
TOL = 1e-11


def make_partition(tree, seqs, cmap, states, R, rng, attrs=0, rate_matrices=1):
    """-> partition, subst[m], freqs[m], rates, category weights, pattern weights (0 to 3)"""
    S = len(next(iter(seqs.values())))
    b = tree.branch_count()
    p = rd.Partition(tree.tip_count(), b, states, S, rate_matrices, b, R, b, rd.ATTRIB_NONREV | attrs)
    util.load_tips(p, tree, seqs, cmap)
    subst = [rng.uniform(0.1, 1.5, states * states - states) for _ in range(rate_matrices)]   # UNREST
    freqs = [rng.dirichlet(np.ones(states) * 4) for _ in range(rate_matrices)]
    rates = np.array(rd.compute_gamma_cats(0.7, R)) if R > 1 else np.ones(1)
    w = rng.dirichlet(np.ones(R) * 3)
    for m in range(rate_matrices):
        p.set_subst_params(m, subst[m])
        p.set_frequencies(m, freqs[m])
    p.set_category_rates(rates)
    p.set_category_weights(w)
    weights = rng.integers(0, 4, S).astype(np.uint32)
    weights[0] = 2   # (a single column counts)
    p.set_pattern_weights(weights)
    return p, subst, freqs, rates, w, weights


def traverse(p, tree, rl, params_indices=None):
    ops, pmi, brl = tree.generate_operations(rl)
    p.update_prob_matrices(pmi, brl, params_indices)
    p.update_clvs(ops)
    return ops


def restate(p, tree, ops, seqs, cmap, states, subst, freqs, rates, w, weights, pidx=None, fidx=None):
    R = len(w)
    pidx = [0] * R if pidx is None else pidx
    fidx = pidx if fidx is None else fidx
    qs = [brlen_ref.build_q(subst[m], freqs[m]) for m in pidx]
    pis = [freqs[m] for m in fidx]
    return brlen_ref.branch_derivatives(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, cmap, states),
                                        brlen_ref.pmatrices(p, ops), qs, pis, w, rates, weights)


def assert_close(what, got, want):
    """got = (d1, d2), want = (d1, d2, A1, A2): each figure printed, then |d - d_ref| <= 1e-11 A"""
    for name, d, ref, A in (("d1", got[0], want[0], want[2]), ("d2", got[1], want[1], want[3])):
        ratio = np.abs(d - ref) / A
        print("%s %s: largest |d - d_ref| / A %.3e (largest |d| %.3e)" % (what, name, ratio.max(), np.abs(ref).max()))
        assert np.all(np.isfinite(d))
        assert np.all(np.abs(d - ref) <= TOL * A)


def tip_root(tree):
    return next(rl for rl in tree.roots() if len(tree.side_tips(rl)) in (1, tree.tip_count() - 1))


def inner_root(tree):
    return next(rl for rl in tree.roots() if 2 <= len(tree.side_tips(rl)) <= tree.tip_count() - 2)


# ---- 1. exactness on the 10-taxon tree --------------------------------------------------------
@pytest.mark.parametrize("where", ["inner", "tip"])
@pytest.mark.parametrize("states,R", [(4, 1), (4, 2), (4, 4), (4, 8), (4, 3), (2, 4), (2, 1)])
def test_derivatives_equal_the_restatement(states, R, where):
    rng = np.random.default_rng(100 * states + R)
    tree = rd.Tree.from_file(TREE)
    labels = list(util.read_fasta(MSA))
    if states == 4:
        cmap, seqs = rd.MAP_NT, random_columns(rng, labels, 97, "ACGT", "RYKMSWBDHVN-")
    else:
        cmap, seqs = rd.MAP_BIN, random_columns(rng, labels, 97, "01", "-")
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, cmap, states, R, rng)
    rl = (inner_root(tree) if where == "inner" else tip_root(tree)).with_ratio(0.3)
    ops = traverse(p, tree, rl)
    if where == "tip":
        assert min(ops[-1].child1_clv_index, ops[-1].child2_clv_index) < tree.tip_count()
    got = p.branch_derivatives(ops)
    assert got[0].shape == (9, 2) and got[1].shape == (9, 2)
    assert_close("states %d R %d %s root" % (states, R, where), got,
                 restate(p, tree, ops, seqs, cmap, states, subst, freqs, rates, w, weights))


def test_two_rate_matrices_with_their_own_indices_per_category():
    rng = np.random.default_rng(12)
    tree = rd.Tree.from_file(TREE)
    seqs = random_columns(rng, list(util.read_fasta(MSA)), 97, "ACGT", "RYKMSWBDHVN-")
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng, rate_matrices=2)
    pidx, fidx = [0, 1, 1, 0], [1, 1, 0, 0]
    ops = traverse(p, tree, inner_root(tree).with_ratio(0.6), pidx)
    got = p.branch_derivatives(ops, pidx, fidx)
    want = restate(p, tree, ops, seqs, rd.MAP_NT, 4, subst, freqs, rates, w, weights, pidx, fidx)
    assert_close("two rate matrices", got, want)
    # the indices matter: the first set for every category is another answer
    other = p.branch_derivatives(ops, [0, 0, 0, 0], [0, 0, 0, 0])
    assert np.abs(other[0] - got[0]).max() > 1e-3


# ---- 2. the lane map and both stages of the sum -------------------------------------------------
@pytest.fixture(scope="module")
def thirty_three():
    rng = np.random.default_rng(33)
    newick, _ = synth.random_tree(33, rng)
    labels = ["t%04d" % i for i in range(33)]
    return newick, random_columns(rng, labels, 2100, "ACGT", "RYN-")


# (300, 3): the generic walk in two workgroups, the second with 44 live lanes; (1, 3): one live lane
@pytest.mark.parametrize("S,R", [(1, 4), (15, 4), (16, 4), (17, 4), (63, 4), (64, 4), (65, 4), (300, 4), (2100, 8),
                                 (300, 3), (1, 3)])
def test_lane_map_and_both_stages_of_the_sum(thirty_three, S, R):
    newick, all_seqs = thirty_three
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(1000 * S + R)
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    ops = traverse(p, tree, tree.root_location(17).with_ratio(0.6))
    assert rd.ancestral_workspace_slots(ops, 33) >= 1   # parents come from the workspace as well as from registers
    got = p.branch_derivatives(ops)
    assert got[0].shape == (32, 2)
    assert_close("S %d R %d" % (S, R), got, restate(p, tree, ops, seqs, rd.MAP_NT, 4, subst, freqs, rates, w, weights))


# ---- 3. depth ---------------------------------------------------------------------------------
# (R = 3: the generic walk under the rule)
@pytest.mark.parametrize("deep_first,R", [pytest.param(True, 4, id="True"), pytest.param(False, 4, id="False"),
                                          pytest.param(True, 3, id="True-R3"), pytest.param(False, 3, id="False-R3")])
def test_deep_tree_under_the_rescale_rule(deep_first, R):
    rng = np.random.default_rng(800 + deep_first)
    newick, labels = caterpillar(799, deep_first, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 800
    seqs = {l: "".join(rng.choice(list("ACGT"), size=8)) for l in labels}
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    ops = traverse(p, tree, tree.root_location("t799").with_ratio(0.5))
    assert len(ops) == 799
    # the rule fires: some column of the root CLV carries a scaler
    assert p.get_scaler(tree.root_scaler_index()).max() > 0
    got = p.branch_derivatives(ops)
    assert_close("deep child first %s R %d" % (deep_first, R), got,
                 restate(p, tree, ops, seqs, rd.MAP_NT, 4, subst, freqs, rates, w, weights))


# ---- 4. determinism, read-only ----------------------------------------------------------------
def test_two_calls_give_equal_bits_and_the_partition_is_only_read(thirty_three):
    newick, all_seqs = thirty_three
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:300] for l, s in all_seqs.items()}
    rng = np.random.default_rng(4)
    p, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng)
    ops = traverse(p, tree, tree.root_location(5).with_ratio(0.2))
    root_clv = p.get_clv(tree.root_clv_index())
    pm = p.get_pmatrix(ops[0].child1_matrix_index)
    lnl = p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
    a = p.branch_derivatives(ops)
    assert rd.branch_last_ms() > 0
    b = p.branch_derivatives(ops)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(p.get_clv(tree.root_clv_index()), root_clv)
    assert np.array_equal(p.get_pmatrix(ops[0].child1_matrix_index), pm)
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl
    # d2 may be left out
    d1 = np.zeros((len(ops), 2))
    fi = np.zeros(4, dtype=np.uint32)
    assert rd.lib.rdamd_branch_derivatives(p.handle, rd.api._op_array(ops), len(ops), rd.api._uptr(fi), rd.api._uptr(fi),
                                           rd.api._dptr(d1), None) == 1
    assert d1.tobytes() == a[0].tobytes()


# ---- 5. refusals --------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable():
    rng = np.random.default_rng(4)
    tree = rd.Tree.from_file(TREE)
    seqs = util.read_fasta(MSA)
    good, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng)
    rl = tree.root_location(3).with_ratio(0.4)
    ops = traverse(good, tree, rl)

    def valid_call():
        d1, d2 = good.branch_derivatives(ops)
        assert np.all(np.isfinite(d1)) and np.all(np.isfinite(d2))
        assert rd.branch_last_ms() > 0

    valid_call()
    w20 = synth.workload(10, 40, 20, 4, 78)
    t20 = rd.Tree.from_newick(w20["newick"])
    p20 = rd.Partition.for_tree(t20, 20, 40, 4, rd.ATTRIB_NONREV)
    util.load_tips(p20, t20, w20["seqs"], util.make_map(w20["alphabet"]))
    p20.set_subst_params(0, np.linspace(0.1, 1.9, 380))
    p20.set_frequencies(0, [0.05] * 20)
    p20.set_category_rates(rd.compute_gamma_cats(1.0, 4))
    ops20 = traverse(p20, t20, t20.root_location(2))
    with pytest.raises(rd.RdamdError, match="20-state"):
        p20.branch_derivatives(ops20)
    assert rd.lib.rdamd_errno() == 63 and rd.branch_last_ms() == 0
    valid_call()
    sparse, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng, rd.ATTRIB_SPARSE_CLVS)
    sparse_ops = traverse(sparse, tree, rl)
    with pytest.raises(rd.RdamdError, match="SPARSE_CLVS"):
        sparse.branch_derivatives(sparse_ops)
    assert rd.lib.rdamd_errno() == 63 and rd.branch_last_ms() == 0
    valid_call()
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    with pytest.raises(rd.RdamdError, match="root operation"):
        good.branch_derivatives(shuffled)
    assert rd.lib.rdamd_errno() == 64 and rd.branch_last_ms() == 0
    valid_call()
    m = rd.Model.from_file_block(rd.Tree.from_file(TREE), MSA, 0, 2)
    m.set_lnl_reducer(lambda values, n: None)
    m.initialize_partitions()
    for call in (m.branch_derivatives, m.optimize_branch_lengths):
        with pytest.raises(rd.RdamdError, match="site group"):
            call(tree.root_location(0))
        assert rd.lib.rdamd_errno() == 61
        valid_call()


# ---- 6. / 7. the model ----------------------------------------------------------------------------
def model_partition(tree, seqs, weights, cats, pp):
    """a partition with the parameters applied as model_t::set_model_params applies them (normalised
    frequencies, MEDIAN gamma rates, equal category weights)"""
    S = len(next(iter(seqs.values())))
    p = rd.Partition.for_tree(tree, 4, S, cats, rd.ATTRIB_NONREV)
    util.load_tips(p, tree, seqs, rd.MAP_NT, weights)
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], cats, rd.GAMMA_RATES_MEDIAN)) if cats > 1 else np.ones(1)
    w = np.full(cats, 1.0 / cats)
    p.set_subst_params(0, pp["subst_rates"])
    p.set_frequencies(0, f)
    p.set_category_rates(rates)
    p.set_category_weights(w)
    return p, f, rates, w


def test_model_derivatives_two_partitions(tmp_path):
    phy, tre = os.path.join(util.DATA, "101.phy"), os.path.join(util.DATA, "101.tree")
    lines = ["UNREST+G4, first = 1-60", "UNREST, second = 61-100, 900-920"]
    pf = tmp_path / "parts.txt"
    pf.write_text("\n".join(lines) + "\n")
    tree, t2 = rd.Tree.from_file(tre), rd.Tree.from_file(tre)
    m = rd.Model.from_partition_file(tree, phy, str(pf), seed=3)
    m.initialize_partitions()
    compressed, weights, _ = rd.msa_pattern_probe(phy, lines)
    names = list(util.read_phylip(phy))
    sizes = [n for n, _ in rd.msa_partition_probe(phy, lines)]
    home = tree.root_location(11).with_ratio(0.3)
    lh_before = m.compute_lh(home)
    rng = np.random.default_rng(9)
    sets = [{"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
             "gamma_alpha": [float(rng.uniform(0.3, 3.0))], "gamma_weights": []} for _ in range(2)]
    rl = tree.root_location(3).with_ratio(0.7)
    node_clv, node_parent, node_children, lengths, d1, d2, lnl = m.branch_derivatives(rl, sets)

    ops, pmi, brl = t2.generate_operations(rl)
    n = len(ops)
    want_clv, want_parent, want_children = rd.ancestral_nodes(ops)
    assert np.array_equal(node_clv, want_clv) and np.array_equal(node_parent, want_parent)
    assert np.array_equal(node_children, want_children)
    place = {int(mi): i for i, mi in enumerate(pmi)}
    sched = np.array([[brl[place[mi]] for _, mi in brlen_ref.children_of(ops[n - 1 - k])] for k in range(n)])
    assert np.array_equal(lengths, sched)

    s1, s2, A1, A2, total, at = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2)), 0.0, 0
    for pi_, (size, cats) in enumerate(zip(sizes, (4, 1))):
        seqs = {k: s[at:at + size] for k, s in zip(names, compressed)}
        wts = np.asarray(weights[at:at + size], dtype=np.uint32)
        p, f, rates, w = model_partition(t2, seqs, wts, cats, sets[pi_])
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
        total += p.compute_root_loglikelihood(t2.root_clv_index(), t2.root_scaler_index())
        g1, g2 = p.branch_derivatives(ops)
        ref = restate(p, t2, ops, seqs, rd.MAP_NT, 4, [sets[pi_]["subst_rates"]], [f], rates, w, wts)
        assert_close("partition %d" % pi_, (g1, g2), ref)
        s1, s2, A1, A2 = s1 + g1, s2 + g2, A1 + ref[2], A2 + ref[3]
        at += size
    # the model normalises the frequencies itself: not necessarily to the last bit as NumPy does
    print("model: d1 %.3e, d2 %.3e of A; lnL %.3e" % ((np.abs(d1 - s1) / A1).max(), (np.abs(d2 - s2) / A2).max(),
                                                      util.rel_err(lnl, total)))
    assert np.all(np.abs(d1 - s1) <= TOL * A1) and np.all(np.abs(d2 - s2) <= TOL * A2)
    assert util.rel_err(lnl, total) < 1e-10
    assert m.compute_lh(home) == lh_before


def scaled_newick(tree_path, rl_of, factors_rng):
    """the tree of the file with its lengths multiplied by factors from [0.3, 3]"""
    t = rd.Tree.from_file(tree_path)
    ops, pmi, brl = t.generate_operations(rl_of(t))
    n = len(ops)
    place = {int(mi): i for i, mi in enumerate(pmi)}
    lengths = np.array([[brl[place[mi]] for _, mi in brlen_ref.children_of(ops[n - 1 - k])] for k in range(n)])
    node_clv, _, _ = rd.ancestral_nodes(ops)
    return t.newick_branch_lengths(node_clv, lengths * factors_rng.uniform(0.3, 3.0, lengths.shape))


def test_model_optimises_branch_lengths_from_two_starts():
    atol, lo, hi = 1e-8, 1e-6, 100.0
    packed, weights = util.compress(util.read_fasta(MSA))
    rng = np.random.default_rng(5)
    pp = {"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
          "gamma_alpha": [0.6], "gamma_weights": []}
    own = rd.Tree.from_file(TREE)
    split = sorted(own.side_tips(own.root_location(3)))
    rest = sorted(set(own.tip_label(i) for i in range(10)) - set(split))

    def rl_of(t):
        return util.find_root(t, split, rest, 0.27)

    own_newick, scaled = open(TREE).read(), scaled_newick(TREE, rl_of, rng)
    after = []
    for start, newick in (("own", own_newick), ("scaled", scaled)):
        tree, t2 = rd.Tree.from_newick(newick), rd.Tree.from_newick(newick)   # the model's, and one to plan with
        m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
        m.initialize_partitions()
        rl = rl_of(tree)
        home = tree.root_location(0).with_ratio(0.4)
        lh_home, root_home = m.compute_lh(home), m.compute_lh_root(home)
        r = m.optimize_branch_lengths(rl, [pp], lo, hi, atol, 200)
        x = r["lengths"]
        print("%s start: lnL %.9f -> %.9f, %d iterations, %d evaluations, converged %s" % (
            start, r["lnl_before"], r["lnl_after"], r["iterations"], r["evaluations"], r["converged"]))
        assert r["converged"]
        assert x.min() >= lo and x.max() <= hi
        assert r["lnl_after"] >= r["lnl_before"]
        # nothing was applied: the model is bit for bit what it was
        assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home
        # an independent evaluation through the partition API at the returned lengths
        rl2 = rl_of(t2)
        ops, pmi, brl = t2.generate_operations(rl2)
        n = len(ops)
        p, f, rates, w = model_partition(t2, packed, weights, 4, pp)
        lens = np.array(brl, dtype=np.float64)
        place = {int(mi): i for i, mi in enumerate(pmi)}
        for k in range(n):
            for c, (_, mi) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
                lens[place[mi]] = x[k, c]
        p.update_prob_matrices(pmi, lens)
        p.update_clvs(ops)
        lnl = p.compute_root_loglikelihood(t2.root_clv_index(), t2.root_scaler_index())
        print("%s start: independent lnL %.9f, relative difference %.3e" % (start, lnl, util.rel_err(lnl, r["lnl_after"])))
        assert util.rel_err(lnl, r["lnl_after"]) < 1e-10
        d1, d2, _, _ = restate(p, t2, ops, packed, rd.MAP_NT, 4, [pp["subst_rates"]], [f], rates, w, weights)
        gain = brlen_ref.predicted_gain(x, d1, d2, lo, hi)
        print("%s start: predicted gain left %.3e" % (start, gain))
        assert gain < 2 * atol   # (the factor 2: the 1e-11 difference between device and restatement derivatives)
        after.append(r["lnl_after"])
    print("lnL after, own start %.10f, scaled start %.10f, gap %.3e" % (after[0], after[1], abs(after[0] - after[1])))
    assert abs(after[0] - after[1]) < 100 * atol


# ---- 8. the command line ------------------------------------------------------------------------
def _run(args):
    return subprocess.run([RD] + args, capture_output=True, text=True, timeout=600)


def test_rd_amd_branch_lengths(tmp_path):
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--silent", "--rate-cats", "4",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(REF):
        common += ["--lbfgsb", REF]
    prefix = str(tmp_path / "bl")
    out = _run(common + ["--prefix", prefix, "--branch-lengths"])
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [l.split("\t") for l in open(prefix + ".brlen.tsv").read().splitlines()]
    assert rows[0] == ["node", "child", "name", "input_length", "length", "d1", "d2", "at_bound"]
    assert len(rows) - 1 == 18
    assert [(r[0], r[1]) for r in rows[1:]] == [("N%d" % k, str(c)) for k in range(9) for c in range(2)]
    assert all(1e-6 <= float(r[4]) <= 100 and r[7] in ("no", "min", "max") for r in rows[1:])
    nw = open(prefix + ".brlen.tree").read()
    named = rd.Tree.from_newick(nw)
    assert named.tip_count() == 10 and all(")N%d" % k in nw for k in range(9))
    # the tree's lengths are the table's: a child's name is followed by its optimised length
    for r in rows[1:]:
        assert "%s:%s" % (r[2], r[4]) in nw, r
    line = next(l for l in out.stdout.splitlines() if l.startswith("Branch lengths at root"))
    before = float(line.split("lnL before ")[1].split(",")[0])
    after = float(line.split("after ")[1].split(",")[0])
    assert after >= before and "converged 1" in line
    # ... and the best record's lnL is the "before" value
    records = rd.Checkpoint(prefix).read_results()
    assert abs(max(r[1] for r in records) - before) <= 1e-6 * abs(before)

    refused = _run(["--msa", MSA, "--tree", TREE, "--silent", "--prefix", str(tmp_path / "no"), "--exhaustive",
                    "--site-shards", "2", "--branch-lengths"])
    assert refused.returncode != 0
    assert "--branch-lengths" in refused.stdout + refused.stderr and "--site-shards" in refused.stdout + refused.stderr
    assert not os.path.exists(str(tmp_path / "no") + ".brlen.tsv")
