"""Branch pair sums: the pre-order walk of csrc/kernels_preorder.hip with its pair-sum consumer, through
rdamd_branch_pair_sums, and the gradient assembled from them on the host.

The restatement is tests/grad_ref.py (NumPy, every vector renormalised per site).  Every term of N,
M and W is non-negative, so a sum is its own absolute-value companion: device sums are compared at
|x - x_ref| <= 1e-11 x_ref, test_gpu_brlen.py's TOL and reasoning (the rounding error of a sum of
S <= 20 000 terms is a small multiple of 2^-53 S A, three or more orders below).

The depth cases keep every vector inside the range in which both sides hold numbers exactly.  The
restatement divides a site's vector by its largest entry over all rates; the device keeps ONE
power-of-two scaling per site for all rates (the 2^256 rule of the CLVs and of the outer vectors),
under which a site's largest entry stays above 2^-512 (the product of two vectors whose largest
entries are above 2^-256, rescaled when it falls below).  A double is normal down to 2^-1022, so an
entry is held with all its bits on the device when it is at least 2^-510 of its site's largest, and
in the restatement when at least 2^-1022.  With the gamma rates of make_partition (alpha 0.7: rates
0.07 to 2.6) the slow categories of the 800-tip caterpillar fall below both limits -- the
restatement's own smallest entries are denormals, 2^-1074 -- so neither side is a reference for
them.  The depth test therefore draws its rates at alpha 20 (0.73 to 1.30) and asserts, from the
restatement alone, that no non-zero entry of any inner CLV or outer vector is below 2^-500 of its
site's largest (about 2^-280 is the smallest); the rescale rule still fires."""
import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import brlen_ref
import grad_ref
import util
from test_gpu_ancestral import caterpillar, random_columns
from test_gpu_brlen import MSA, TREE, TOL, inner_root, make_partition, thirty_three, tip_root, traverse  # noqa: F401  (thirty_three: fixture)

pytestmark = pytest.mark.gpu


def restate(p, tree, ops, seqs, cmap, states, freqs, w, weights, fidx=None):
    fidx = [0] * len(w) if fidx is None else fidx
    return grad_ref.pair_sums(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, cmap, states),
                              brlen_ref.pmatrices(p, ops), [freqs[m] for m in fidx], w, weights)


def assert_close(what, got, want):
    """got, want = (N, M, W): each figure printed, then |x - x_ref| <= 1e-11 x_ref"""
    for name, x, ref in zip(("N", "M", "W"), got, want):
        assert x.shape == ref.shape and np.all(np.isfinite(x))
        ratio = np.abs(x - ref) / np.where(ref > 0, ref, 1.0)
        print("%s %s: largest |x - x_ref| / x_ref %.3e (largest x %.3e)" % (what, name, ratio.max(), ref.max()))
        assert np.all(np.abs(x - ref) <= TOL * ref)


def assert_identities(what, p, ops, got, w, freqs_per_cat, weights):
    """I1 and I3 at 1e-11 of the total weight"""
    N, M, W = got
    total, n = float(np.sum(weights)), len(ops)
    pm = brlen_ref.pmatrices(p, ops)
    i1 = max(abs((N[k, c] * pm[m]).sum() - total) for k in range(n)
             for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])))
    i3a, i3b = abs((M * np.asarray(freqs_per_cat)).sum() - total), abs((np.asarray(w) * W).sum() - total)
    print("%s: I1 %.3e, I3 %.3e %.3e of the total weight %g" % (what, i1 / total, i3a / total, i3b / total, total))
    assert i1 <= 1e-11 * total and i3a <= 1e-11 * total and i3b <= 1e-11 * total


# ---- 1. exactness on the 10-taxon tree --------------------------------------------------------
@pytest.mark.parametrize("where", ["inner", "tip"])
@pytest.mark.parametrize("states,R", [(4, 1), (4, 2), (4, 4), (4, 8), (4, 3), (2, 4), (2, 1)])
def test_pair_sums_equal_the_restatement(states, R, where):
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
    got = p.branch_pair_sums(ops)
    assert got[0].shape == (9, 2, R, states, states) and got[1].shape == (R, states) and got[2].shape == (R,)
    what = "states %d R %d %s root" % (states, R, where)
    assert_close(what, got, restate(p, tree, ops, seqs, cmap, states, freqs, w, weights))
    assert_identities(what, p, ops, got, w, [freqs[0]] * R, weights)


def test_two_rate_matrices_with_their_own_indices_per_category():
    rng = np.random.default_rng(12)
    tree = rd.Tree.from_file(TREE)
    seqs = random_columns(rng, list(util.read_fasta(MSA)), 97, "ACGT", "RYKMSWBDHVN-")
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng, rate_matrices=2)
    pidx, fidx = [0, 1, 1, 0], [1, 1, 0, 0]
    ops = traverse(p, tree, inner_root(tree).with_ratio(0.6), pidx)
    got = p.branch_pair_sums(ops, fidx)
    assert_close("two rate matrices", got, restate(p, tree, ops, seqs, rd.MAP_NT, 4, freqs, w, weights, fidx))
    assert_identities("two rate matrices", p, ops, got, w, [freqs[m] for m in fidx], weights)
    # the indices matter: the first set for every category is another answer
    other = p.branch_pair_sums(ops, [0, 0, 0, 0])
    assert np.abs(other[0] - got[0]).max() > 1e-3
    # ... and the gradient assembled on the host from the device's sums is the restatement's from its own
    lengths = grad_ref.branch_lengths(*tree.generate_operations(inner_root(tree).with_ratio(0.6)))
    g = rd.gradient_from_pair_sums(got[0], got[1], got[2], lengths, subst, freqs, pidx, fidx, rates, w)
    ref = restate(p, tree, ops, seqs, rd.MAP_NT, 4, freqs, w, weights, fidx)
    want, comp = grad_ref.gradient(ref[0], ref[1], ref[2], lengths, subst, freqs, pidx, fidx, rates, w)
    for name, a, b, C in zip(("subst", "freqs", "rates", "weights"), g, want, comp):
        print("gradient %s: largest |g - g_ref| / C %.3e" % (name, (np.abs(a - b) / C).max()))
        assert np.all(np.abs(a - b) <= 10 * TOL * C)   # a device sum and a host contraction meet


# ---- 2. the lane map and both stages of the sum -------------------------------------------------
@pytest.mark.parametrize("S,R", [(1, 4), (15, 4), (16, 4), (17, 4), (63, 4), (64, 4), (65, 4), (300, 4), (2100, 8),
                                 (300, 3), (1, 3)])
def test_lane_map_and_both_stages_of_the_sum(thirty_three, S, R):
    newick, all_seqs = thirty_three
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(1000 * S + R)
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    ops = traverse(p, tree, tree.root_location(17).with_ratio(0.6))
    assert rd.ancestral_workspace_slots(ops, 33) >= 1
    got = p.branch_pair_sums(ops)
    assert got[0].shape == (32, 2, R, 4, 4)
    assert_close("S %d R %d" % (S, R), got, restate(p, tree, ops, seqs, rd.MAP_NT, 4, freqs, w, weights))


# ---- 3. passes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R,blocks", [(2100, 8, 66), (300, 3, 2)])
def test_passes_give_the_bytes_of_one_pass(thirty_three, S, R, blocks):
    newick, all_seqs = thirty_three
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:S] for l, s in all_seqs.items()}
    rng = np.random.default_rng(7 * S + R)
    p, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    ops = traverse(p, tree, tree.root_location(17).with_ratio(0.6))
    row_bytes = 8 * (len(ops) * 2 * R * 16 + R * 5)   # one workgroup's partial sums
    assert blocks == -(-(S * R if R == 8 else S) // 256)
    whole = p.branch_pair_sums(ops)
    assert rd.pair_sums_last_ms() > 0
    for bound in (20 * row_bytes + 8, row_bytes - 8, 1):
        cut = p.branch_pair_sums(ops, workspace_bytes=bound)
        assert rd.pair_sums_last_ms() > 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, cut)), bound


# ---- 4. I2 on the device ------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 3])
def test_contraction_with_q_p_is_the_branch_derivative(thirty_three, R):
    newick, all_seqs = thirty_three
    tree = rd.Tree.from_newick(newick)
    seqs = {l: s[:300] for l, s in all_seqs.items()}
    rng = np.random.default_rng(40 + R)
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    ops = traverse(p, tree, tree.root_location(17).with_ratio(0.6))
    N, M, W = p.branch_pair_sums(ops)
    d1, _ = p.branch_derivatives(ops)
    q = brlen_ref.build_q(subst[0], freqs[0])
    pm = brlen_ref.pmatrices(p, ops)
    n, worst = len(ops), 0.0
    for k in range(n):
        for c, (_, m) in enumerate(brlen_ref.children_of(ops[n - 1 - k])):
            got = sum(rates[r] * (N[k, c, r] * (q @ pm[m][r])).sum() for r in range(R))
            bound = sum(rates[r] * (N[k, c, r] * np.abs(q @ pm[m][r])).sum() for r in range(R))
            worst = max(worst, abs(got - d1[k, c]) / bound)
            assert abs(got - d1[k, c]) <= 1e-10 * bound
    print("R %d: I2, largest |contraction - d1| / bound %.3e" % (R, worst))
    assert_identities("R %d" % R, p, ops, (N, M, W), w, [freqs[0]] * R, weights)


# ---- 5. depth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("deep_first,R", [pytest.param(True, 4, id="True"), pytest.param(False, 4, id="False"),
                                          pytest.param(True, 3, id="True-R3"), pytest.param(False, 3, id="False-R3")])
def test_deep_tree_under_the_rescale_rule(deep_first, R):
    rng = np.random.default_rng(800 + deep_first)
    newick, labels = caterpillar(799, deep_first, rng)
    tree = rd.Tree.from_newick(newick)
    assert tree.tip_count() == 800
    seqs = {l: "".join(rng.choice(list("ACGT"), size=8)) for l in labels}
    p, subst, freqs, rates, w, weights = make_partition(tree, seqs, rd.MAP_NT, 4, R, rng)
    p.set_category_rates(rd.compute_gamma_cats(20.0, R))   # (see the module's docstring)
    ops = traverse(p, tree, tree.root_location("t799").with_ratio(0.5))
    assert len(ops) == 799
    assert p.get_scaler(tree.root_scaler_index()).max() > 0   # the rule fires
    got = p.branch_pair_sums(ops)
    smallest = []
    want = grad_ref.pair_sums(ops, tree.tip_count(), brlen_ref.tip_vectors(tree, seqs, rd.MAP_NT, 4),
                              brlen_ref.pmatrices(p, ops), [freqs[0]] * R, w, weights, smallest)
    print("deep child first %s R %d: smallest entry of a vector relative to its site's largest 2^%.1f" % (
        deep_first, R, np.log2(min(smallest))))
    assert min(smallest) >= 2.0 ** -500
    for name, x, ref in zip(("N", "M", "W"), got, want):
        out = np.abs(x - ref) > TOL * ref
        print("deep child first %s R %d %s: %d of %d entries out of bound, the largest of them %.3e in the restatement" % (
            deep_first, R, name, out.sum(), out.size, ref[out].max() if out.any() else 0.0))
    assert_close("deep child first %s R %d" % (deep_first, R), got, want)


# ---- 6. determinism, read-only ------------------------------------------------------------------
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
    a = p.branch_pair_sums(ops)
    assert rd.pair_sums_last_ms() > 0
    b = p.branch_pair_sums(ops)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert np.array_equal(p.get_clv(tree.root_clv_index()), root_clv)
    assert np.array_equal(p.get_pmatrix(ops[0].child1_matrix_index), pm)
    assert p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index()) == lnl
    # root_out and cat_out may be left out
    pair = np.zeros_like(a[0])
    fi = np.zeros(4, dtype=np.uint32)
    assert rd.lib.rdamd_branch_pair_sums(p.handle, rd.api._op_array(ops), len(ops), rd.api._uptr(fi), 0, rd.api._dptr(pair),
                                         None, None) == 1
    assert pair.tobytes() == a[0].tobytes()


# ---- 7. refusals --------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_library_usable():
    rng = np.random.default_rng(4)
    tree = rd.Tree.from_file(TREE)
    seqs = util.read_fasta(MSA)
    good, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng)
    rl = tree.root_location(3).with_ratio(0.4)
    ops = traverse(good, tree, rl)

    def valid_call():
        N, M, W = good.branch_pair_sums(ops)
        assert all(np.all(np.isfinite(v)) for v in (N, M, W)) and N.max() > 0
        assert rd.pair_sums_last_ms() > 0

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
        p20.branch_pair_sums(ops20)
    assert rd.lib.rdamd_errno() == 63 and rd.pair_sums_last_ms() == 0
    valid_call()
    sparse, _, _, _, _, _ = make_partition(tree, seqs, rd.MAP_NT, 4, 4, rng, rd.ATTRIB_SPARSE_CLVS)
    sparse_ops = traverse(sparse, tree, rl)
    with pytest.raises(rd.RdamdError, match="SPARSE_CLVS"):
        sparse.branch_pair_sums(sparse_ops)
    assert rd.lib.rdamd_errno() == 63 and rd.pair_sums_last_ms() == 0
    valid_call()
    shuffled = list(ops)
    shuffled[-1], shuffled[-2] = shuffled[-2], shuffled[-1]
    with pytest.raises(rd.RdamdError, match="root operation"):
        good.branch_pair_sums(shuffled)
    assert rd.lib.rdamd_errno() == 64 and rd.pair_sums_last_ms() == 0
    valid_call()
    fi = np.zeros(4, dtype=np.uint32)
    assert rd.lib.rdamd_branch_pair_sums(good.handle, rd.api._op_array(ops), len(ops), rd.api._uptr(fi), 0, None, None,
                                         None) != 1
    assert rd.lib.rdamd_errno() == 67 and rd.pair_sums_last_ms() == 0
    valid_call()


# ---- 8. the model -------------------------------------------------------------------------------
def test_site_group_model_is_refused():
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file_block(rd.Tree.from_file(TREE), MSA, 0, 2)
    m.set_lnl_reducer(lambda values, n: None)
    m.initialize_partitions()
    pp = {"subst_rates": [0.5] * 12, "freqs": [0.25] * 4, "gamma_alpha": [1.0], "gamma_weights": []}
    with pytest.raises(rd.RdamdError, match="site group"):
        m.gradient(tree.root_location(0), [pp])
    assert rd.lib.rdamd_errno() == 61


def check_model_gradient(m, tree, rl, sets, home):
    """Model.gradient against central differences (step 1e-5, per pattern, fsum) of Model.site_lnls at
    perturbed checkpoint parameters, at 1e-4 max(1, |g|); the model afterwards is what it was"""
    import math
    step = 1e-5
    lh_home, root_home = m.compute_lh(home), m.compute_lh_root(home)
    before = [m.partition_frequencies(p) for p in range(m.partition_count())]
    weights, _ = m.site_patterns()
    weights = weights.astype(np.float64)
    grad, lnl = m.gradient(rl, sets)
    base = m.site_lnls([rl], [sets])[0]
    assert util.rel_err(lnl, math.fsum(weights * base)) < 1e-10
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home
    assert all(np.array_equal(m.partition_frequencies(p), before[p]) for p in range(m.partition_count()))
    for p, pp in enumerate(sets):
        for key in ("subst_rates", "freqs", "gamma_alpha", "gamma_weights"):
            assert len(grad[p][key]) == len(pp[key])
            worst = 0.0
            for i in range(len(pp[key])):
                f = []
                for sign in (1.0, -1.0):
                    moved = [{k: list(v) for k, v in q.items()} for q in sets]
                    moved[p][key][i] += sign * step
                    f.append(m.site_lnls([rl], [moved])[0])
                cd = math.fsum(weights * (f[0] - f[1])) / (2 * step)
                g = grad[p][key][i]
                worst = max(worst, abs(g - cd) / max(1.0, abs(g)))
            if len(pp[key]):
                print("partition %d %s: largest scaled error %.3e (largest |g| %.3e)" % (p, key, worst,
                                                                                          np.abs(grad[p][key]).max()))
            assert worst <= 1e-4
    assert m.compute_lh_root(home) == root_home and m.compute_lh(home) == lh_home


def test_model_gradient_one_partition():
    packed, weights = util.compress(util.read_fasta(MSA))
    tree = rd.Tree.from_file(TREE)
    m = rd.Model(tree, packed, rate_cats=4, weights=weights, seed=3)
    m.initialize_partitions()
    rng = np.random.default_rng(5)
    pp = {"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
          "gamma_alpha": [0.6], "gamma_weights": []}
    check_model_gradient(m, tree, tree.root_location(3).with_ratio(0.27), [pp], tree.root_location(0).with_ratio(0.4))


def test_model_gradient_two_partitions(tmp_path):
    import os
    phy, tre = os.path.join(util.DATA, "101.phy"), os.path.join(util.DATA, "101.tree")
    pf = tmp_path / "parts.txt"
    pf.write_text("UNREST+G4, first = 1-60\nUNREST, second = 61-100, 900-920\n")
    tree = rd.Tree.from_file(tre)
    m = rd.Model.from_partition_file(tree, phy, str(pf), seed=3)
    m.initialize_partitions()
    rng = np.random.default_rng(9)
    sets = [{"subst_rates": rng.uniform(0.05, 1.0, 12).tolist(), "freqs": rng.uniform(0.2, 1.0, 4).tolist(),
             "gamma_alpha": [float(rng.uniform(0.3, 3.0))], "gamma_weights": []} for _ in range(2)]
    check_model_gradient(m, tree, tree.root_location(3).with_ratio(0.7), sets, tree.root_location(11).with_ratio(0.3))


# ---- 9. the command line ------------------------------------------------------------------------
def _run(args):
    import os
    import subprocess
    return subprocess.run([os.path.join(util.ROOT, "root_digger_amd", "bin", "rd_amd")] + args, capture_output=True, text=True,
                          timeout=600)


def test_rd_amd_gradient(tmp_path):
    import os
    ref = os.path.join(util.ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--silent", "--rate-cats", "4",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(ref):
        common += ["--lbfgsb", ref]
    prefix, plain = str(tmp_path / "grad"), str(tmp_path / "plain")
    out = _run(common + ["--prefix", prefix, "--gradient"])
    assert out.returncode == 0, out.stdout + out.stderr
    records = rd.Checkpoint(prefix).read_results()
    best = max(range(len(records)), key=lambda i: (records[i][1], -i))   # the first maximum
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=4, seed=5)
    m.initialize_partitions()
    rl = tree.root_location(records[best][0]).with_ratio(records[best][2])
    grad, lnl = m.gradient(rl, records[best][3])
    rows = [l.split("\t") for l in open(prefix + ".gradient.tsv").read().splitlines()]
    assert rows[0] == ["partition", "name", "value", "gradient", "forward_difference", "at_bound"]
    want_names, want_values, want_grad = [], [], []
    for key, name in (("subst_rates", "subst_rate"), ("freqs", "freq"), ("gamma_alpha", "alpha"), ("gamma_weights", "weight")):
        for i, v in enumerate(records[best][3][0][key]):
            want_names.append("%s_%d" % (name, i))
            want_values.append(v)
            want_grad.append(grad[0][key][i])
    assert [r[1] for r in rows[1:]] == want_names and len(want_names) == 17
    assert all(r[0] == "0" and r[5] in ("no", "min", "max") for r in rows[1:])
    assert [float(r[2]) for r in rows[1:]] == want_values
    assert [float(r[3]) for r in rows[1:]] == want_grad   # (%.17g: the bits)
    # (the forward difference is off by h times the curvature, which is not small beside a gradient near an optimum)
    assert all(np.isfinite(float(r[4])) for r in rows[1:])
    line = next(l for l in out.stdout.splitlines() if l.startswith("Gradient at root"))
    assert "largest projected component" in line and abs(float(line.split("lnL ")[1].split(",")[0]) - lnl) <= 1e-6 * abs(lnl)

    # the same run without the option: every shared output byte for byte, nothing new
    out2 = _run(common + ["--prefix", plain])
    assert out2.returncode == 0, out2.stdout + out2.stderr
    made = sorted(f[len("grad"):] for f in os.listdir(tmp_path) if f.startswith("grad"))
    shared = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain"))
    assert sorted(set(made) - set(shared)) == [".gradient.tsv"]
    for ext in shared:
        if ext != ".ckp":   # (the checkpoint's header holds the prefix)
            assert open(plain + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    assert [l for l in out.stdout.splitlines() if not l.startswith("Gradient at root")] == out2.stdout.splitlines()

    # refused where --branch-lengths is
    refused = _run(["--msa", MSA, "--tree", TREE, "--silent", "--prefix", str(tmp_path / "no"), "--exhaustive",
                    "--site-shards", "2", "--gradient"])
    assert refused.returncode != 0
    assert "--gradient" in refused.stdout + refused.stderr and "--site-shards" in refused.stdout + refused.stderr
    assert not os.path.exists(str(tmp_path / "no") + ".gradient.tsv")
