"""Partitions with SEVERAL rate matrices, every rate category naming its own: params_indices[r] for
the P-matrices, freqs_indices[r] -- another vector -- for the root frequencies, on every entry point
of the C ABI that takes such a vector.  The reference is the CPU oracle, itself pinned for this case
by tests/test_oracle_rate_matrices.py; tolerances are those of tests/test_gpu_parity.py (P 1e-13
absolute, CLVs 1e-12 relative, scalers bit-exact, lnL 1e-11 relative).

Every comparison starts with a guard against a vacuous pass: by the oracle, the lnL with the mixed
indices differs by more than 1e-6 relative from the lnL with all-zero indices on the same data -- the
value a kernel that ignored the index would return -- and from the lnL with only one of the two
vectors zeroed.

The M parameter sets are independent draws of the generators synth.workload uses for its one set
(util.mixture_params), the category rates the workload's own (gamma shape 1): exp(Qt) by scaling and
squaring loses about 2^s ulp over its s squarings, in the oracle as in the kernels, so how far
||Q|| x rate x 25 may go at 1e-13 is test_prob_matrices' question (test_gpu_parity.py), not this file's."""
import functools
import itertools

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
from oracle_lib import OraclePartition, ORC_MAP_NT
from test_gpu_parity import compare_state, LNL_TOL
from test_gpu_ancestral import FIVE, cat_and_mean, children_of, device_pmatrices, random_columns, tip_vectors
import util

pytestmark = pytest.mark.gpu

P_TOL = 1e-13
SHAPES = [(4, 1, 2), (4, 4, 3), (4, 8, 3), (4, 3, 3), (2, 2, 2), (5, 3, 2), (20, 4, 4), (20, 8, 2)]   # (K, R, M)


# ---- index vectors --------------------------------------------------------------------------
def index_patterns(R, M):
    """{name: vector}: all distinct (where R allows it), with repeats (where R > 2), constant at M - 1"""
    out = {}
    if R <= M:
        out["distinct"] = [(r + M - 1) % M for r in range(R)]
    if R > 2:
        if M > 2:   # [2, 0, 2, 1] for four categories over three matrices
            rep = [2, 0, 2, 1, 1, 2, 0, 0, 1, 0, 2, 2, 0, 1, 1, 0]
            out["repeats"] = [M - 1 if x == 2 else x for x in rep[:R]]
        else:
            out["repeats"] = [1, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1][:R]
    out["constant"] = [M - 1] * R
    for v in out.values():
        assert len(v) == R and max(v) < M and any(v)
    return out


def shifted(vector, M):
    """another vector: different from `vector` in every category"""
    return [(x + 1) % M for x in vector]


# ---- data -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(K):
    """(newick, sequences, GPU character map, oracle character map): 9 to 12 tips, 130 columns (65 of
    20 states) with gaps and ambiguity codes in about a fifth of the cells"""
    n, S = {4: (12, 130), 2: (10, 130), 5: (9, 130), 20: (9, 65)}[K]
    w = synth.workload(n, S, K, 4, 4100 + K)
    rng = np.random.default_rng(4200 + K)
    if K == 4:
        return w["newick"], util.odd_cells(rng, w["seqs"], "RYKMSWBDHVN-"), rd.MAP_NT, ORC_MAP_NT
    everything = (1 << K) - 1
    cmap = util.make_map(w["alphabet"], {"-": everything, "x": everything, "b": 0b11 if K == 2 else 0b110})
    return w["newick"], util.odd_cells(rng, w["seqs"], "-xb"), cmap, cmap


class Case:
    """a GPU partition and an oracle partition of the same sizes, data and M parameter sets"""

    def __init__(self, K, R, M, S, seed, newick=None, seqs=None, cmaps=None, equal_sets=False):
        base_newick, base_seqs, cg, co = base(K) if newick is None else (newick, seqs) + cmaps
        self.K, self.R, self.M, self.S = K, R, M, S
        self.tree = rd.Tree.from_newick(base_newick)
        self.seqs = {k: v[:S] for k, v in base_seqs.items()}
        rng = self.rng = np.random.default_rng(seed)
        t, b = self.tree.tip_count(), self.tree.branch_count()
        self.g = rd.Partition(t, b, K, S, M, b, R, b)
        self.o = OraclePartition(t, b, K, S, M, b, R, b)
        self.pattern_weights = rng.integers(1, 4, size=S).astype(np.uint32)
        util.load_tips(self.g, self.tree, self.seqs, cg, self.pattern_weights)
        util.load_tips(self.o, self.tree, self.seqs, co, self.pattern_weights)
        self.subst, self.freqs = util.mixture_params(rng, K, M)
        if equal_sets:
            self.subst, self.freqs = [self.subst[0]] * M, [self.freqs[0]] * M
        self.rates = np.array(rd.compute_gamma_cats(1.0, R)) if R > 1 else np.ones(1)   # (synth.workload's)
        self.cat_weights = rng.dirichlet(np.ones(R) * 3)
        util.set_mixture((self.g, self.o), self.subst, self.freqs, self.rates, self.cat_weights)

    @property
    def root(self):
        """(CLV, scaler) of the root operation, once the tree is rooted"""
        return self.tree.root_clv_index(), self.tree.root_scaler_index()

    def rooting(self, tip_child=None):
        """a root location (the tree is left rooted there); tip_child: whether the root operation reads a tip"""
        for rl in self.tree.roots():
            ops, _, _ = self.tree.generate_operations(rl)
            last = ops[len(ops) - 1]
            has_tip = min(last.child1_clv_index, last.child2_clv_index) < self.tree.tip_count()
            if tip_child is None or has_tip == tip_child:
                return rl.with_ratio(0.3)
        raise AssertionError("no such root")

    def lh(self, part, rl, pidx, fidx):
        """the full traversal: P by pidx, the root frequencies by fidx"""
        ops, pmi, brl = self.tree.generate_operations(rl)
        part.update_prob_matrices(pmi, brl, pidx)
        part.update_clvs(ops)
        return part.compute_root_loglikelihood(*self.root, fidx)

    def guard(self, rl, pidx, fidx):
        """the oracle's lnL with (pidx, fidx), which no kernel that ignored an index could return; the
        oracle is left in that state"""
        zero = [0] * self.R
        for other in {(tuple(zero), tuple(zero)), (tuple(pidx), tuple(zero)), (tuple(zero), tuple(fidx))}:
            if other != (tuple(pidx), tuple(fidx)):
                blind = self.lh(self.o, rl, list(other[0]), list(other[1]))
                mixed = self.lh(self.o, rl, pidx, fidx)
                assert util.rel_err(mixed, blind) > 1e-6, (other, mixed, blind)
        assert any(pidx) or any(fidx)
        return self.lh(self.o, rl, pidx, fidx)

    def close(self):
        self.g.destroy()
        self.o.destroy()


def close_sites(a, b, tol=LNL_TOL):
    return np.all(np.abs(a - b) <= tol * np.abs(b))


# ---- P-matrices and tip tables ----------------------------------------------------------------
@pytest.mark.parametrize("K,R,M,pattern", [(K, R, M, name) for K, R, M in SHAPES for name in index_patterns(R, M)])
def test_prob_matrices_and_tip_tables(K, R, M, pattern):
    c = Case(K, R, M, 33, 10 * K + R)
    pidx = index_patterns(R, M)[pattern]
    rl = c.rooting(tip_child=True)
    want = c.guard(rl, pidx, pidx)
    # (the matrices depend on the index as well: by the oracle, P of a branch of length 0.3 by `pidx` is not P by zeros)
    c.o.update_prob_matrices([0], [0.3], pidx)
    by_index = c.o.get_pmatrix(0)
    c.o.update_prob_matrices([0], [0.3], [0] * R)
    assert np.max(np.abs(by_index - c.o.get_pmatrix(0))) > 1e-3
    # every matrix of the partition: the edge lengths of test_prob_matrices, then random ones
    nm = c.g.prob_matrices
    idx = c.rng.permutation(nm).astype(np.uint32)
    bl = np.concatenate([[0.0, 1e-8, 1e-6, 25.0], c.rng.exponential(0.3, nm - 4)])
    for p in (c.g, c.o):
        p.update_prob_matrices(idx, bl, pidx)
    for m in range(nm):
        a, b = c.g.get_pmatrix(m), c.o.get_pmatrix(m)
        assert a.shape == (R, K, K)
        assert np.max(np.abs(a - b)) < P_TOL, m
        assert np.all(a >= 0.0)
        assert np.allclose(a.sum(axis=2), 1.0, atol=1e-12)
    # one full traversal whose operations read tips: the tip tables of every category
    c.g.params_indices = c.o.params_indices = np.array(pidx, dtype=np.uint32)
    ops, _, _ = c.tree.generate_operations(rl)
    got = util.compute_lh(c.g, c.tree, rl)
    assert util.compute_lh(c.o, c.tree, rl) == want
    assert any(min(op.child1_clv_index, op.child2_clv_index) < c.tree.tip_count() for op in ops)
    compare_state(c.g, c.o, ops, c.tree)
    assert util.rel_err(got, want) < LNL_TOL, (got, want)
    assert util.rel_err(util.compute_lh_root(c.g, c.tree, rl), want) < LNL_TOL
    c.close()


# ---- root lnL, single and batched -------------------------------------------------------------
@pytest.mark.parametrize("K,R,M,S", [(K, R, M, S) for K, R, M in SHAPES + [(4, 16, 2)] for S in (1, 65, 130)
                                     if K * S <= 20 * 65])
def test_root_lnl_single_and_batched(K, R, M, S):
    """the group kernel for 1, 2, 4, 8 and 16 categories, the site kernel for 3 categories and 5 states, and
    the 20-state operand layout: the frequency set of category r is freqs_indices[r], whatever built P"""
    c = Case(K, R, M, S, 100 * K + R + S)
    rl = c.rooting()
    ops, _, _ = c.tree.generate_operations(rl)
    inner = [ops[i] for i in range(len(ops) - 5, len(ops))]
    clvs = [op.parent_clv_index for op in inner]
    scalers = [op.parent_scaler_index for op in inner]
    assert len(set(clvs)) == 5 and clvs[-1] == c.root[0]
    for name, fidx in index_patterns(R, M).items():
        pidx = shifted(fidx, M)
        want = c.guard(rl, pidx, fidx)
        c.lh(c.g, rl, pidx, fidx)
        got, got_sites = c.g.compute_root_loglikelihood(*c.root, fidx, persite=True)
        same, want_sites = c.o.compute_root_loglikelihood(*c.root, fidx, persite=True)
        assert same == want
        print("%s: total %.2e, per site %.2e" % (name, util.rel_err(got, want),
                                                 np.max(np.abs(got_sites - want_sites) / np.abs(want_sites))))
        assert util.rel_err(got, want) < LNL_TOL, (name, got, want)
        assert got_sites.shape == (S,) and close_sites(got_sites, want_sites), name
        assert got == c.g.compute_root_loglikelihood(*c.root, fidx)
        # five CLVs of the traversal in one launch: every value the single call's, bit for bit
        many = c.g.compute_root_loglikelihoods(clvs, scalers, fidx)
        for i, (clv, sc) in enumerate(zip(clvs, scalers)):
            one = c.g.compute_root_loglikelihood(clv, sc, fidx)
            assert many[i] == one, (name, i)
            assert util.rel_err(one, c.o.compute_root_loglikelihood(clv, sc, fidx)) < LNL_TOL, (name, i)
        assert many[4] == got
    c.close()


# ---- fused root step --------------------------------------------------------------------------
def unfused_root_step(part, op, pmi, l1, l2, pidx):
    part.update_prob_matrices(pmi, [l1, l2], pidx)
    part.update_clvs([op])
    return part.compute_root_loglikelihood(op.parent_clv_index, op.parent_scaler_index, pidx)


def root_positions(rl):
    alphas = [0.3, 0.0, 0.3 + 1e-8, 1.0]
    return [rl.saved_brlen * a for a in alphas], [rl.saved_brlen * (1 - a) for a in alphas]


@pytest.mark.parametrize("tip_child", [False, True])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_fused_root_step(R, tip_child):
    """rdamd_root_loglikelihood_fused takes ONE vector: category r reads matrix and frequency set
    params_indices[r].  Against the oracle; bit for bit against the three calls it replaces; and the
    state it leaves is theirs for the last position (csrc/kernels_root.hip, `the state contract`)."""
    M = 3
    c = Case(4, R, M, 130, 300 + R)
    pidx = index_patterns(R, M)["repeats" if R > 2 else "distinct" if R == 2 else "constant"]
    rl = c.rooting(tip_child)
    c.guard(rl, pidx, pidx)
    c.lh(c.g, rl, pidx, pidx)
    op, pmi, _ = c.tree.generate_derivative_operations(rl)
    assert (min(op.child1_clv_index, op.child2_clv_index) < c.tree.tip_count()) == tip_child
    l1, l2 = root_positions(rl)
    got = c.g.root_loglikelihood_fused(op, l1, l2, pidx)
    want = c.o.root_loglikelihood_fused(op, l1, l2, pidx)
    blind = c.o.root_loglikelihood_fused(op, l1, l2, [0] * R)
    c.o.root_loglikelihood_fused(op, l1, l2, pidx)
    for a in range(4):
        assert util.rel_err(want[a], blind[a]) > 1e-6
        assert util.rel_err(got[a], want[a]) < LNL_TOL, (a, got[a], want[a])
    for a in range(4):
        assert unfused_root_step(c.g, op, pmi, l1[a], l2[a], pidx) == got[a], a
    # the state after the call is the LAST position's: both matrices and the scaler have the bits the three
    # calls leave, the root CLV is the one the returned value was reduced from (its entries may differ from
    # the traversal kernel's in the last bit: the two kernels contract their products differently)
    assert np.array_equal(c.g.root_loglikelihood_fused(op, l1, l2, pidx), got)
    assert c.g.compute_root_loglikelihood(op.parent_clv_index, op.parent_scaler_index, pidx) == got[3]
    left = [c.g.get_pmatrix(int(m)) for m in pmi] + [c.g.get_scaler(op.parent_scaler_index), c.g.get_clv(op.parent_clv_index)]
    compare_state(c.g, c.o, [op], c.tree)
    unfused_root_step(c.g, op, pmi, l1[3], l2[3], pidx)
    unfused = [c.g.get_pmatrix(int(m)) for m in pmi] + [c.g.get_scaler(op.parent_scaler_index), c.g.get_clv(op.parent_clv_index)]
    for x, y in zip(left[:3], unfused[:3]):
        assert np.array_equal(x, y)
    assert np.allclose(left[3], unfused[3], rtol=1e-12, atol=0.0)
    for m, x in zip(pmi, left[:2]):
        assert np.max(np.abs(x - c.o.get_pmatrix(int(m)))) < P_TOL
    # ... and a traversal that follows reads those matrices (a tip child: through its tables)
    c.g.root_loglikelihood_fused(op, l1, l2, pidx)
    c.g.update_clvs([op])
    compare_state(c.g, c.o, [op], c.tree)
    assert c.g.compute_root_loglikelihood(op.parent_clv_index, op.parent_scaler_index, pidx) == got[3]
    c.close()


def test_fused_root_step_three_categories_fall_back():
    c = Case(4, 3, 3, 65, 303)
    pidx = index_patterns(3, 3)["repeats"]
    rl = c.rooting(True)
    c.guard(rl, pidx, pidx)
    c.lh(c.g, rl, pidx, pidx)
    op, pmi, _ = c.tree.generate_derivative_operations(rl)
    l1, l2 = root_positions(rl)
    got = c.g.root_loglikelihood_fused(op, l1, l2, pidx)
    want = c.o.root_loglikelihood_fused(op, l1, l2, pidx)
    for a in range(4):
        assert util.rel_err(got[a], want[a]) < LNL_TOL, (a, got[a], want[a])
        assert unfused_root_step(c.g, op, pmi, l1[a], l2[a], pidx) == got[a], a
    c.close()


def test_fused_multi_every_partition_its_own_indices():
    """one launch over three partitions of different size, each with its own vector: every row is what
    rdamd_root_loglikelihood_fused gives on that partition alone, bit for bit"""
    rows = []
    for S, pidx in ((40, [2, 0, 2, 1]), (130, [0, 1, 1, 2]), (65, [1, 2, 0, 0])):
        c = Case(4, 4, 3, S, 400 + S)
        rl = c.rooting(S == 65)
        c.guard(rl, pidx, pidx)
        c.lh(c.g, rl, pidx, pidx)
        op, _, _ = c.tree.generate_derivative_operations(rl)
        c.g.params_indices = np.array(pidx, dtype=np.uint32)
        c.g.profile_enable(True)
        rows.append((c, op, pidx) + root_positions(rl))
    for c, *_ in rows:
        c.g.profile_read()
    got = rd.root_loglikelihood_fused_multi([r[0].g for r in rows], [r[1] for r in rows], [r[3] for r in rows],
                                            [r[4] for r in rows])
    assert [r[0].g.profile_read()["root"][1] for r in rows] == [1, 0, 0]      # one launch: no fallback
    for (c, op, pidx, l1, l2), values in zip(rows, got):
        left = c.g.get_clv(op.parent_clv_index)
        assert np.array_equal(values, c.g.root_loglikelihood_fused(op, l1, l2, pidx)), c.S
        assert np.array_equal(left, c.g.get_clv(op.parent_clv_index))
        want = c.o.root_loglikelihood_fused(op, l1, l2, pidx)
        for a in range(4):
            assert util.rel_err(values[a], want[a]) < LNL_TOL, (c.S, a)
        c.close()


# ---- ancestral posteriors and site rates --------------------------------------------------------
def enumeration_per_category(ops, tips, tipvec, pmat, pis, w):
    """test_gpu_ancestral.enumeration with a frequency vector per category, pis[r]: the joint probability
    summed over ALL assignments of the inner nodes, category by category -> (post[n][S][K], w_r L_r[S][R])"""
    n, K, R = len(ops), len(pis[0]), len(w)
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
        pr = np.tile(np.array([pis[r][x[0]] for r in range(R)]), (S, 1))
        for k in range(n):
            for c, m in children_of(ops[n - 1 - k]):
                pr = pr * (tipfac[c][:, :, x[k]] if c < tips else pmat[m][None, :, x[k], x[index_of[c]]])
        like += pr
        for k in range(n):
            marg[k, :, :, x[k]] += pr
    post = (np.asarray(w)[None, None, :, None] * marg).sum(axis=2)
    return post / post.sum(axis=2, keepdims=True), np.asarray(w)[None, :] * like


@pytest.mark.parametrize("K,R,M,pidx,fidx", [(4, 4, 3, [2, 0, 2, 1], [1, 1, 0, 2]), (2, 2, 2, [1, 0], [0, 1])])
def test_ancestral_posteriors_and_site_rates(K, R, M, pidx, fidx):
    rng = np.random.default_rng(500 + K)
    if K == 4:
        cmap, ocmap, seqs = rd.MAP_NT, ORC_MAP_NT, random_columns(rng, "abcde", 30, "ACGT", "RYKMSWBDHVN-")
    else:
        cmap = ocmap = rd.MAP_BIN
        seqs = random_columns(rng, "abcde", 30, "01", "-")
    c = Case(K, R, M, 30, 510 + K, FIVE, seqs, (cmap, ocmap))
    rl = c.tree.root_location(5).with_ratio(0.3)
    c.guard(rl, pidx, fidx)
    c.lh(c.g, rl, pidx, fidx)
    ops, _, _ = c.tree.generate_operations(rl)
    assert len(ops) == 4
    post = c.g.marginal_ancestral(ops, fidx)
    cat, mean = c.g.site_rate_posteriors(*c.root, fidx)
    pis = [c.freqs[fidx[r]] for r in range(R)]
    want, site_rate = enumeration_per_category(ops, 5, tip_vectors(c.tree, c.seqs, cmap, K), device_pmatrices(c.g, ops),
                                               pis, c.cat_weights)
    want_cat, want_mean = cat_and_mean(site_rate, c.rates)
    # (with the frequencies of set 0 in every category the answer is another one)
    blind, blind_rate = enumeration_per_category(ops, 5, tip_vectors(c.tree, c.seqs, cmap, K), device_pmatrices(c.g, ops),
                                                 [c.freqs[0]] * R, c.cat_weights)
    assert np.abs(blind - want).max() > 1e-4 and np.abs(cat_and_mean(blind_rate, c.rates)[0] - want_cat).max() > 1e-4
    print("K %d: post %.3e, cat %.3e, mean %.3e" % (K, np.abs(post - want).max(), np.abs(cat - want_cat).max(),
                                                    np.abs(mean - want_mean).max()))
    assert post.shape == (4, 30, K)
    assert np.abs(post - want).max() < 1e-12
    assert np.abs(cat - want_cat).max() < 1e-12
    assert np.abs(mean - want_mean).max() < 1e-12
    c.close()


# ---- exact properties ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,R,M", [(4, 4, 3), (4, 8, 3), (2, 2, 2), (5, 3, 2), (20, 4, 4)])
def test_equal_parameter_sets_make_the_indices_irrelevant(K, R, M):
    """all M sets equal: every index vector gives the bits of the all-zero vector -- P-matrices, CLVs,
    scalers, lnL, on the traversal, the root-only and the fused root paths"""
    c = Case(K, R, M, 65, 600 + K + R, equal_sets=True)
    rl = c.rooting(True)
    ops, pmi, brl = c.tree.generate_operations(rl)
    op, rpmi, _ = c.tree.generate_derivative_operations(rl)
    l1, l2 = root_positions(rl)

    def everything(pidx, fidx):
        out = [np.array([c.lh(c.g, rl, pidx, fidx)])]
        out += [c.g.get_pmatrix(int(m)) for m in pmi]
        for o in ops:
            out.append(c.g.get_clv(o.parent_clv_index))
            if o.parent_scaler_index >= 0:
                out.append(c.g.get_scaler(o.parent_scaler_index))
        out.append(c.g.root_loglikelihood_fused(op, l1, l2, pidx))
        out += [c.g.get_pmatrix(int(m)) for m in rpmi] + [c.g.get_clv(op.parent_clv_index)]
        out.append(np.array([unfused_root_step(c.g, op, rpmi, l1[1], l2[1], pidx)]))
        return out

    zero = [0] * R
    base_line = everything(zero, zero)
    assert util.rel_err(base_line[0][0], c.lh(c.o, rl, zero, zero)) < LNL_TOL
    for name, pidx in index_patterns(R, M).items():
        for x, y in zip(base_line, everything(pidx, shifted(pidx, M))):
            assert np.array_equal(x, y), name
    c.close()


@pytest.mark.parametrize("K", [4, 2, 20])
def test_one_parameter_set_changes_only_the_categories_that_name_it(K):
    """rdamd_set_subst_params(1, ...) / rdamd_set_frequencies(1, ...): the per-matrix dirty flags of the
    host mirror (and the 2-state embedding's own per-matrix copies)"""
    R, M = 4, 2
    c = Case(K, R, M, 33, 700 + K)
    pidx = [0, 1, 0, 1]
    zero = [0] * R
    rl = c.rooting(True)
    ops, pmi, brl = c.tree.generate_operations(rl)
    c.guard(rl, pidx, pidx)
    c.lh(c.g, rl, pidx, pidx)
    before = [c.g.get_pmatrix(int(m)) for m in pmi]
    lnl_zero, lnl_mixed = (c.g.compute_root_loglikelihood(*c.root, f) for f in (zero, pidx))
    # frequencies of set 1 alone: the root lnL by set 0 keeps its bits, the mixed one follows the oracle
    fresh_f = c.rng.dirichlet(np.ones(K) * 5)
    for p in (c.g, c.o):
        p.set_frequencies(1, fresh_f)
    assert c.g.compute_root_loglikelihood(*c.root, zero) == lnl_zero
    now = c.g.compute_root_loglikelihood(*c.root, pidx)
    assert now != lnl_mixed and util.rel_err(now, c.o.compute_root_loglikelihood(*c.root, pidx)) < LNL_TOL
    assert np.allclose(np.ctypeslib.as_array(rd.lib.rdamd_partition_frequencies(c.g.handle, 1), shape=(K,)), fresh_f, rtol=0, atol=0)
    assert np.allclose(np.ctypeslib.as_array(rd.lib.rdamd_partition_frequencies(c.g.handle, 0), shape=(K,)), c.freqs[0], rtol=0, atol=0)
    for p in (c.g, c.o):
        p.set_frequencies(1, c.freqs[1])
    assert c.g.compute_root_loglikelihood(*c.root, pidx) == lnl_mixed
    # exchange rates of set 1 alone: categories 0 and 2 keep their P bits, 1 and 3 move with the oracle
    fresh_s = c.rng.uniform(0.05, 2.0, K * K - K)
    for p in (c.g, c.o):
        p.set_subst_params(1, fresh_s)
        p.update_prob_matrices(pmi, brl, pidx)
    assert list(c.g.subst_params(1)) == list(fresh_s) and list(c.g.subst_params(0)) == list(c.subst[0])
    for m, old in zip(pmi, before):
        new = c.g.get_pmatrix(int(m))
        assert np.array_equal(new[[0, 2]], old[[0, 2]])
        assert not np.array_equal(new[1], old[1]) and not np.array_equal(new[3], old[3])
        assert np.max(np.abs(new - c.o.get_pmatrix(int(m)))) < P_TOL
    c.close()


def test_evaluate_batch_on_a_partition_with_three_rate_matrices():
    """the fused evaluator carries ONE parameter set per job: on a partition with three matrices it
    returns the oracle's values for the jobs' own parameters and leaves the partition's mixed state alone
    (as test_fused_matches_unfused_and_leaves_partition_state_alone, test_gpu_parity.py)"""
    c = Case(4, 4, 3, 130, 800)
    pidx = [2, 0, 2, 1]
    c.g.params_indices = c.o.params_indices = np.array(pidx, dtype=np.uint32)
    rl0 = c.rooting(False)
    c.guard(rl0, pidx, pidx)
    base_lnl = util.compute_lh(c.g, c.tree, rl0)
    assert util.rel_err(base_lnl, util.compute_lh(c.o, c.tree, rl0)) < LNL_TOL
    co = base(4)[3]
    plain = OraclePartition.for_tree(c.tree, 4, 130, 4)
    util.load_tips(plain, c.tree, c.seqs, co, c.pattern_weights)
    plain.set_category_rates(c.rates)
    plain.set_category_weights(c.cat_weights)
    rls = [c.tree.root_location(i).with_ratio(a) for i, a in ((2, 0.7), (9, 0.1), (17, 0.5))]
    scheds = [c.g.schedule(*c.tree.generate_operations(rl)) for rl in rls]
    subst = c.rng.uniform(0.05, 2.0, (3, 12))
    freqs = c.rng.dirichlet(np.ones(4) * 5, 3)
    got = c.g.evaluate_batch(scheds, subst, freqs)
    for j, rl in enumerate(rls):
        plain.set_subst_params(0, subst[j])
        plain.set_frequencies(0, freqs[j])
        assert util.rel_err(got[j], util.compute_lh(plain, c.tree, rl)) < LNL_TOL, j
    c.tree.root_by(rl0)
    assert util.compute_lh_root(c.g, c.tree, rl0) == base_lnl
    plain.destroy()
    c.close()


# ---- refusals -------------------------------------------------------------------------------
def test_an_index_past_the_last_rate_matrix_is_refused_by_every_call():
    R, M = 4, 3
    cases = [Case(4, R, M, S, 900 + S) for S in (33, 40, 65)]
    good, bad = [2, 0, 2, 1], [2, 0, 2, M]
    for c in cases:
        rl = c.rooting(True)
        c.want = c.guard(rl, good, good)
        c.rl = rl
        c.lh(c.g, rl, good, good)
        c.ops = c.tree.generate_operations(rl)
        c.op = c.tree.generate_derivative_operations(rl)[0]
        c.g.params_indices = np.array(good, dtype=np.uint32)
    c = cases[0]
    ops, pmi, brl = c.ops
    l1, l2 = root_positions(c.rl)

    def multi():
        for x in cases[1:]:
            x.g.params_indices = np.array(good, dtype=np.uint32)
        c.g.params_indices = np.array(bad, dtype=np.uint32)
        try:
            rd.root_loglikelihood_fused_multi([x.g for x in cases], [x.op for x in cases],
                                              [root_positions(x.rl)[0] for x in cases], [root_positions(x.rl)[1] for x in cases])
        finally:
            c.g.params_indices = np.array(good, dtype=np.uint32)

    calls = {
        "rdamd_update_prob_matrices": lambda: c.g.update_prob_matrices(pmi, brl, bad),
        "rdamd_compute_root_loglikelihood": lambda: c.g.compute_root_loglikelihood(*c.root, bad),
        "rdamd_compute_root_loglikelihoods": lambda: c.g.compute_root_loglikelihoods([c.root[0]], [c.root[1]], bad),
        "rdamd_root_loglikelihood_fused": lambda: c.g.root_loglikelihood_fused(c.op, l1, l2, bad),
        "rdamd_root_loglikelihood_fused_multi": multi,
        "rdamd_marginal_ancestral": lambda: c.g.marginal_ancestral(ops, bad),
        "rdamd_site_rate_posteriors": lambda: c.g.site_rate_posteriors(*c.root, bad),
    }
    for name, call in calls.items():
        with pytest.raises(rd.RdamdError) as err:
            call()
        assert name + ":" in str(err.value), (name, str(err.value))
        assert rd.lib.rdamd_errno() == 7, name
        for x in cases if name.endswith("multi") else cases[:1]:
            assert util.rel_err(x.lh(x.g, x.rl, good, good), x.want) < LNL_TOL, name
    # the fallback of the fused root step (three categories) names itself as well
    c3 = Case(4, 3, M, 33, 933)
    rl = c3.rooting(True)
    want = c3.guard(rl, [2, 0, 1], [2, 0, 1])
    c3.lh(c3.g, rl, [2, 0, 1], [2, 0, 1])
    op = c3.tree.generate_derivative_operations(rl)[0]
    with pytest.raises(rd.RdamdError) as err:
        c3.g.root_loglikelihood_fused(op, *root_positions(rl), [2, M, 1])
    assert "rdamd_root_loglikelihood_fused:" in str(err.value), str(err.value)
    assert util.rel_err(c3.lh(c3.g, rl, [2, 0, 1], [2, 0, 1]), want) < LNL_TOL
    for x in cases + [c3]:
        x.close()


def test_setters_ignore_an_index_past_the_last_rate_matrix():
    """rdamd_set_subst_params / rdamd_set_frequencies return nothing: an index that names no rate matrix
    changes nothing, silently"""
    c = Case(4, 4, 3, 33, 950)
    pidx, fidx = [2, 0, 2, 1], [1, 1, 0, 2]
    rl = c.rooting(True)
    c.guard(rl, pidx, fidx)
    ops, pmi, brl = c.tree.generate_operations(rl)
    before = c.lh(c.g, rl, pidx, fidx)
    pm = [c.g.get_pmatrix(int(m)) for m in pmi]
    for idx in (3, 8):
        c.g.set_subst_params(idx, np.full(12, 0.5))
        c.g.set_frequencies(idx, [0.4, 0.3, 0.2, 0.1])
    assert c.lh(c.g, rl, pidx, fidx) == before
    assert all(np.array_equal(x, c.g.get_pmatrix(int(m))) for x, m in zip(pm, pmi))
    for m in range(3):
        assert list(c.g.subst_params(m)) == list(c.subst[m])
    c.close()
