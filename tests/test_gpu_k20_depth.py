"""The 20-state fused evaluator (kernels_fused_k20.hip) at and beyond the stack depth its LDS holds.

A workgroup of fused20_eval_kernel is one wave per rate category R; each wave keeps one A copy and
its stack levels in LDS.  Programs deeper than the LDS of a CU holds at this R keep their lower
levels in global memory.  Balanced trees need the deepest stacks a tree of their size can ask for
(the depth grows with the log of the tip count), so the cases below are chosen by the depth the
schedule reports, on both sides of every limit, and checked against the CPU oracle through every
entry point: the batch, the exporting variant (dense and sparse partitions), the materialising
traversal, and the model (compute_lh, compute_lh_batch, optimize_params).  The largest trees
(4 096 taxa and more) are checked against the materialising traversal kernels of a second
partition instead: the oracle needs minutes there, and those kernels are checked against it
elsewhere (test_gpu_parity.py).  Random unrelated
sequences make the rescaling fire on the way up, so parked rescale counts pass through the levels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import synth
import util
from oracle_lib import OraclePartition
from test_gpu_parity import LNL_TOL

pytestmark = pytest.mark.gpu

# The kernel's LDS layout, restated: per wave a 16-site root exchange (8 + 4 bytes per site), one
# A copy of 4 KB and 2816 bytes per stack level; one workgroup may have the 160 KB of a CU.
ROOT_XCHG, A_COPY, LEVEL, LDS_BYTES = 16 * 12, 4096, 5 * 64 * 8 + 64 * 4, 160 * 1024


def d_max(R):
    """the deepest stack that fits in LDS at R rate categories: 56, 27, 17, 13, 10, 8, 6, 5"""
    return (LDS_BYTES // R - ROOT_XCHG - A_COPY) // LEVEL


AA = synth.AA
CMAP = util.make_map(AA)


def _setup(n_tips, S, R, seed):
    rng = np.random.default_rng(seed)
    tree = rd.Tree.from_newick(util.balanced_newick(n_tips, rng))
    seqs = {"t%d" % i: "".join(AA[k] for k in rng.integers(0, 20, S)) for i in range(n_tips)}
    weights = rng.integers(1, 4, size=S).astype(np.uint32)
    return rng, tree, seqs, weights


def _gpu(tree, seqs, S, R, weights, attributes=0):
    g = rd.Partition.for_tree(tree, 20, S, R, attributes)
    util.load_tips(g, tree, seqs, CMAP, weights)
    return g


def _comb_tree(tree, n_tips, rng, block=64):
    """the same taxa as a comb of balanced 64-taxon clades (a shallow stack), labelled so that every
    taxon keeps its tip index: schedules of both trees run on the same partition"""
    lens = rng.uniform(0.02, 0.3, 4 * n_tips)
    def newick(label):
        k = iter(lens)
        def clade(lo, hi):
            nodes = ["%s:%.5f" % (label(i), next(k)) for i in range(lo, hi)]
            while len(nodes) > 1:
                nodes = ["(%s,%s):%.5f" % (nodes[i], nodes[i + 1], next(k)) for i in range(0, len(nodes), 2)]
            return nodes[0]
        blocks = [clade(b, min(b + block, n_tips)) for b in range(0, n_tips, block)]
        s = blocks[-1]
        for b in reversed(blocks[1:-1]):
            s = "(%s,%s):%.5f" % (b, s, next(k))
        return "(%s,%s);" % (blocks[0], s)
    shape = rd.Tree.from_newick(newick(lambda i: "x%d" % i))
    by_index = {tree.tip_index("t%d" % i): "t%d" % i for i in range(n_tips)}
    comb = rd.Tree.from_newick(newick(lambda i: by_index[shape.tip_index("x%d" % i)]))
    assert all(comb.tip_index("t%d" % i) == tree.tip_index("t%d" % i) for i in range(n_tips))
    return comb


def _pick_roots(g, tree, rng):
    """the deepest of a sample of root locations (the central branch of a balanced tree is among the
    last ones) and two random others, each with its schedule"""
    n = tree.root_count()
    cand = sorted(set(range(max(0, n - 4), n)) | set(int(i) for i in rng.choice(n, min(n, 8), replace=False)))
    depth = {i: g.schedule(*tree.generate_operations(tree.root_location(i))).stack_depth() for i in cand}
    deep = max(cand, key=lambda i: (depth[i], -i))
    others = [int(i) for i in rng.choice([i for i in range(n) if i != deep], 2, replace=False)]
    rls = [tree.root_location(i).with_ratio(float(rng.uniform(0.1, 0.9))) for i in [deep] + others]
    scheds = [g.schedule(*tree.generate_operations(rl)) for rl in rls]
    return rls, scheds


def _params(rng, n, R):
    subst = rng.uniform(1e-3, 1.0, (n, 380))
    freqs = rng.dirichlet(np.ones(20) * 5, n)
    rates = np.array([rd.compute_gamma_cats(a, R) for a in rng.uniform(0.3, 3.0, n)])
    cw = rng.dirichlet(np.ones(R) * 3, n)
    return subst, freqs, rates, cw


def _oracle(o, tree, rl, subst, freqs, rates, cw):
    o.set_subst_params(0, subst)
    o.set_frequencies(0, freqs)
    o.set_category_rates(rates)
    o.set_category_weights(cw)
    return util.compute_lh(o, tree, rl)


def _clv_close(a, sa, b, sb, rtol=1e-12):
    """CLVs ([site][rate][state]) with per-site counts of 2^256 rescales: the same numbers, each entry
    within rtol of the largest entry of its site.  (Deep trees leave a rate category several 2^256
    rescales behind the site's largest; the oracle's per-site rule takes such a category through the
    denormal range and loses its bits, the evaluator's per-(site, rate) counts keep them -- a part
    of the site the lnL cannot see.)  Returns (ok, worst error relative to its site, where)."""
    sa = sa.astype(np.int64)[:, None, None]
    sb = sb.astype(np.int64)[:, None, None]
    lo = np.minimum(sa, sb)
    fa = np.ldexp(a, (-256 * (sa - lo)).astype(np.int64))
    fb = np.ldexp(b, (-256 * (sb - lo)).astype(np.int64))
    site = np.maximum(np.abs(fa), np.abs(fb)).max(axis=(1, 2), keepdims=True)
    err = np.abs(fa - fb) / np.maximum(site, 1e-300)
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    return bool(np.all(np.abs(fa - fb) <= rtol * site + 1e-250)), float(err.max()), worst


def _children_match(part, o, tree, rl, subst, freqs, rates, cw, want):
    """rdamd_evaluate_root_children on `part` against the oracle, which holds the traversal of rl
    with these parameters: the lnL, and both inner children's CLVs and per-site scalers"""
    ops, pmi, brl = tree.generate_operations(rl)
    got = part.evaluate_root_children(ops, pmi, brl, subst, freqs, rates, cw)
    assert util.rel_err(got, want) < LNL_TOL, (got, want)
    root = ops[len(ops) - 1]
    seen = 0
    for clv, sc in ((root.child1_clv_index, root.child1_scaler_index),
                    (root.child2_clv_index, root.child2_scaler_index)):
        if clv < tree.tip_count():
            continue
        gs = part.get_scaler(sc)
        ok, worst, where = _clv_close(part.get_clv(clv), gs, o.get_clv(clv), o.get_scaler(sc))
        assert ok, (clv, worst, where)
        seen = max(seen, int(gs.max()))
    return got, seen


# (R, tips, sites, target depth, reference): every rooting of a balanced tree of 2^k taxa has a
# stack of k - 3 levels.  R = 5 over its limit (11 levels) takes 16 384 taxa, and that case alone
# took 106 s (tip loading and schedules of 32 765 rootings' worth of tree): it is left out; the
# R = 5 launch at its limit and R = 6 one level over it cover the same code.
CASES = [
    (8, 256, 49, d_max(8), "oracle"), (8, 512, 33, d_max(8) + 1, "oracle"),
    (7, 512, 37, d_max(7), "oracle"), (7, 1024, 33, d_max(7) + 1, "oracle"),
    (6, 2048, 33, d_max(6), "oracle"), (6, 4096, 33, d_max(6) + 1, "traversal"),
    (5, 8192, 33, d_max(5), "traversal"),
    (4, 512, 130, 6, "oracle"),   # the 256-thread instantiation on a deep tree (its limit, 13, needs 2^16 taxa)
]


@pytest.mark.parametrize("R,n_tips,S,target,reference", CASES,
                         ids=["R%d-%dtips-depth%d" % (c[0], c[1], c[3]) for c in CASES])
def test_k20_stack_depth_vs_oracle(R, n_tips, S, target, reference):
    assert [d_max(r) for r in range(1, 9)] == [56, 27, 17, 13, 10, 8, 6, 5]
    rng, tree, seqs, weights = _setup(n_tips, S, R, 1000 * R + n_tips)
    g = _gpu(tree, seqs, S, R, weights)
    if reference == "oracle":
        o = OraclePartition.for_tree(tree, 20, S, R)
        util.load_tips(o, tree, seqs, CMAP, weights)
    else:
        o = _gpu(tree, seqs, S, R, weights)
    rls, scheds = _pick_roots(g, tree, rng)
    depths = [s.stack_depth() for s in scheds]
    # the case means what it says: the deepest rooting sits exactly at (or one over) the limit
    assert depths[0] == target, depths
    assert max(depths) == depths[0], depths
    over = target > d_max(R)

    subst, freqs, rates, cw = _params(rng, 3, R)
    got = g.evaluate_batch(scheds, subst, freqs, rates, cw)
    assert np.array_equal(got, g.evaluate_batch(scheds, subst, freqs, rates, cw))   # repeat: bit-identical
    want = [None] * 3
    for j in (2, 1, 0):   # (the deep rooting last: the oracle keeps its CLVs for the checks below)
        want[j] = _oracle(o, tree, rls[j], subst[j], freqs[j], rates[j], cw[j])
    for j in range(3):
        assert util.rel_err(got[j], want[j]) < LNL_TOL, (j, depths[j], got[j], want[j])

    if over:
        # what the lock-step combiner makes: a job that fits next to one that does not, in one
        # launch (the shallow one: the same taxa as a comb of balanced clades)
        comb = _comb_tree(tree, n_tips, rng)
        rl_c = comb.root_location(0).with_ratio(0.3)
        sc = g.schedule(*comb.generate_operations(rl_c))
        assert sc.stack_depth() <= d_max(R) < depths[0], (sc.stack_depth(), depths)
        want_c = _oracle(o, comb, rl_c, subst[1], freqs[1], rates[1], cw[1])
        mixed = g.evaluate_batch([sc, scheds[0]], subst[[1, 0]], freqs[[1, 0]], rates[[1, 0]], cw[[1, 0]])
        assert util.rel_err(mixed[0], want_c) < LNL_TOL and util.rel_err(mixed[1], want[0]) < LNL_TOL
        alone = g.evaluate_batch([sc], subst[1:2], freqs[1:2], rates[1:2], cw[1:2])
        assert util.rel_err(alone[0], mixed[0]) < 1e-13
        want[0] = _oracle(o, tree, rls[0], subst[0], freqs[0], rates[0], cw[0])   # (its CLVs back)

    # the exporting variant on a dense and on a sparse partition (a replica's)
    p0 = (subst[0], freqs[0], rates[0], cw[0])
    lnl, seen = _children_match(g, o, tree, rls[0], *p0, want[0])
    assert seen >= 1   # the children really carry rescale counts
    sp = _gpu(tree, seqs, S, R, weights, rd.ATTRIB_NONREV | rd.ATTRIB_SPARSE_CLVS)
    sp_lnl, _ = _children_match(sp, o, tree, rls[0], *p0, want[0])
    assert sp_lnl == lnl
    sp.destroy()

    # the materialising path (P-matrices + the MFMA traversal kernel) on the same partition
    g.set_subst_params(0, subst[0])
    g.set_frequencies(0, freqs[0])
    g.set_category_rates(rates[0])
    g.set_category_weights(cw[0])
    trav = util.compute_lh(g, tree, rls[0])
    assert util.rel_err(trav, want[0]) < LNL_TOL
    assert util.rel_err(trav, got[0]) < 1e-11
    g.destroy()
    o.destroy()


def _model(tree, seqs, R, weights):
    m = rd.Model(tree, seqs, states=20, cmap=CMAP, rate_cats=R, weights=weights, seed=7)
    m.initialize_partitions()
    return m


def _oracle_model(o, tree, rl, subst, freqs, alpha, R):
    o.set_subst_params(0, subst)
    o.set_frequencies(0, freqs)
    o.set_category_rates(rd.compute_gamma_cats(alpha, R, rd.GAMMA_RATES_MEDIAN))
    o.set_category_weights([1.0 / R] * R)
    return util.compute_lh(o, tree, rl)


def test_k20_model_over_the_lds_limit():
    """rd.Model at eight rate categories on a balanced tree whose deepest rooting does not fit in
    LDS: compute_lh, compute_lh_batch and one optimize_params against the oracle"""
    R, n_tips, S = 8, 512, 35
    rng, tree, seqs, weights = _setup(n_tips, S, R, 8256)
    g = _gpu(tree, seqs, S, R, weights)
    rls, scheds = _pick_roots(g, tree, rng)
    depths = [s.stack_depth() for s in scheds]
    assert min(depths) == d_max(R) + 1, depths
    g.destroy()
    o = OraclePartition.for_tree(tree, 20, S, R)
    util.load_tips(o, tree, seqs, CMAP, weights)
    m = _model(tree, seqs, R, weights)
    subst = rng.uniform(0.05, 2.0, 380)
    freqs = rng.dirichlet(np.ones(20) * 5)
    m.set_subst_rates(subst)
    m.set_freqs(freqs)
    m.set_gamma_alpha(0.8)
    want = [_oracle_model(o, tree, rl, subst, freqs, 0.8, R) for rl in rls[:2]]   # (both over the limit)
    assert util.rel_err(m.compute_lh(rls[0]), want[0]) < LNL_TOL
    batch = m.compute_lh_batch(rls[:2], [subst] * 2, [freqs] * 2, [0.8, 0.8])
    for a, b in zip(batch, want):
        assert util.rel_err(a, b) < LNL_TOL

    ref = os.path.join(util.ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/liblbfgsb_ref.so not built (needs /root/reference at build time)")
    import ctypes
    lb = ctypes.CDLL(ref)
    # one optimisation over the limit: it runs, improves, and ends where the oracle puts its lnL
    subst0, freqs0 = [1.0 / 380] * 380, [0.05] * 20
    for rl in rls[:1]:
        m.set_lbfgsb(lb.setulb)
        m.set_subst_rates(subst0)
        m.set_freqs(freqs0)
        m.set_gamma_alpha(1.0)
        before = m.compute_lh(rl)
        res = m.optimize_params(rl, subst0, freqs0, 1.0, pgtol=1e-2, factor=1e12)
        assert res["evaluations"] >= 381
        fr = np.array(res["freqs"]) / np.sum(res["freqs"])
        m.set_subst_rates(res["subst"])
        m.set_freqs(fr)
        m.set_gamma_alpha(res["gamma_alpha"])
        after = m.compute_lh(rl)
        assert after > before + 1.0, (before, after)
        assert util.rel_err(after, _oracle_model(o, tree, rl, res["subst"], fr, res["gamma_alpha"], R)) < LNL_TOL
    m.destroy()
    o.destroy()


_ORDER_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.dirname(sys.argv[1]))
import root_digger_amd as rd
import util
import test_gpu_k20_depth as t
out = {}
for key, R, n_tips, S, seed in (("deep8", 8, 512, 35, 1), ("shallow5", 5, 32, 35, 2)):
    rng, tree, seqs, weights = t._setup(n_tips, S, R, seed)
    g = t._gpu(tree, seqs, S, R, weights)
    rls, scheds = t._pick_roots(g, tree, rng)
    subst, freqs, rates, cw = t._params(rng, 1, R)
    out[key] = {"depth": scheds[0].stack_depth(), "lnl": float(g.evaluate_batch(scheds[:1], subst, freqs, rates, cw)[0])}
    if key == "deep8":
        keep = (g, tree, rls[0], subst[0], freqs[0], rates[0], cw[0])
g, tree, rl, subst, freqs, rates, cw = keep
ops, pmi, brl = tree.generate_operations(rl)
out["export8"] = g.evaluate_root_children(ops, pmi, brl, subst, freqs, rates, cw)
print(json.dumps(out))
"""


def test_k20_launch_order_does_not_leak_lds_settings():
    """One process: a deep launch at R = 8 (the 512-thread instantiation raises its LDS limit),
    then a shallow one at R = 5 (same instantiation, less LDS), then the exporting variant at R = 8
    (another instantiation, which must raise its own).  A child process, so that no earlier test
    has raised anything."""
    here = os.path.dirname(os.path.abspath(__file__))
    res = subprocess.run([sys.executable, "-c", _ORDER_CHILD, here], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=300, cwd=here)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["deep8"]["depth"] == d_max(8) + 1 and out["shallow5"]["depth"] <= d_max(5), out
    # the same cases, rebuilt here (same seeds), on the oracle
    for key, R, n_tips, S, seed in (("deep8", 8, 512, 35, 1), ("shallow5", 5, 32, 35, 2)):
        rng, tree, seqs, weights = _setup(n_tips, S, R, seed)
        g = _gpu(tree, seqs, S, R, weights)
        rls, _ = _pick_roots(g, tree, rng)
        g.destroy()
        subst, freqs, rates, cw = _params(rng, 1, R)
        o = OraclePartition.for_tree(tree, 20, S, R)
        util.load_tips(o, tree, seqs, CMAP, weights)
        want = _oracle(o, tree, rls[0], subst[0], freqs[0], rates[0], cw[0])
        o.destroy()
        assert util.rel_err(out[key]["lnl"], want) < LNL_TOL, (key, out[key], want)
        if key == "deep8":
            assert util.rel_err(out["export8"], want) < LNL_TOL, (out["export8"], want)
