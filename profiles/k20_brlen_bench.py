"""The 20-state branch-length derivative call (rdamd_branch_length_derivatives: HIP events around the
walk with its derivative consumer and the small launch that adds the tiles' partials, branch_last_ms)
against the ancestral-sequence call of the same walk (rdamd_ancestral_sequences,
ancestral_sequences_last_ms) and one materialising traversal (rdamd_update_clvs, profile family 0)
of the same partition, timed in the same process with the runs interleaved, on c3's shape: 200 taxa
x 10 000 sites, 20 states, four gamma categories (profiles/r19_k20_brlen.md).
usage: k20_brlen_bench.py [--taxa 200] [--sites 10000] [--rate-cats 4] [--runs 7]
One line: medians and minima over the runs after one warm-up run; d1 alone is the call with d2_out = NULL."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import root_digger_amd as rd  # noqa: E402
from root_digger_amd import synth  # noqa: E402
import util  # noqa: E402


def traversal_ms(p, ops):
    p.update_clvs(ops)
    return p.profile_read()["clv"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taxa", type=int, default=200)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--rate-cats", type=int, default=4)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    R, S = args.rate_cats, args.sites
    w = synth.workload(args.taxa, S, 20, R, 3, simulate_seqs=False)
    tree = rd.Tree.from_newick(w["newick"])
    p = rd.Partition.for_tree(tree, 20, S, R, rd.ATTRIB_NONREV)
    util.load_tips(p, tree, w["seqs"], util.make_map(w["alphabet"]))
    rng = np.random.default_rng(3)
    p.set_subst_params(0, rng.uniform(0.1, 1.5, 380))
    p.set_frequencies(0, rng.dirichlet(np.ones(20) * 4))
    p.set_category_rates(rd.compute_gamma_cats(1.0, R) if R > 1 else [1.0])
    p.set_pattern_weights(rng.integers(1, 6, S).astype(np.uint32))
    ops, pmi, brl = tree.generate_operations(tree.root_location(0).with_ratio(0.5))
    p.update_prob_matrices(pmi, brl)
    p.profile_enable(True)
    clv, walk, both, first = [], [], [], []
    for run in range(args.runs + 1):      # (the first run warms up)
        t_clv = traversal_ms(p, ops)
        p.ancestral_sequences(ops)
        t_walk = rd.ancestral_sequences_last_ms()
        d1, d2 = p.branch_length_derivatives(ops)
        t_both = rd.branch_last_ms()
        only, _ = p.branch_length_derivatives(ops, second=False)
        t_first = rd.branch_last_ms()
        assert only.tobytes() == d1.tobytes()
        if run:
            clv.append(t_clv)
            walk.append(t_walk)
            both.append(t_both)
            first.append(t_first)
    tips = tree.tip_count()
    inner = sum(1 for o in ops for c in (o.child1_clv_index, o.child2_clv_index) if c >= tips)
    branches = 2 * len(ops)
    print("k20 brlen: %d taxa x %d sites, R %d: d1 and d2 %.3f ms (min %.3f), d1 alone %.3f ms (min %.3f), ancestral "
          "sequences %.3f ms (min %.3f), traversal %.3f ms (min %.3f); ratios to the traversal %.2f, %.2f, %.2f; "
          "%d operations, %d branches of which %d above tips (%d MFMAs per wave with d2, %d without, %d in the posterior "
          "walk, %d in the traversal); largest |d1| %.3e, |d2| %.3e" % (
              tips, S, R, np.median(both), np.min(both), np.median(first), np.min(first), np.median(walk), np.min(walk),
              np.median(clv), np.min(clv), np.median(both) / np.median(clv), np.median(first) / np.median(clv),
              np.median(walk) / np.median(clv), len(ops), branches, branches - inner, 50 * inner + 50 * branches,
              50 * inner + 25 * branches, 50 * inner, 25 * inner, np.abs(d1).max(), np.abs(d2).max()), flush=True)


if __name__ == "__main__":
    main()
