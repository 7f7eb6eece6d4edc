"""The 20-state pre-order walk (rdamd_ancestral_sequences: HIP events around the walk and the
arg-max, ancestral_sequences_last_ms) against one materialising traversal (rdamd_update_clvs,
profile family 0) of the same partition, timed in the same process with the runs interleaved, on
c3's shape: 200 taxa x 10 000 sites, 20 states, four gamma categories (profiles/r18_k20_preorder.md).
usage: k20_ancestral_bench.py [--taxa 200] [--sites 10000] [--rate-cats 4] [--runs 7]
One line: medians and minima over the runs after one warm-up run."""
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
    ops, pmi, brl = tree.generate_operations(tree.root_location(0).with_ratio(0.5))
    p.update_prob_matrices(pmi, brl)
    p.profile_enable(True)
    clv, walk = [], []
    for run in range(args.runs + 1):      # (the first run warms up)
        t_clv = traversal_ms(p, ops)
        p.ancestral_sequences(ops)
        if run:
            clv.append(t_clv)
            walk.append(rd.ancestral_sequences_last_ms())
    slots = rd.ancestral_workspace_slots(ops, tree.tip_count())
    tiles = (S + 15) // 16
    inner = sum(1 for o in ops for c in (o.child1_clv_index, o.child2_clv_index) if c >= tree.tip_count())
    print("k20: %d taxa x %d sites, R %d: walk + arg-max %.3f ms (min %.3f), traversal %.3f ms (min %.3f), ratio %.2f; "
          "%d operations, %d inner children (%d MFMAs per wave in the walk, %d in the traversal); workspace %d slots = "
          "%.1f MB; posterior table %.1f MB" % (
              tree.tip_count(), S, R, np.median(walk), np.min(walk), np.median(clv), np.min(clv),
              np.median(walk) / np.median(clv), len(ops), inner, 50 * inner, 25 * inner, slots,
              slots * R * tiles * 320 * 8 / 1e6, len(ops) * S * 160 / 1e6), flush=True)


if __name__ == "__main__":
    main()
