"""The pair-sum launch (rdamd_branch_pair_sums: HIP events around its launches, pair_sums_last_ms)
against the branch-length derivative launch (rdamd_branch_derivatives, branch_last_ms) on the same
partition, timed in the same process with the runs interleaved, on the two inputs of
profiles/r12_branch_lengths.md: c2's shape (100 taxa x 50 000 columns, four gamma categories) and
125.phy.  With --workspace-mib also the pair sums under that bound on the partial sums of one pass.
usage: pair_sums_bench.py [--input c2|d125] [--runs 7] [--workspace-mib N]
One line per input."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import root_digger_amd as rd  # noqa: E402
import util  # noqa: E402
from ancestral_bench import SUBST, FREQS, inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=["c2", "d125"], action="append")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--workspace-mib", type=int, default=0)
    args = ap.parse_args()
    R = 4
    for name in args.input or ["c2", "d125"]:
        tree, seqs = inputs(name)
        S = len(next(iter(seqs.values())))
        p = rd.Partition.for_tree(tree, 4, S, R, rd.ATTRIB_NONREV)
        util.load_tips(p, tree, seqs, rd.MAP_NT)
        p.set_subst_params(0, SUBST)
        p.set_frequencies(0, FREQS)
        p.set_category_rates(rd.compute_gamma_cats(1.0, R))
        ops, pmi, brl = tree.generate_operations(tree.root_location(0).with_ratio(0.5))
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
        pair, branch, cut = [], [], []
        for run in range(args.runs + 1):      # (the first run warms up)
            N, M, W = p.branch_pair_sums(ops)
            t_pair = rd.pair_sums_last_ms()
            p.branch_derivatives(ops)
            t_branch = rd.branch_last_ms()
            t_cut = float("nan")
            if args.workspace_mib:
                p.branch_pair_sums(ops, workspace_bytes=args.workspace_mib << 20)
                t_cut = rd.pair_sums_last_ms()
            if run:
                pair.append(t_pair)
                branch.append(t_branch)
                cut.append(t_cut)
        print("%s: %d taxa x %d patterns, R %d: pair sums %.3f ms (min %.3f, max %.3f), branch derivatives %.3f ms "
              "(min %.3f, max %.3f), ratio %.2f; under %d MiB %.3f ms; %d runs; largest N %.3e" % (
                  name, tree.tip_count(), S, R, np.median(pair), np.min(pair), np.max(pair), np.median(branch),
                  np.min(branch), np.max(branch), np.median(pair) / np.median(branch), args.workspace_mib, np.median(cut),
                  args.runs, N.max()), flush=True)


if __name__ == "__main__":
    main()
