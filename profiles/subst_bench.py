"""The substitution launch (rdamd_branch_substitutions: HIP events around its one launch,
branch_substitutions_last_ms), without and with joint_out, against the three other launches of the
pre-order walk on the same partition -- ancestral posteriors (ancestral_last_ms), branch-length
derivatives (branch_last_ms) and pair sums (pair_sums_last_ms) --, timed in the same process with
the runs interleaved, on the two inputs of profiles/r12_branch_lengths.md: c2's shape (100 taxa x
50 000 columns, four gamma categories) and 125.phy.  The host's share of a call (the count matrices:
one block exponential per branch and category, and their upload) is timed beside it.
usage: subst_bench.py [--input c2|d125] [--runs 7] [--no-joint]
One line per input."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import root_digger_amd as rd  # noqa: E402
import grad_ref  # noqa: E402
import util  # noqa: E402
from ancestral_bench import SUBST, FREQS, inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=["c2", "d125"], action="append")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-joint", action="store_true")
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
        lengths = grad_ref.branch_lengths(ops, [int(m) for m in pmi], brl)
        times = {k: [] for k in ("subst", "joint", "ancestral", "branch", "pair", "call")}
        for run in range(args.runs + 1):      # (the first run warms up)
            t0 = time.perf_counter()
            out = p.branch_substitutions(ops, lengths)
            t = {"call": 1e3 * (time.perf_counter() - t0), "subst": rd.branch_substitutions_last_ms(), "joint": float("nan")}
            if not args.no_joint:
                p.branch_substitutions(ops, lengths, joint=True)
                t["joint"] = rd.branch_substitutions_last_ms()
            p.marginal_ancestral(ops)
            t["ancestral"] = rd.ancestral_last_ms()
            p.branch_derivatives(ops)
            t["branch"] = rd.branch_last_ms()
            p.branch_pair_sums(ops)
            t["pair"] = rd.pair_sums_last_ms()
            if run:
                for k, v in t.items():
                    times[k].append(v)
        med = {k: float(np.median(v)) for k, v in times.items()}
        cells = 2 * len(ops) * S
        print("%s: %d taxa x %d patterns, R %d: substitutions %.3f ms (min %.3f, max %.3f; %.1f MB out), with joint_out %.3f ms "
              "(%.1f MB out); ancestral %.3f ms, branch derivatives %.3f ms, pair sums %.3f ms; ratio to the derivatives %.2f "
              "/ %.2f; whole call without joint_out %.1f ms on the host; %d runs; sum of n %.6e" % (
                  name, tree.tip_count(), S, R, med["subst"], np.min(times["subst"]), np.max(times["subst"]), cells * 25 / 1e6,
                  med["joint"], cells * 153 / 1e6, med["ancestral"], med["branch"], med["pair"], med["subst"] / med["branch"],
                  med["joint"] / med["branch"], med["call"], args.runs, out["count"].sum()), flush=True)


if __name__ == "__main__":
    main()
