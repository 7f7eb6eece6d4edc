"""The branch-length derivative launch (rdamd_branch_derivatives: HIP events around its two launches,
branch_last_ms) against the pre-order pass of the ancestral states (rdamd_marginal_ancestral,
ancestral_last_ms) on the same partition, timed in the same process with the runs interleaved, on the
two inputs of profiles/r12_branch_lengths.md: c2's shape (100 taxa x 50 000 columns, four gamma
categories) and 125.phy.  With --optimize also the wall time of one Model.optimize_branch_lengths on c2
and its evaluation count.
usage: brlen_bench.py [--input c2|d125] [--runs 7] [--optimize] [--baseline-library PATH/librdamd.so]
--baseline-library: another build of the library (the previous commit's), loaded next to this one;
its rdamd_marginal_ancestral runs on a partition of its own with the same data and is the yardstick,
and this build's own ancestral pass is timed next to it (it must not have moved).  One line per input."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import root_digger_amd as rd  # noqa: E402
from root_digger_amd import synth  # noqa: E402
import util  # noqa: E402
from ancestral_bench import SUBST, FREQS, BaselinePartition, inputs  # noqa: E402


class BaselineAncestral(BaselinePartition):
    """the same partition in another build of the library: traverse once, then time its pre-order pass"""

    def ancestral_ms(self, ops, post):
        lib = self.lib
        lib.rdamd_ancestral_last_ms.restype = C.c_double
        fi = np.zeros(4, dtype=np.uint32)
        rc = lib.rdamd_marginal_ancestral(self.h, ops, C.c_uint(len(ops)), fi.ctypes.data_as(C.POINTER(C.c_uint)),
                                          post.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 1:
            raise RuntimeError("the baseline library's rdamd_marginal_ancestral failed")
        return float(lib.rdamd_ancestral_last_ms())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=["c2", "d125"], action="append")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--optimize", action="store_true")
    ap.add_argument("--baseline-library")
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
        rl = tree.root_location(0).with_ratio(0.5)
        ops, pmi, brl = tree.generate_operations(rl)
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
        base = None
        if args.baseline_library:
            base = BaselineAncestral(args.baseline_library, tree, seqs, R)
            base.traversal_ms(ops, pmi, brl)
            post = np.zeros((len(ops), S, 4))
        own, parent, branch = [], [], []
        for run in range(args.runs + 1):      # (the first run warms up)
            p.marginal_ancestral(ops)
            t_own = rd.ancestral_last_ms()
            t_parent = base.ancestral_ms(ops, post) if base else float("nan")
            d1, d2 = p.branch_derivatives(ops)
            if run:
                own.append(t_own)
                parent.append(t_parent)
                branch.append(rd.branch_last_ms())
        yard = np.median(parent) if base else np.median(own)
        print("%s: %d taxa x %d patterns, R %d: branch derivatives %.3f ms (min %.3f, max %.3f), ancestral pass %.3f ms "
              "(min %.3f, max %.3f; parent build %.3f ms), ratio %.2f; %d runs; largest |d1| %.3e" % (
                  name, tree.tip_count(), S, R, np.median(branch), np.min(branch), np.max(branch), np.median(own), np.min(own),
                  np.max(own), np.median(parent), np.median(branch) / yard, args.runs, np.abs(d1).max()), flush=True)
        if args.optimize and name == "c2":
            m = rd.Model(tree, seqs, rate_cats=R, seed=3)
            m.initialize_partitions()
            m.compute_lh(rl)   # (the first evaluation of a model builds its schedules)
            t0 = time.perf_counter()
            r = m.optimize_branch_lengths(rl, None, 1e-6, 100.0, 1e-8, 200)
            wall = time.perf_counter() - t0
            print("c2 optimisation: %.3f s wall, %d iterations, %d evaluations (%.1f ms each), lnL %.6f -> %.6f, converged %s" % (
                wall, r["iterations"], r["evaluations"], 1e3 * wall / r["evaluations"], r["lnl_before"], r["lnl_after"],
                r["converged"]), flush=True)


if __name__ == "__main__":
    main()
