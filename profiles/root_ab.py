#!/usr/bin/env python3
"""Time the root log-likelihood calls (csrc/kernels_root.hip) with the partition's own event timer
(profile_enable / profile_read, family `root`): the single call, the batch over all 2n - 3 root
CLVs of the all-directions schedule, and the one-launch root step with 8 positions, on shapes users
run.  One run = one process = one JSON line per (shape, call); another build of the library is
timed through profiles/with_ablation.py, in processes that alternate with this build's.
    python3 profiles/root_ab.py [--calls 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import root_digger_amd as rd          # noqa: E402
from root_digger_amd import synth     # noqa: E402
import util                           # noqa: E402

# name -> (tips, sites, states, rate categories)
SHAPES = {"c2": (100, 50000, 4, 4), "k4r3": (100, 50000, 4, 3), "c3": (200, 10000, 20, 4)}


def timed(part, calls, warmup, fn):
    for _ in range(warmup):
        fn()
    part.profile_read()
    for _ in range(calls):
        fn()
    ms, launches = part.profile_read()["root"]
    assert launches == calls, (launches, calls)
    return ms / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    for name, (n, S, K, R) in SHAPES.items():
        w = synth.workload(n, S, K, R, 77, simulate_seqs=False)
        tree = rd.Tree.from_newick(w["newick"])
        d = tree.generate_directional_operations()
        b = tree.branch_count()
        g = rd.Partition(n, max(d["clv_buffers"], b), K, S, 1, max(d["prob_matrices"], b), R,
                         max(d["scale_buffers"], b))
        util.load_tips(g, tree, w["seqs"], rd.MAP_NT if K == 4 else util.make_map(w["alphabet"]))
        g.set_subst_params(0, w["subst"])
        g.set_frequencies(0, g.empirical_frequencies())
        g.set_category_rates(w["rates"])
        g.update_prob_matrices(d["matrix_indices"], d["branch_lengths"])
        g.update_clvs(d["ops"])
        g.profile_enable(True)
        clv, sc = int(d["root_clv"][0]), int(d["root_scaler"][0])
        out = {"single": timed(g, args.calls, args.warmup, lambda: g.compute_root_loglikelihood(clv, sc)),
               "batch": timed(g, args.calls, args.warmup,
                              lambda: g.compute_root_loglikelihoods(d["root_clv"], d["root_scaler"]))}
        if name == "c2":
            rl = tree.root_location(17).with_ratio(0.4)
            util.compute_lh(g, tree, rl)
            op, _, _ = tree.generate_derivative_operations(rl)
            l1 = [rl.saved_brlen * a for a in np.linspace(0.1, 0.9, 8)]
            l2 = [rl.saved_brlen - x for x in l1]
            out["fused8"] = timed(g, args.calls, args.warmup, lambda: g.root_loglikelihood_fused(op, l1, l2))
        for call, ms in out.items():
            print(json.dumps({"library": os.path.relpath(rd.lib_path, ROOT), "shape": name, "call": call,
                              "calls": args.calls, "ms_per_call": round(ms, 6)}), flush=True)
        g.destroy()


if __name__ == "__main__":
    main()
