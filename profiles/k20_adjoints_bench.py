"""The adjoints of the 20-state pair sums (rdamd_pair_sum_adjoints) on c3's shape: 200 taxa x 10 000
sites, 20 states, four gamma categories, in one process with the runs interleaved
(profiles/r21_k20_adjoints.md):
  - the device route: the kernel alone (HIP events, pair_sum_adjoints_last_ms) and the whole call with
    its allocations and copies (wall clock);
  - the host route (wall clock);
  - the two assemblies from the adjoints (wall clock);
  - rdamd_pair_sums beside them (HIP events, pair_sums_last_ms, and the whole call, wall clock);
  - the whole Model.gradient and the whole Model.substitutions(per_site=False) of a protein model (wall
    clock).
On a tree without rdamd_pair_sum_adjoints (the parent commit) only the pair sums and the two model calls
are timed, so the same script gives both sides of the comparison.
usage: k20_adjoints_bench.py [--taxa 200] [--sites 10000] [--rate-cats 4] [--runs 9] [--host-runs 3]
One line: medians and minima over the runs after one warm-up run."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import root_digger_amd as rd  # noqa: E402
from root_digger_amd import synth  # noqa: E402
import grad_ref  # noqa: E402
import util  # noqa: E402


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return 1e3 * (time.perf_counter() - t0), out


def figure(values):
    return "%.3f ms (min %.3f)" % (np.median(values), np.min(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taxa", type=int, default=200)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--rate-cats", type=int, default=4)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--host-runs", type=int, default=3)
    args = ap.parse_args()
    R, S = args.rate_cats, args.sites
    have = hasattr(rd, "pair_sum_adjoints")
    w = synth.workload(args.taxa, S, 20, R, 3, simulate_seqs=False)
    cmap = util.make_map(w["alphabet"])
    tree = rd.Tree.from_newick(w["newick"])
    p = rd.Partition.for_tree(tree, 20, S, R, rd.ATTRIB_NONREV)
    util.load_tips(p, tree, w["seqs"], cmap)
    rng = np.random.default_rng(3)
    subst, freqs = rng.uniform(0.1, 1.5, 380), rng.dirichlet(np.ones(20) * 4)
    rates = np.array(rd.compute_gamma_cats(1.0, R) if R > 1 else [1.0])
    p.set_subst_params(0, subst)
    p.set_frequencies(0, freqs)
    p.set_category_rates(rates)
    p.set_pattern_weights(rng.integers(1, 6, S).astype(np.uint32))
    rl = tree.root_location(0).with_ratio(0.5)
    sched = tree.generate_operations(rl)
    ops, pmi, brl = sched
    p.update_prob_matrices(pmi, brl)
    p.update_clvs(ops)
    lengths = grad_ref.branch_lengths(*sched)
    wts = np.full(R, 1.0 / R)
    model_args = (lengths, [subst], [freqs], [0] * R, rates)

    mtree = rd.Tree.from_newick(w["newick"])
    m = rd.Model(mtree, w["seqs"], states=20, cmap=cmap, rate_cats=R, seed=3)
    m.initialize_partitions()
    mrl = mtree.root_location(0).with_ratio(0.5)
    m.compute_lh(mrl)   # (the first evaluation of a model builds its schedules)
    pp = {"subst_rates": subst.tolist(), "freqs": freqs.tolist(), "gamma_alpha": [1.0], "gamma_weights": []}

    t = {k: [] for k in ("pair_dev", "pair_wall", "adj_dev", "adj_wall", "asm_g", "asm_s", "gradient", "substitutions")}
    F = None
    for run in range(args.runs + 1):      # (the first run warms up)
        row = {}
        row["pair_wall"], (N, M, W) = wall(lambda: p.pair_sums(ops))
        row["pair_dev"] = rd.pair_sums_last_ms()
        if have:
            row["adj_wall"], got = wall(lambda: rd.pair_sum_adjoints(N, *model_args, where="device"))
            row["adj_dev"] = rd.pair_sum_adjoints_last_ms()
            assert F is None or got.tobytes() == F.tobytes()
            F = got
            row["asm_g"], _ = wall(lambda: rd.gradient_from_adjoints(F, M, W, lengths, [subst], [freqs], [0] * R, [0] * R, rates, wts))
            row["asm_s"], _ = wall(lambda: rd.substitution_counts_from_adjoints(F, *model_args))
        row["gradient"], _ = wall(lambda: m.gradient(mrl, [pp]))
        row["substitutions"], _ = wall(lambda: m.substitutions(mrl, [pp], per_site=False))
        if run:
            for k, v in row.items():
                t[k].append(v)
    head = "k20 adjoints: %d taxa x %d sites, R %d, %d (branch, rate) problems: " % (tree.tip_count(), S, R, 2 * len(ops) * R)
    tail = "rdamd_pair_sums %s on the device, %s the whole call; Model.gradient %s; Model.substitutions(per_site=False) %s" % (
        figure(t["pair_dev"]), figure(t["pair_wall"]), figure(t["gradient"]), figure(t["substitutions"]))
    if not have:
        print(head + "no rdamd_pair_sum_adjoints in this tree; " + tail, flush=True)
        return
    host = []
    for _ in range(args.host_runs):
        ms, H = wall(lambda: rd.pair_sum_adjoints(N, *model_args, where="host"))
        host.append(ms)
    scale = np.abs(H).reshape(-1, 400).max(axis=1)
    diff = float((np.abs(F - H).reshape(-1, 400).max(axis=1) / scale).max())
    print(head + "device adjoints %s the kernel, %s the whole call; host route %s; gradient_from_adjoints %s, "
          "substitution_counts_from_adjoints %s; adjoints + gradient assembly %.3f ms; %s; largest max|F_dev - F_host| / "
          "max|F_host| %.3e" % (figure(t["adj_dev"]), figure(t["adj_wall"]), figure(host), figure(t["asm_g"]), figure(t["asm_s"]),
                                np.median(t["adj_wall"]) + np.median(t["asm_g"]), tail, diff), flush=True)


if __name__ == "__main__":
    main()
