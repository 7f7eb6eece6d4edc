"""The 20-state pair-sum call (rdamd_pair_sums: HIP events around the passes of the walk with its
pair-sum consumer and the launches that add the tiles' partials, pair_sums_last_ms) at three bounds on
the partials of one pass -- 256 MiB, 1 GiB and one pass -- against the branch-length derivative call
of the same walk (branch_last_ms) and one materialising traversal (rdamd_update_clvs, profile family
0) of the same partition, timed in the same process with the runs interleaved, on c3's shape: 200
taxa x 10 000 sites, 20 states, four gamma categories (profiles/r20_k20_pair_sums.md).  Then the HOST
time (wall clock) of rdamd_gradient_from_pair_sums and rdamd_substitution_counts_from_pair_sums at 20
states on those sums, and the wall time of one whole evaluation (P-matrices, traversal, root lnL):
381 of those are what a one-sided gradient of a protein partition costs L-BFGS-B.
usage: k20_pair_sums_bench.py [--taxa 200] [--sites 10000] [--rate-cats 4] [--runs 7] [--host-runs 3]
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


def traversal_ms(p, ops):
    p.update_clvs(ops)
    return p.profile_read()["clv"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taxa", type=int, default=200)
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--rate-cats", type=int, default=4)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=3)
    args = ap.parse_args()
    R, S = args.rate_cats, args.sites
    w = synth.workload(args.taxa, S, 20, R, 3, simulate_seqs=False)
    tree = rd.Tree.from_newick(w["newick"])
    p = rd.Partition.for_tree(tree, 20, S, R, rd.ATTRIB_NONREV)
    util.load_tips(p, tree, w["seqs"], util.make_map(w["alphabet"]))
    rng = np.random.default_rng(3)
    subst, freqs = rng.uniform(0.1, 1.5, 380), rng.dirichlet(np.ones(20) * 4)
    rates = np.array(rd.compute_gamma_cats(1.0, R) if R > 1 else [1.0])
    p.set_subst_params(0, subst)
    p.set_frequencies(0, freqs)
    p.set_category_rates(rates)
    p.set_pattern_weights(rng.integers(1, 6, S).astype(np.uint32))
    sched = tree.generate_operations(tree.root_location(0).with_ratio(0.5))
    ops, pmi, brl = sched
    p.update_prob_matrices(pmi, brl)
    p.profile_enable(True)
    tiles = -(-S // 16)
    row = 8 * (len(ops) * 2 * R * 400 + R * 21)
    bounds = [("256 MiB", 256 << 20), ("1 GiB", 1 << 30), ("one pass", tiles * row)]
    clv, brlen, pair = [], [], {name: [] for name, _ in bounds}
    whole = None
    for run in range(args.runs + 1):      # (the first run warms up)
        t_clv = traversal_ms(p, ops)
        p.branch_length_derivatives(ops)
        t_brlen = rd.branch_last_ms()
        t_pair = {}
        for name, bound in bounds:
            got = p.pair_sums(ops, workspace_bytes=bound)
            t_pair[name] = rd.pair_sums_last_ms()
            if whole is None:
                whole = got
            assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, got))
        if run:
            clv.append(t_clv)
            brlen.append(t_brlen)
            for name, _ in bounds:
                pair[name].append(t_pair[name])
    p.profile_enable(False)
    evals = []
    for run in range(args.runs + 1):
        t0 = time.perf_counter()
        p.update_prob_matrices(pmi, brl)
        p.update_clvs(ops)
        p.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())
        if run:
            evals.append(1e3 * (time.perf_counter() - t0))
    N, M, W = whole
    lengths = grad_ref.branch_lengths(*sched)
    wts = np.full(R, 1.0 / R)
    host_g, host_s = [], []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        rd.gradient_from_pair_sums(N, M, W, lengths, [subst], [freqs], [0] * R, [0] * R, rates, wts)
        host_g.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rd.substitution_counts(N, lengths, [subst], [freqs], [0] * R, rates)
        host_s.append(1e3 * (time.perf_counter() - t0))
    passes = ", ".join("%s (%d passes) %.3f ms (min %.3f)" % (name, -(-tiles // max(1, min(tiles, bound // row))),
                                                            np.median(pair[name]), np.min(pair[name])) for name, bound in bounds)
    best = min(np.median(pair[name]) for name, _ in bounds)
    print("k20 pair sums: %d taxa x %d sites, R %d, %d tiles, a row of partials %d bytes: pair sums at %s; branch-length "
          "derivatives %.3f ms (min %.3f); traversal %.3f ms (min %.3f); one evaluation (wall) %.3f ms (min %.3f), 381 of "
          "them %.1f ms; host: gradient_from_pair_sums %.1f ms (min %.1f), substitution_counts %.1f ms (min %.1f) for %d "
          "(branch, rate) block exponentials; the whole gradient %.1f ms = 1 evaluation + pair sums + host, %.1f x under 381 "
          "evaluations; largest N %.3e" % (
              tree.tip_count(), S, R, tiles, row, passes, np.median(brlen), np.min(brlen), np.median(clv), np.min(clv),
              np.median(evals), np.min(evals), 381 * np.median(evals), np.median(host_g), np.min(host_g), np.median(host_s),
              np.min(host_s), 2 * len(ops) * R, np.median(evals) + best + np.median(host_g),
              381 * np.median(evals) / (np.median(evals) + best + np.median(host_g)), N.max()), flush=True)


if __name__ == "__main__":
    main()
