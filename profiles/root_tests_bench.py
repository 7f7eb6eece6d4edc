"""The KH / SH / weighted-SH stage of rdamd_rell_tests against the resampling kernel of the same
call (HIP events: rell_last_resample_ms, rell_last_tests_ms) on the two shapes of
profiles/r9_root_tests.md.  usage: root_tests_bench.py [--shape c2|t1000] [--runs 3] [--replicates B].
One line per run.  The O(n^2 B) work is counted from the shapes: pair terms = rows^2 x B (the WSH
kernel visits every ordered pair, the spread kernel every unordered pair of its upper tiles), and
the WSH kernel reads the rows^2 table of reciprocal spreads once per block of 64 replicates."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import root_digger_amd as rd  # noqa: E402

SHAPES = {            # rows, patterns (unit weights), replicates
    "c2": (197, 50000, 10000),
    "t1000": (1997, 50000, 10000),
}


def matrix(rows, patterns, seed):
    """negative site lnLs, neighbouring rows close to each other"""
    rng = np.random.default_rng(seed)
    base = -rng.uniform(1.0, 12.0, patterns)
    m = np.empty((rows, patterns))
    for i in range(rows):
        base = np.minimum(base + rng.normal(0.0, 0.02, patterns), -1e-3)
        m[i] = base
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replicates", type=int, default=0)
    args = ap.parse_args()
    for name in args.shape or ["c2", "t1000"]:
        rows, patterns, reps = SHAPES[name]
        reps = args.replicates or reps
        m = matrix(rows, patterns, 1)
        w = np.ones(patterns, dtype=np.uint32)
        rd.rell_tests(m[:, :64], w[:64], 64, seed=1)          # (code objects loaded, every kernel launched once)
        for run in range(args.runs):
            t = time.time()
            got = rd.rell_tests(m, w, reps, seed=run + 1)
            wall = time.time() - t
            resample, tests = rd.rell_last_resample_ms(), rd.rell_last_tests_ms()
            terms = float(rows) * rows * reps
            table_gb = float(rows) * rows * 8 * -(-reps // 64) / 1e9
            print("%-5s %4d x %6d B = %5d run %d: resampling %9.3f ms, everything after it %8.3f ms (ratio %.4f), "
                  "whole call %.2f s; %.3g pair terms, WSH table reads %.2f GB; kept at 0.05: KH %d SH %d WSH %d, "
                  "95%% ELW set %d"
                  % (name, rows, patterns, reps, run, resample, tests, tests / resample, wall, terms, table_gb,
                     int((got["p_kh"] >= 0.05).sum()), int((got["p_sh"] >= 0.05).sum()),
                     int((got["p_wsh"] >= 0.05).sum()), int(rd.elw_confidence_set(got["elw"]).sum())), flush=True)


if __name__ == "__main__":
    main()
