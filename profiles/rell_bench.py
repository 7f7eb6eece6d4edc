"""Resampling step of the RELL bootstrap alone (rdamd_rell_bootstrap's sums kernel, HIP events
around it) on the three shapes of profiles/r8_rell.md.  usage: rell_bench.py [--shape small|c2|c5]
[--runs 3].  One line per run: kernel milliseconds and gathered bytes (B x N x rows x 8) per second."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import root_digger_amd as rd  # noqa: E402

SHAPES = {            # rows, patterns (unit weights), replicates
    "small": (17, 991, 10000),
    "c2": (197, 50000, 10000),
    "c5": (1997, 100000, 1000),
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
    args = ap.parse_args()
    for name in args.shape or ["small", "c2", "c5"]:
        rows, patterns, reps = SHAPES[name]
        m = matrix(rows, patterns, 1)
        w = np.ones(patterns, dtype=np.uint32)
        padded = -(-rows // 256) * 256 if rows > 128 else (-(-rows // 128) * 128 if rows > 64 else
                                                           64 if rows > 32 else 32 if rows > 16 else 16 if rows > 8 else 8)
        for run in range(args.runs):
            t = time.time()
            bp, elw = rd.rell_bootstrap(m, w, reps, seed=run + 1)
            wall = time.time() - t
            ms = rd.rell_last_resample_ms()
            gathered = reps * patterns * rows * 8.0
            print("%-5s %4d x %6d B = %5d run %d: resampling kernel %9.3f ms, %6.2f TB/s gathered "
                  "(table %.0f MB as stored), whole call %.2f s, best row %d bp %.4f"
                  % (name, rows, patterns, reps, run, ms, gathered / (ms * 1e-3) / 1e12, patterns * padded * 8 / 1e6,
                     wall, int(np.argmax(bp)), float(bp.max())), flush=True)


if __name__ == "__main__":
    main()
