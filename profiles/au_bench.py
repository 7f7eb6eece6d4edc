"""The multiscale resampling of the AU test (rdamd_rell_multiscale: HIP events around its launches,
rell_last_multiscale_ms) against what its ten scales would cost as single-scale bootstraps:
(sum of M_k / N) x the resampling kernel of one rdamd_rell_bootstrap call (rell_last_resample_ms),
on the two shapes of profiles/r10_au.md.
usage: au_bench.py [--shape c2|c5|w8|w16|w32|w64|w128] [--runs 3] [--baseline-library PATH/librdamd.so]
(default: c2 and c5; the w shapes are the narrower launch shapes on 20 000 columns)
--baseline-library: another build of the library (the previous commit's), loaded next to this one;
its rdamd_rell_bootstrap runs on the same matrix in the same process and is the yardstick, and this
build's own kernel is timed next to it (it must not have moved).  One line per run."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import root_digger_amd as rd  # noqa: E402

SHAPES = {            # rows, patterns (unit weights), replicates per scale
    "c2": (197, 50000, 10000),
    "c5": (1997, 100000, 1000),
    # the narrower launch shapes: 8, 16, 32, 64 lanes per replicate with one row per lane, 64 with two
    "w8": (8, 20000, 4000), "w16": (16, 20000, 4000), "w32": (32, 20000, 4000), "w64": (64, 20000, 4000),
    "w128": (128, 20000, 4000),
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


class Baseline:
    """rdamd_rell_bootstrap of another build of the library"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        pd, pu, u = C.POINTER(C.c_double), C.POINTER(C.c_uint), C.c_uint
        self.lib.rdamd_rell_bootstrap.restype = C.c_int
        self.lib.rdamd_rell_bootstrap.argtypes = [pd, u, u, pu, u, C.c_uint64, pd, pd, pd]
        self.lib.rdamd_rell_last_resample_ms.restype = C.c_double
        self.lib.rdamd_version.restype = C.c_char_p

    def resample_ms(self, m, w, reps, seed):
        pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint)
        bp, elw = np.zeros(m.shape[0]), np.zeros(m.shape[0])
        if self.lib.rdamd_rell_bootstrap(m.ctypes.data_as(pd), m.shape[0], m.shape[1], w.ctypes.data_as(pu), reps, seed,
                                         bp.ctypes.data_as(pd), elw.ctypes.data_as(pd), None) != 1:
            raise RuntimeError("the baseline library's rdamd_rell_bootstrap failed")
        return float(self.lib.rdamd_rell_last_resample_ms()), bp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--baseline-library")
    args = ap.parse_args()
    base = Baseline(args.baseline_library) if args.baseline_library else None
    for name in args.shape or ["c2", "c5"]:
        rows, patterns, reps = SHAPES[name]
        m = matrix(rows, patterns, 1)
        w = np.ones(patterns, dtype=np.uint32)
        n_draws = rd.au_scales(patterns)
        factor = sum(n_draws) / float(patterns)
        # (code objects loaded, every kernel of this shape's instantiation launched once)
        rd.au_test(m[:, :64], w[:64], 64, seed=1)
        rd.rell_bootstrap(m[:, :64], w[:64], 64, seed=1)
        if base:
            base.resample_ms(m[:, :64].copy(), w[:64].copy(), 64, 1)
        for run in range(args.runs):
            seed = run + 1
            t = time.time()
            counts = rd.rell_multiscale(m, w, n_draws, reps, seed)
            wall = time.time() - t
            multi = rd.rell_last_multiscale_ms()
            fit = rd.au_fit(counts, n_draws, patterns, reps)
            bp, _ = rd.rell_bootstrap(m, w, reps, seed=rd.rell_scale_seed(seed, 5))
            single = rd.rell_last_resample_ms()
            assert np.array_equal(np.rint(bp * reps), counts[5])      # (the scale of the alignment is the bootstrap)
            line = ("%-3s %4d x %6d B = %5d run %d: multiscale %9.3f ms, one bootstrap %8.3f ms, "
                    "x %.2f (sum M_k / N) = %9.3f ms, ratio %.4f"
                    % (name, rows, patterns, reps, run, multi, single, factor, factor * single, multi / (factor * single)))
            if base:
                prev, prev_bp = base.resample_ms(m, w, reps, rd.rell_scale_seed(seed, 5))
                assert np.array_equal(prev_bp, bp)
                line += ("; previous build's bootstrap %8.3f ms, x %.2f = %9.3f ms, ratio %.4f"
                         % (prev, factor, factor * prev, multi / (factor * prev)))
            line += ("; whole multiscale call %.2f s; rows fitted %d, kept at 0.05 %d"
                     % (wall, int((fit["used"] >= 2).sum()), int((fit["p_au"] >= 0.05).sum())))
            print(line, flush=True)


if __name__ == "__main__":
    main()
