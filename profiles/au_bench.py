"""The multiscale resampling of the AU test (rdamd_rell_multiscale: HIP events around its launches,
rell_last_multiscale_ms) against what its ten scales would cost as single-scale bootstraps:
(sum of M_k / N) x the resampling kernel of one rdamd_rell_bootstrap call (rell_last_resample_ms),
on the two shapes of profiles/r10_au.md.
usage: au_bench.py [--shape c2|c5|w8|w16|w32|w64|w128] [--runs 3] [--baseline-library PATH/librdamd.so]
(default: c2 and c5; the w shapes are the narrower launch shapes on 20 000 columns)
--baseline-library: another build of the library (the previous commit's), loaded next to this one;
its rdamd_rell_bootstrap and rdamd_rell_multiscale run on the same matrix in the same process,
interleaved with this build's, after one untimed full-size call of each; the two builds must return
equal counts and proportions.  One line per run, then per shape the medians of both builds, the
baseline's own spread (max - min) / median over its runs, and whether this build's medians lie
within it."""
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
    """rdamd_rell_bootstrap and rdamd_rell_multiscale of another build of the library"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        pd, pu, u = C.POINTER(C.c_double), C.POINTER(C.c_uint), C.c_uint
        self.lib.rdamd_rell_bootstrap.restype = C.c_int
        self.lib.rdamd_rell_bootstrap.argtypes = [pd, u, u, pu, u, C.c_uint64, pd, pd, pd]
        self.lib.rdamd_rell_last_resample_ms.restype = C.c_double
        self.lib.rdamd_rell_multiscale.restype = C.c_int
        self.lib.rdamd_rell_multiscale.argtypes = [pd, u, u, pu, u, C.POINTER(C.c_uint64), u, C.c_uint64, pu, pd]
        self.lib.rdamd_rell_last_multiscale_ms.restype = C.c_double
        self.lib.rdamd_version.restype = C.c_char_p

    def resample_ms(self, m, w, reps, seed):
        pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint)
        bp, elw = np.zeros(m.shape[0]), np.zeros(m.shape[0])
        if self.lib.rdamd_rell_bootstrap(m.ctypes.data_as(pd), m.shape[0], m.shape[1], w.ctypes.data_as(pu), reps, seed,
                                         bp.ctypes.data_as(pd), elw.ctypes.data_as(pd), None) != 1:
            raise RuntimeError("the baseline library's rdamd_rell_bootstrap failed")
        return float(self.lib.rdamd_rell_last_resample_ms()), bp

    def multiscale_ms(self, m, w, n_draws, reps, seed):
        pd, pu = C.POINTER(C.c_double), C.POINTER(C.c_uint)
        draws = np.asarray(n_draws, dtype=np.uint64)
        counts = np.zeros((len(draws), m.shape[0]), dtype=np.uint32)
        if self.lib.rdamd_rell_multiscale(m.ctypes.data_as(pd), m.shape[0], m.shape[1], w.ctypes.data_as(pu), len(draws),
                                          draws.ctypes.data_as(C.POINTER(C.c_uint64)), reps, seed,
                                          counts.ctypes.data_as(pu), None) != 1:
            raise RuntimeError("the baseline library's rdamd_rell_multiscale failed")
        return float(self.lib.rdamd_rell_last_multiscale_ms()), counts


def summary(name, what, ours, theirs):
    """this build's median against the baseline's, judged by the baseline's own spread"""
    med, ref = float(np.median(ours)), float(np.median(theirs))
    spread = (max(theirs) - min(theirs)) / ref
    off = med / ref - 1.0
    return ("%-3s %-10s median %9.3f ms, baseline %9.3f ms (%s), baseline spread %.2f %%, this build %+.2f %%: %s"
            % (name, what, med, ref, " ".join("%.3f" % t for t in theirs), 100 * spread, 100 * off,
               "within" if abs(off) <= spread else "OUTSIDE, faster" if off < 0 else "OUTSIDE, SLOWER"))


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
        times = {"multi": [], "prev_multi": [], "single": [], "prev_single": []}
        if base:
            base.resample_ms(m[:, :64].copy(), w[:64].copy(), 64, 1)
            # (the first large launches of a process run slow: one untimed full-size call of each)
            rd.rell_multiscale(m, w, n_draws, reps, 99)
            base.multiscale_ms(m, w, n_draws, reps, 99)
            rd.rell_bootstrap(m, w, reps, seed=99)
            base.resample_ms(m, w, reps, 99)
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
                prev_multi, prev_counts = base.multiscale_ms(m, w, n_draws, reps, seed)
                assert np.array_equal(prev_counts, counts)
                prev, prev_bp = base.resample_ms(m, w, reps, rd.rell_scale_seed(seed, 5))
                assert np.array_equal(prev_bp, bp)
                line += ("; previous build's multiscale %9.3f ms, bootstrap %8.3f ms, x %.2f = %9.3f ms, ratio %.4f"
                         % (prev_multi, prev, factor, factor * prev, multi / (factor * prev)))
                for key, t in (("multi", multi), ("prev_multi", prev_multi), ("single", single), ("prev_single", prev)):
                    times[key].append(t)
            line += ("; whole multiscale call %.2f s; rows fitted %d, kept at 0.05 %d"
                     % (wall, int((fit["used"] >= 2).sum()), int((fit["p_au"] >= 0.05).sum())))
            print(line, flush=True)
        if base:
            print(summary(name, "multiscale", times["multi"], times["prev_multi"]), flush=True)
            print(summary(name, "bootstrap", times["single"], times["prev_single"]), flush=True)


if __name__ == "__main__":
    main()
