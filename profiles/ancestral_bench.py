"""The pre-order pass of the ancestral states (rdamd_marginal_ancestral: HIP events around its one
launch, ancestral_last_ms) against one materialising traversal (rdamd_update_clvs, profile family 0)
of the same partition, timed in the same process with the runs interleaved, on the two inputs of
profiles/r11_ancestral.md: c2's shape (100 taxa x 50 000 columns, four gamma categories) and 125.phy.
usage: ancestral_bench.py [--input c2|d125] [--runs 7] [--baseline-library PATH/librdamd.so]
--baseline-library: another build of the library (the previous commit's), loaded next to this one;
its rdamd_update_clvs runs on a partition of its own with the same data and is the yardstick, and this
build's own traversal is timed next to it (it must not have moved).  One line per input."""
import argparse
import ctypes as C
import lzma
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import root_digger_amd as rd  # noqa: E402
from root_digger_amd import synth  # noqa: E402
import util  # noqa: E402

SUBST = [.34, .42, .24, .74, .16, .88, .75, .54, .20, .06, .08, .41]
FREQS = [.21, .29, .27, .23]


def inputs(name):
    if name == "c2":
        w = synth.workload(100, 50000, 4, 4, 2, simulate_seqs=False)
        return rd.Tree.from_newick(w["newick"]), w["seqs"]
    data = os.path.join(ROOT, "tests", "golden", "data")
    text = lzma.open(os.path.join(data, "125.phy.xz"), "rt").read()
    with tempfile.NamedTemporaryFile("w", suffix=".phy") as tmp:
        tmp.write(text)
        tmp.flush()
        seqs, _ = util.compress(util.read_phylip(tmp.name))
    return rd.Tree.from_file(os.path.join(data, "125.tree")), seqs


class BaselinePartition:
    """the same partition in another build of the library: create, load, traverse, time"""

    def __init__(self, path, tree, seqs, R):
        self.lib = lib = C.CDLL(path)
        lib.rdamd_partition_create.restype = C.c_void_p
        b, S = tree.branch_count(), len(next(iter(seqs.values())))
        self.h = C.c_void_p(lib.rdamd_partition_create(tree.tip_count(), b, 4, S, 1, b, R, b, rd.ATTRIB_NONREV))
        if not self.h:
            raise RuntimeError("the baseline library's rdamd_partition_create failed")
        for label, seq in seqs.items():
            lib.rdamd_set_tip_states(self.h, C.c_uint(tree.tip_index(label)), rd.MAP_NT, seq.encode())
        arr = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        lib.rdamd_set_subst_params(self.h, 0, arr(SUBST))
        lib.rdamd_set_frequencies(self.h, 0, arr(FREQS))
        lib.rdamd_set_category_rates(self.h, arr(rd.compute_gamma_cats(1.0, R)))
        lib.rdamd_profile_enable(self.h, 1)

    def traversal_ms(self, ops, pmi, brl):
        lib, R = self.lib, 4
        mi = np.ascontiguousarray(pmi, dtype=np.uint32)
        bl = np.ascontiguousarray(brl, dtype=np.float64)
        pi = np.zeros(R, dtype=np.uint32)
        u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))  # noqa: E731
        lib.rdamd_update_prob_matrices(self.h, u(pi), u(mi), bl.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint(mi.size))
        lib.rdamd_update_clvs(self.h, ops, C.c_uint(len(ops)))
        ms, n = (C.c_double * 8)(), (C.c_uint * 8)()
        lib.rdamd_profile_read(self.h, ms, n)
        return ms[0]


def traversal_ms(p, ops):
    p.update_clvs(ops)
    return p.profile_read()["clv"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=["c2", "d125"], action="append")
    ap.add_argument("--runs", type=int, default=7)
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
        base = BaselinePartition(args.baseline_library, tree, seqs, R) if args.baseline_library else None
        p.update_prob_matrices(pmi, brl)
        p.profile_enable(True)
        own, parent, outer = [], [], []
        for run in range(args.runs + 1):      # (the first run warms up)
            t_own = traversal_ms(p, ops)
            t_parent = base.traversal_ms(ops, pmi, brl) if base else float("nan")
            p.marginal_ancestral(ops)
            if run:
                own.append(t_own)
                parent.append(t_parent)
                outer.append(rd.ancestral_last_ms())
        slots = rd.ancestral_workspace_slots(ops, tree.tip_count())
        yard = np.median(parent) if base else np.median(own)
        print("%s: %d taxa x %d patterns, R %d: pre-order pass %.3f ms (min %.3f), traversal %.3f ms (parent build %.3f ms), "
              "ratio %.2f; workspace %d slots = %.1f MB of %d inner CLVs = %.1f MB; posteriors %.1f MB" % (
                  name, tree.tip_count(), S, R, np.median(outer), np.min(outer), np.median(own), np.median(parent),
                  np.median(outer) / yard, slots, slots * S * R * 32 / 1e6, len(ops), len(ops) * S * R * 32 / 1e6,
                  len(ops) * S * 32 / 1e6), flush=True)


if __name__ == "__main__":
    main()
