#!/usr/bin/env python3
"""Every route to a root log-likelihood (csrc/kernels_root.hip), as text: float.hex of the single
call, the batched call, the one-launch root step with 1, 5 and 8 positions, and a digest of the
per-site values, for seeded shapes that reach every kernel instantiation and the grid cap.  Two
builds of the library agree bit for bit exactly when they print the same text:
    python3 profiles/root_bits.py > new.txt
    python3 profiles/with_ablation.py <other librdamd.so> profiles/root_bits.py > old.txt
The last line of the output is the SHA-256 of everything before it."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import root_digger_amd as rd          # noqa: E402
from root_digger_amd import synth     # noqa: E402
import util                           # noqa: E402

# (tips, sites, states, rate categories)
SHAPES = [(12, 777, 4, 1), (12, 1500, 4, 4), (12, 513, 4, 8), (12, 300, 4, 16), (12, 777, 4, 3),
          (12, 203, 20, 4),          # operand layout, ragged last tile
          (5, 66000, 4, 4),          # past the grid cap, one lane per (site, rate)
          (5, 262200, 4, 3)]         # past the grid cap, one lane per site
ALPHAS = [0.42, 1e-8, 0.0, 1.0 - 1e-8, 1.0, 0.125, 0.125 + 1e-8, 0.875]


def main():
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    for n, S, K, R in SHAPES:
        tag = "n%d S%d K%d R%d" % (n, S, K, R)
        w = synth.workload(n, S, K, R, 1300 + S + R)
        tree = rd.Tree.from_newick(w["newick"])
        d = tree.generate_directional_operations()
        b = tree.branch_count()
        g = rd.Partition(n, max(d["clv_buffers"], b), K, S, 1, max(d["prob_matrices"], b), R,
                         max(d["scale_buffers"], b))
        weights = np.random.default_rng(S).integers(1, 4, size=S).astype(np.uint32)
        util.load_tips(g, tree, w["seqs"], rd.MAP_NT if K == 4 else util.make_map(w["alphabet"]), weights)
        g.set_subst_params(0, w["subst"])
        g.set_frequencies(0, g.empirical_frequencies())
        g.set_category_rates(w["rates"])
        g.update_prob_matrices(d["matrix_indices"], d["branch_lengths"])
        g.update_clvs(d["ops"])
        for rid in range(tree.root_count()):
            one = g.compute_root_loglikelihood(int(d["root_clv"][rid]), int(d["root_scaler"][rid]))
            emit("%s single %d %s" % (tag, rid, float(one).hex()))
        for rid, v in enumerate(g.compute_root_loglikelihoods(d["root_clv"], d["root_scaler"])):
            emit("%s batch %d %s" % (tag, rid, float(v).hex()))
        v, persite = g.compute_root_loglikelihood(int(d["root_clv"][0]), int(d["root_scaler"][0]), persite=True)
        text = "\n".join(float(x).hex() for x in persite)
        emit("%s persite %s %d values sha256 %s" % (tag, float(v).hex(), persite.size,
                                                   hashlib.sha256(text.encode()).hexdigest()))
        rl = tree.root_location(2).with_ratio(0.42)
        util.compute_lh(g, tree, rl)
        op, _, _ = tree.generate_derivative_operations(rl)
        for npos in (1, 5, 8):
            got = g.root_loglikelihood_fused(op, [rl.saved_brlen * a for a in ALPHAS[:npos]],
                                             [rl.saved_brlen * (1 - a) for a in ALPHAS[:npos]])
            emit("%s fused %d %s" % (tag, npos, " ".join(float(x).hex() for x in got)))
        g.destroy()
    print("sha256 %s" % hashlib.sha256("\n".join(lines).encode()).hexdigest())


if __name__ == "__main__":
    main()
