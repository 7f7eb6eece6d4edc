#!/usr/bin/env python3
"""(Lives under tests/: it borrows the reference's L-BFGS-B build, oracle/_ref, as the caller's
optimiser -- nothing outside tests/ may touch oracle/.)
The lock-stepped search in rounds on a site-sharded PARTITIONED model: a synthetic 100-taxon x
50 000-column alignment (synth.workload, BASELINE c2's shape) as 1, 4 and 16 equal UNREST+G4
partitions, G = 2 site blocks.  The two ranks of the site group are two THREADS of this process on
ONE device (device 0), summed by a host reducer in rank order (rd_amd --site-reduce host's sum):
their launches share the device, so the timings are not those of two GPUs.  Reports, per
partition count: objective launches per round (one per partition with jobs), round wall time,
collectives per candidate -- what a fused multi-partition launch would have to beat.

  partitioned_shards_profile.py <out.json> [candidates] [in_flight]"""
import ctypes as C
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import root_digger_amd as rd  # noqa: E402
from root_digger_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
TAXA, SITES, G = 100, 50000, 2


class Group:
    def __init__(self, n):
        self.n, self.vals, self.barrier = n, [None] * n, threading.Barrier(n, timeout=600)

    def reducer(self, rank):
        def fn(values, n):
            self.vals[rank] = np.array(values[:n])
            self.barrier.wait()
            acc = self.vals[0].copy()
            for r in range(1, self.n):
                acc = acc + self.vals[r]
            self.barrier.wait()
            values[:n] = acc
        return fn


def one(tmp, msa, tree_file, n_parts, candidates, in_flight):
    width = SITES // n_parts
    pf = os.path.join(tmp, "parts_%d.txt" % n_parts)
    with open(pf, "w") as f:
        for p in range(n_parts):
            f.write("UNREST+G4, p%d = %d-%d\n" % (p, p * width + 1, SITES if p == n_parts - 1 else (p + 1) * width))
    group, out, errors = Group(G), [None] * G, []
    rd.set_device(0)

    def rank(r):
        try:
            rd.set_device(0)
            tree = rd.Tree.from_file(tree_file)
            m = rd.Model.from_partition_file_block(tree, msa, pf, r, G, seed=3)
            m.set_lnl_reducer(group.reducer(r))
            m.initialize_partitions()
            m.set_lbfgsb(C.CDLL(REF).setulb)
            m.compute_lh(tree.root_location(0))
            m.assign_by_rank(0, max(1, tree.root_count() // candidates))
            t0 = time.perf_counter()
            res = m.exhaustive_search(1e-2, 1e-2, 1e-2, 1e13, lockstep=in_flight)
            wall = time.perf_counter() - t0
            out[r] = {"wall_s": wall, "candidates": len(res["root_id"]), "rounds": m.round_stats(),
                      "launches": m.lockstep_stats(), "per_partition": m.round_partition_stats(),
                      "patterns": m.patterns, "digest": hash(tuple(res["llh"]))}
            m.destroy()
        except BaseException as e:
            errors.append(repr(e))
            group.barrier.abort()
    ts = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errors:
        raise RuntimeError(errors)
    assert out[0]["digest"] == out[1]["digest"]
    r0 = out[0]
    st, ls = r0["rounds"], r0["launches"]
    return {
        "partitions": n_parts,
        "columns_per_partition": width,
        "patterns_rank0": r0["patterns"],
        "candidates": r0["candidates"],
        "wall_s": round(max(o["wall_s"] for o in out), 3),
        "rounds": st["rounds"], "collectives": st["collectives"], "redos": st["redos"],
        "objective_launches": ls["objective_launches"], "objective_jobs": ls["objective_jobs"],
        "root_launches": ls["root_launches"],
        "objective_launches_per_collective": round(ls["objective_launches"] / max(1, st["collectives"] - st["redos"]), 3),
        "jobs_per_objective_launch": round(ls["objective_jobs"] / max(1, ls["objective_launches"]), 2),
        "round_wall_ms": round(1e3 * max(o["wall_s"] for o in out) / max(1, st["collectives"]), 3),
        "collectives_per_candidate": round(st["collectives"] / max(1, r0["candidates"]), 1),
        "round_host_seconds": st["seconds"],
        "per_partition_launches": [p["launches"] for p in r0["per_partition"]],
    }


def main():
    out_path = sys.argv[1]
    candidates = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    in_flight = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    w = synth.workload(TAXA, SITES, 4, 4, 0xD166E5 + 1)
    with tempfile.TemporaryDirectory() as tmp:
        msa, tree_file = os.path.join(tmp, "aln.fasta"), os.path.join(tmp, "tree.nwk")
        with open(msa, "w") as f:
            for k, v in w["seqs"].items():
                f.write(">%s\n%s\n" % (k, v))
        with open(tree_file, "w") as f:
            f.write(w["newick"])
        rows = []
        for n_parts in (1, 4, 16):
            rows.append(one(tmp, msa, tree_file, n_parts, candidates, in_flight))
            print(json.dumps(rows[-1]), flush=True)
    doc = {
        "what": "lock-stepped exhaustive search in rounds, site-sharded partitioned model",
        "workload": "synth.workload(100, 50000, 4, 4, 0xD166E5 + 1): 100 taxa x 50 000 columns, equal UNREST+G4 partitions",
        "layout": "G = 2 site blocks; both ranks are threads of ONE process on ONE MI355X (device 0), host reducer "
                  "(rank-order sum through Python): launches of the two ranks share the device, timings are not "
                  "those of two GPUs",
        "search": {"candidates": candidates, "in_flight": in_flight, "worker_groups": 1,
                   "atol_pgtol_brtol_factor": [1e-2, 1e-2, 1e-2, 1e13]},
        "rows": rows,
    }
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
