"""Site-sharded PARTITIONED runs: a partition file (src/main.cpp:512-555, each partition with its
own parameters, src/model.cpp:1935-1960) under --site-shards G.  Every rank of a site group holds
block b of EVERY partition's own columns (rdamd_model_create_partitioned_block; the split is
dist.partition_site_blocks), and a lock-stepped round launches the fused evaluator once per
partition that has jobs, each on its own stream, with ONE collective for all of them.

* in one process, G block models on threads with a host reducer that sums in rank order: per-partition
  lnLs, compute_lh, compute_lh_root, the root sweeps and the empirical frequencies equal the unsharded
  partitioned model, and every block holds the same bits;
* the search in rounds == the sequential sharded search (rd_amd, 2 / 4 ranks of one device, host
  reducer), to the bit; == the one-rank search to optimiser tolerance;
* a round in which only one partition's batch needs the evaluator's second pass repeats its
  collective and re-launches that partition alone;
* the RCCL communicator (one rank) as the device reducer behind a partitioned block model's rounds;
* refusals (a partition shorter than G) and resuming from the checkpoint."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import root_digger_amd as rd
from root_digger_amd import dist as rdist
from root_digger_amd import synth
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD = os.path.join(ROOT, "root_digger_amd", "bin", "rd_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
MSA, TREE = os.path.join(util.DATA, "10.fasta"), os.path.join(util.DATA, "10.tree")
PHY, PHY_TREE = os.path.join(util.DATA, "101.phy"), os.path.join(util.DATA, "101.tree")
# the two partition files of test_gpu_optimizer.py's partitioned lock-step test, and three uneven
# partitions (one of two ranges)
FILES = {
    "equal": "UNREST+G4, a = 1-400\nUNREST+G4, b = 401-1000\n",
    "mixed": "UNREST+G4, a = 1-300\nUNREST, b = 301-1000\n",
    "three": "UNREST+G4, a = 1-137\nUNREST+G4, b = 138-611, 900-1000\nUNREST, c = 612-899\n",
}
FILES_101 = {
    "equal": "UNREST+G4, a = 1-929\nUNREST+G4, b = 930-1858\n",
    "mixed": "UNREST+G4, a = 1-300\nUNREST, b = 301-1858\n",
    "three": "UNREST+G4, a = 1-301\nUNREST+G4, b = 302-1400, 1700-1858\nUNREST, c = 1401-1699\n",
}
LOOSE = (1e-2, 1e-2, 1e-2, 1e13)      # atol, pgtol, brtol, factor (bit-for-bit comparisons)


def _need_ref():
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/liblbfgsb_ref.so not built")


def _ranges(text):
    out = []
    for line in text.strip().splitlines():
        spec = line.split("=", 1)[1]
        out.append([tuple(int(v) for v in r.split("-")) for r in spec.split(",")])
    return out


class _Group:
    """a site group of G ranks as threads of this process: each rank's reducer hands its vector in
    and gets the sum in RANK ORDER back, ((v0 + v1) + v2) + ... -- rd_amd's host reducer's sum"""

    def __init__(self, G):
        self.G, self.vals = G, [None] * G
        self.barrier = threading.Barrier(G, timeout=300)

    def reducer(self, rank):
        def fn(values, n):
            self.vals[rank] = np.array(values[:n])
            self.barrier.wait()
            acc = self.vals[0].copy()
            for r in range(1, self.G):
                acc = acc + self.vals[r]
            self.barrier.wait()
            values[:n] = acc
        return fn

    def run(self, body):
        """body(rank) on G threads; -> [result of rank r]"""
        out, errors = [None] * self.G, []

        def go(r):
            try:
                out[r] = body(r)
            except BaseException as e:          # (the others must not wait for this rank)
                errors.append((r, e))
                self.barrier.abort()
        ts = [threading.Thread(target=go, args=(r,)) for r in range(self.G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=900)
        assert not errors, errors
        return out


def _measure(m, tree, roots):
    m.initialize_partitions()                      # (group) empirical frequencies + seeded rates
    out = {"freqs": [list(m.partition_frequencies(p)) for p in range(m.partition_count())]}
    rls = [tree.root_location(i).with_ratio(0.3) for i in roots]
    out["part_lh"] = [list(m.partition_lnls(rl)) for rl in rls]
    out["lh"] = [m.compute_lh(rl) for rl in rls]
    out["lh_root"] = [m.compute_lh_root(rls[-1].with_ratio(a)) for a in (0.1, 0.9)]
    out["sweep"] = list(m.compute_all_root_lh())
    out["sweep_batched"] = list(m.compute_all_root_lh_batched())
    return out


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) < tol


@pytest.mark.parametrize("data", ["10", "101"])
@pytest.mark.parametrize("name", sorted(FILES))
@pytest.mark.parametrize("G", [2, 4])
def test_blocks_reproduce_the_whole_partitioned_model(tmp_path, data, name, G):
    msa, tree_path, text = (MSA, TREE, FILES[name]) if data == "10" else (PHY, PHY_TREE, FILES_101[name])
    pf = tmp_path / "parts.txt"
    pf.write_text(text)
    tree = rd.Tree.from_file(tree_path)
    roots = (0, 5, 16)
    whole = rd.Model.from_partition_file(tree, msa, str(pf), seed=3)
    one = _measure(whole, tree, roots)
    whole.destroy()
    group = _Group(G)
    want = [rdist.partition_site_blocks(_ranges(text), b, G) for b in range(G)]

    def rank(r):
        m = rd.Model.from_partition_file_block(rd.Tree.from_file(tree_path), msa, str(pf), r, G, seed=3)
        assert m.partition_count() == len(want[r])
        # (the block's columns are the helper's ranges: their count per partition)
        cols = [sum(hi - lo + 1 for lo, hi in rr) for rr in _ranges(text)]
        assert m.columns == cols
        assert all(0 < pt <= sum(hi - lo + 1 for lo, hi in w) for pt, w in zip(m.patterns, want[r]))
        m.set_lnl_reducer(group.reducer(r))
        out = _measure(m, tree, roots)
        m.destroy()
        return out
    got = group.run(rank)
    for key in ("freqs", "lh", "lh_root", "sweep", "sweep_batched"):
        for r in range(1, G):
            assert got[r][key] == got[0][key], key            # every rank of the group: the same bits
        assert _close(got[0][key], one[key], 1e-12), key      # = the unsharded partitioned model
    # a partition's lnL is the sum of its blocks' (each block's own, unsummed)
    per_part = np.sum([np.array(got[r]["part_lh"]) for r in range(G)], axis=0)
    assert _close(per_part, one["part_lh"], 1e-12)
    assert _close(np.sum(one["part_lh"], axis=1), one["lh"], 1e-12)


def _run_ranks(args, world, timeout=900):
    s = __import__("socket").socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    procs = [subprocess.Popen(args, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=timeout) for p in procs]
    return [p.returncode for p in procs], outs


def _stats(outs, world):
    stats = {}
    for _, err in outs:
        for line in err.splitlines():
            mt = re.match(r"\[rank (\d+)\] stats: (.*)", line)
            if mt:
                stats[int(mt.group(1))] = dict(kv.split("=") for kv in mt.group(2).split())
    assert sorted(stats) == list(range(world)), outs
    return stats


def _common(pf, shards, early_stop=False):
    return ["--msa", MSA, "--tree", TREE, "--partition", str(pf), "--exhaustive", "--atol", "0.5", "--brtol", "0.1",
            "--bfgstol", "0.5", "--factor", "1e15", "--seed", "5", "--lbfgsb", REF, "--device", "0",
            "--site-shards", str(shards), "--site-reduce", "host", "--stats"] + (["--early-stop"] if early_stop else [])


# (at most four ranks: with the test process, more would hold one shared device from more processes
# than it admits)
@pytest.mark.parametrize("world,shards,early_stop,name", [(2, 2, False, "equal"), (2, 2, False, "mixed"),
                                                          (2, 2, False, "three"), (4, 2, False, "mixed"),
                                                          (4, 4, False, "three"), (2, 2, True, "mixed")])
def test_partitioned_lock_step_equals_the_sequential_sharded_search(tmp_path, world, shards, early_stop, name):
    """the same sums in the same order (a partition's objective: the group sum of its blocks; a root
    lnL: partitions in file order, then the group): the records of --lockstep 8 are those of
    --lockstep 0 bit for bit, every rank of a group agrees, one collective per round"""
    _need_ref()
    pf = tmp_path / "parts.txt"
    pf.write_text(FILES[name])
    seq, lock = str(tmp_path / "seq"), str(tmp_path / "lock")
    rc, outs = _run_ranks([RD] + _common(pf, shards, early_stop) + ["--prefix", seq, "--lockstep", "0"], world)
    assert rc == [0] * world, outs
    st_seq = _stats(outs, world)
    rc, outs = _run_ranks([RD] + _common(pf, shards, early_stop) + ["--prefix", lock, "--lockstep", "8"], world)
    assert rc == [0] * world, outs
    st_lock = _stats(outs, world)
    n_parts = len(FILES[name].strip().splitlines())
    # one line per partition and rank: its block's patterns of the partition's columns
    lines = re.findall(r"\[rank (\d+)\] candidate group \d+/\d+, partition (\d+), site block (\d+)/(\d+): (\d+) patterns "
                       r"of (\d+) columns", "".join(o for o, _ in outs))
    assert len(lines) == world * n_parts
    ra = sorted(rd.Checkpoint(seq).read_results())
    rb = sorted(rd.Checkpoint(lock).read_results())
    assert [r[0] for r in ra] == list(range(17))
    assert ra == rb                                          # ids, lnL, alpha, parameters: same bits
    for g in range(world // shards):
        members = range(g * shards, (g + 1) * shards)
        assert len({st_lock[r]["results_digest"] for r in members}) == 1
        assert len({st_lock[r]["collectives"] for r in members}) == 1
        assert st_lock[g * shards]["results_digest"] == st_seq[g * shards]["results_digest"]
    st = st_lock[0]
    # ONE collective per round (plus its repeats), whatever the number of partitions launched in it
    assert 0 < int(st["collectives"]) <= int(st["rounds"]) + int(st["redos"])
    assert int(st_seq[0]["own_collectives"]) > 3 * int(st["collectives"])
    assert open(seq + ".rooted.tree").read() == open(lock + ".rooted.tree").read()


def _thread_search(text, tmp_path, G, lockstep, tight):
    pf = tmp_path / ("parts_%d.txt" % G)
    pf.write_text(text)
    pgtol, factor, atol, brtol = (1e-7, 1e4, 1e-7, 1e-9) if tight else (1e-2, 1e13, 1e-2, 1e-2)
    group = _Group(G) if G > 1 else None

    def rank(r):
        tree = rd.Tree.from_file(TREE)
        m = (rd.Model.from_partition_file_block(tree, MSA, str(pf), r, G, seed=3) if G > 1
             else rd.Model.from_partition_file(tree, MSA, str(pf), seed=3))
        if group:
            m.set_lnl_reducer(group.reducer(r))
        m.initialize_partitions()
        m.set_lbfgsb(C.CDLL(REF).setulb)
        m.compute_lh(tree.root_location(0))
        m.assign_by_rank(0, 3)                               # the first six candidates
        res = m.exhaustive_search(atol, pgtol, brtol, factor, lockstep=lockstep)
        st = m.round_stats()
        m.destroy()
        return (list(res["root_id"]), list(res["llh"]), list(res["alpha"])), st
    if group:
        return group.run(rank)
    return [rank(0)]


def test_sharded_search_in_rounds_is_the_one_rank_search_to_optimiser_tolerance(tmp_path):
    _need_ref()
    got = _thread_search(FILES["mixed"], tmp_path, 2, 6, tight=True)
    one = _thread_search(FILES["mixed"], tmp_path, 1, 0, tight=True)[0][0]
    assert got[0][0] == got[1][0]                            # the ranks agree bit for bit
    assert got[0][1]["rounds"] > 0 and got[0][1]["collectives"] > 0
    ids, llh, alpha = got[0][0]
    assert ids == one[0] == list(range(6))
    assert _close(llh, one[1], 2e-6)
    assert np.max(np.abs(np.array(alpha) - np.array(one[2]))) < 2e-2


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for k, v in seqs.items():
            f.write(">%s\n%s\n" % (k, v))


def test_only_the_partition_whose_batch_needs_its_second_pass_launches_again(tmp_path, monkeypatch):
    """300 tips on branches of 1e-7 with the speculative evaluator forced on: under the 120 columns of
    UNRELATED sequences (partition a) a site's likelihood falls far below the FP64 range and every
    job is flagged for the second pass; the 120 CONSERVED columns beside them (partition b) never are.
    A round repeats its collective, re-launches partition a alone, and the records are the
    sequential search's bit for bit -- without a reducer and with the RCCL communicator (one rank)."""
    _need_ref()
    monkeypatch.setenv("RDAMD_RESCALE_SPECULATION", "1")
    w = synth.workload(300, 120, 4, 4, 631, simulate_seqs=False)
    nw = re.sub(r":[0-9.eE+-]+", ":1e-7", w["newick"])
    rng = np.random.default_rng(5)
    conserved = "".join(rng.choice(list("ACGT"), 120))
    seqs = {k: v + conserved for k, v in w["seqs"].items()}
    msa, pf = str(tmp_path / "aln.fasta"), str(tmp_path / "parts.txt")
    _write_fasta(msa, seqs)
    with open(pf, "w") as f:
        f.write("UNREST+G4, a = 1-120\nUNREST+G4, b = 121-240\n")
    tree_file = str(tmp_path / "t.nwk")
    with open(tree_file, "w") as f:
        f.write(nw)

    def model():
        tree = rd.Tree.from_file(tree_file)
        m = rd.Model.from_partition_file_block(tree, msa, pf, 0, 1, seed=3)
        m.initialize_partitions()
        m.set_lbfgsb(C.CDLL(REF).setulb)
        m.compute_lh(tree.root_location(0))
        m.assign_by_rank(0, 100)                             # the first six candidates
        return m

    def search(m, lockstep):
        r = m.exhaustive_search(*LOOSE, lockstep=lockstep)
        return list(r["root_id"]), list(r["llh"]), list(r["alpha"])

    seq = model()
    want = search(seq, 0)
    assert np.all(np.isfinite(want[1])) and len(want[0]) == 6
    assert seq.partition_second_passes(0) > 0 and seq.partition_second_passes(1) == 0
    seq.destroy()
    comm = rd.Comm(rd.Comm.unique_id(), 0, 1)
    for with_reducer in (False, True):
        m = model()
        if with_reducer:
            m.set_lnl_reducer(comm.reducer, on_device=True, user=comm.handle)
        m.set_lockstep_rounds(1)
        assert search(m, 6) == want, with_reducer
        st, parts = m.round_stats(), m.round_partition_stats()
        assert st["redos"] > 0 and st["collectives"] > st["redos"], st
        assert parts[0]["redo_launches"] == st["redos"] and parts[1]["redo_launches"] == 0, parts
        assert parts[0]["launches"] > 0 and parts[1]["launches"] > 0, parts
        assert m.partition_second_passes(1) == 0
        m.destroy()
    comm.destroy()


@pytest.mark.parametrize("name", ["mixed", "three"])
def test_rounds_with_the_rccl_communicator_on_a_partitioned_block_model(tmp_path, name):
    """block 0 of 1 with rdamd_comm_reducer on a one-rank group: the batches of all partitions go to
    their slices of the round's device vector, the collective on partition 0's stream waits for the
    other partitions' streams through events.  A one-rank sum changes nothing: the records are the
    same model's without a reducer, bit for bit"""
    _need_ref()
    pf = tmp_path / "parts.txt"
    pf.write_text(FILES[name])

    def run(reducer):
        tree = rd.Tree.from_file(TREE)
        m = rd.Model.from_partition_file_block(tree, MSA, str(pf), 0, 1, seed=3)
        if reducer:
            m.set_lnl_reducer(reducer.reducer, on_device=True, user=reducer.handle)
        m.initialize_partitions()
        m.set_lbfgsb(C.CDLL(REF).setulb)
        m.compute_lh(tree.root_location(0))
        m.set_lockstep_rounds(1)
        m.assign_by_rank(0, 1)
        r = m.exhaustive_search(*LOOSE, lockstep=17)
        out = (list(r["root_id"]), list(r["llh"]), list(r["alpha"]))
        st, parts = m.round_stats(), m.round_partition_stats()
        m.destroy()
        return out, st, parts
    plain, _, _ = run(None)
    comm = rd.Comm(rd.Comm.unique_id(), 0, 1)
    got, st, parts = run(comm)
    comm.destroy()
    assert got == plain
    assert plain[0] == list(range(17))
    assert 0 < st["collectives"] <= st["rounds"] + st["redos"]
    assert all(p["launches"] > 0 for p in parts), parts


def test_a_partition_shorter_than_the_site_blocks_is_refused_by_name(tmp_path):
    pf = tmp_path / "parts.txt"
    pf.write_text("UNREST+G4, long = 1-999\nUNREST, tiny = 1000-1000\n")
    rc, outs = _run_ranks([RD, "--msa", MSA, "--tree", TREE, "--partition", str(pf), "--exhaustive", "--device", "0",
                           "--site-shards", "2", "--site-reduce", "host", "--prefix", str(tmp_path / "x")], 2, timeout=300)
    assert all(c != 0 for c in rc), outs
    text = "".join(o + e for o, e in outs)
    assert "Partition 'tiny' has 1 columns, fewer than the 2 site blocks" in text, text[-2000:]
    assert "Starting exhaustive search" not in text


def test_a_sharded_partitioned_run_resumes_from_its_checkpoint(tmp_path):
    """the options saved in the checkpoint carry the partition file: a second invocation with the same
    prefix and --site-shards (and no --partition) builds every rank's BLOCKS of the partitioned model
    again, finds every candidate done and writes the same tree"""
    _need_ref()
    pf = tmp_path / "parts.txt"
    pf.write_text(FILES["three"])
    prefix = str(tmp_path / "run")
    rc, outs = _run_ranks([RD] + _common(pf, 2) + ["--prefix", prefix, "--lockstep", "8"], 2)
    assert rc == [0, 0], outs
    tree = open(prefix + ".rooted.tree").read()
    first = sorted(rd.Checkpoint(prefix).read_results())
    os.remove(prefix + ".rooted.tree")
    args = [RD, "--msa", MSA, "--tree", TREE, "--lbfgsb", REF, "--device", "0", "--site-shards", "2",
            "--site-reduce", "host", "--prefix", prefix, "--lockstep", "8"]
    rc, outs = _run_ranks(args, 2)
    assert rc == [0, 0], outs
    text = "".join(o for o, _ in outs)
    assert len(re.findall(r"partition \d+, site block \d+/2", text)) == 2 * 3, text[-2000:]
    assert open(prefix + ".rooted.tree").read() == tree
    assert sorted(rd.Checkpoint(prefix).read_results()) == first
