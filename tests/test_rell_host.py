"""Host side of the RELL bootstrap (no GPU): the counter-based draw function and the
column -> pattern relation the alignment compression keeps.

The draw function is re-implemented here twice from its definition in
include/root_digger_amd.h (Python integers, NumPy uint64), not from the library's code."""
import numpy as np
import pytest

import root_digger_amd as rd
import util

M64 = (1 << 64) - 1


def sm_int(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def column_int(seed, b, d, n):
    key = sm_int(seed ^ sm_int(b))
    u = sm_int((key + d) & M64)
    return ((u >> 32) * n) >> 32


def sm_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def column_np(seed, b, d, n):
    """all arguments uint64 arrays (n < 2^32)"""
    with np.errstate(over="ignore"):
        key = sm_np(seed ^ sm_np(b))
        u = sm_np(key + d)
        return ((u >> np.uint64(32)) * n) >> np.uint64(32)


def test_rell_column_reproduces_the_pinned_draws():
    for case in util.golden("rell_draws.json")["cases"]:
        for d, want in enumerate(case["columns"]):
            assert rd.rell_column(case["seed"], case["b"], d, case["N"]) == want
            assert column_int(case["seed"], case["b"], d, case["N"]) == want
            got = column_np(*(np.array([v], dtype=np.uint64) for v in (case["seed"], case["b"], d, case["N"])))
            assert int(got[0]) == want


def test_rell_column_matches_numpy_on_random_arguments():
    rng = np.random.default_rng(20260101)
    k = 100000
    seed = rng.integers(0, 1 << 64, k, dtype=np.uint64)
    b = rng.integers(0, 1 << 40, k, dtype=np.uint64)
    d = rng.integers(0, 1 << 32, k, dtype=np.uint64)
    # column counts of every magnitude, 1 .. 2^32 - 1
    n = (rng.integers(1, 1 << 32, k, dtype=np.uint64) >> rng.integers(0, 32, k, dtype=np.uint64)).clip(1, None)
    want = column_np(seed, b, d, n)
    assert np.all(want < n)
    got = np.array([rd.rell_column(int(s), int(bb), int(dd), int(nn)) for s, bb, dd, nn in zip(seed, b, d, n)],
                   dtype=np.uint64)
    assert np.array_equal(got, want)
    for i in range(0, k, 997):
        assert column_int(int(seed[i]), int(b[i]), int(d[i]), int(n[i])) == int(want[i])


def test_one_replicate_draws_a_bootstrap_sample():
    """N draws with replacement leave 1 - 1/e of the columns drawn at least once"""
    n = 5000
    for seed, b in ((1, 0), (12345, 3), (987654321, 9999)):
        cols = [rd.rell_column(seed, b, d, n) for d in range(n)]
        assert max(cols) < n
        share = len(set(cols)) / n
        print("N = %d seed %d replicate %d: share of distinct columns %.4f" % (n, seed, b, share))
        assert abs(share - (1.0 - np.exp(-1.0))) < 0.03


def _columns(seqs, names):
    return ["".join(seqs[k][s] for k in names) for s in range(len(seqs[names[0]]))]


def _canonical(cmap):
    """the character compress() keeps for every character: the first one with the same state set"""
    canon = {}
    for c in range(256):
        canon[chr(c)] = chr(c)
        if cmap[c]:
            for e in range(c):
                if cmap[e] == cmap[c]:
                    canon[chr(c)] = chr(e)
                    break
    return canon


PARTITION_LINES = ["DNA, first = 1-400", "DNA, second = 401-700, 901-1000", "DNA, third = 701-900"]


@pytest.mark.parametrize("name,reader,lines", [
    ("10.fasta", util.read_fasta, ()),
    ("101.phy", util.read_phylip, ()),
    ("10.fasta", util.read_fasta, PARTITION_LINES),
])
def test_pattern_of_expands_the_compressed_alignment(name, reader, lines):
    import os
    path = os.path.join(util.DATA, name)
    seqs = reader(path)
    names = list(seqs)
    compressed, weights, pattern_of = rd.msa_pattern_probe(path, lines)
    canon = _canonical(rd.MAP_NT)
    original = [s.translate({ord(k): v for k, v in canon.items()}) for s in _columns(seqs, names)]
    if lines:   # a partition's columns are its ranges back to back; partitions in file order
        order = []
        for line in lines:
            for lo, hi in rd.parse_partition_info(line)["parts"]:
                order.extend(range(lo - 1, hi))
        original = [original[c] for c in order]
    assert len(pattern_of) == len(original)
    assert len(weights) == len(compressed[0]) and len(compressed) == len(names)
    patterns = _columns(dict(zip(names, compressed)), names)
    assert [patterns[p] for p in pattern_of] == original
    assert np.array_equal(np.bincount(pattern_of, minlength=len(weights)), weights)
    assert int(weights.min()) >= 1
