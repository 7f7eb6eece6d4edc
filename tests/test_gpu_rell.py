"""rell_bootstrap (rdamd_rell_bootstrap, csrc/kernels_rell.hip: rell_resample_kernel without the
scales, then the support kernels) against a NumPy re-implementation of its definition in
include/root_digger_amd.h, the order rule of its sums, and the `rd_amd --rell / --site-lh` outputs.

Bounds (derived, not tuned), u = 2**-53, N columns:
  sums   relative 2 N u: N same-sign additions on the device, at most N roundings in the reference;
  bp     equal once replicates whose two largest REFERENCE sums are closer than 4 N u |largest| are
         left out (either side may order those differently); at most 1 % may be left out;
  elw    absolute 2 delta, delta = 2 N u max|sums| (a softmax moves by at most twice the largest
         shift of its arguments)."""
import os
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
import util
from test_rell_host import column_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD = os.path.join(ROOT, "root_digger_amd", "bin", "rd_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
MSA, TREE = os.path.join(util.DATA, "10.fasta"), os.path.join(util.DATA, "10.tree")
U = 2.0 ** -53
PARAMS3 = [.34, .42, .24, .74, .16, .88, .75, .54, .20, .06, .08, .41]


def reference(site_lnl, weights, n_replicates, seed):
    """-> sums[B][rows], winner[B], gap[B] (largest minus second largest sum), elw[rows]"""
    site_lnl = np.asarray(site_lnl, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.int64)
    n = int(weights.sum())
    col2pat = np.repeat(np.arange(len(weights)), weights)
    d = np.arange(n, dtype=np.uint64)
    counts = np.zeros((n_replicates, len(weights)), dtype=np.float64)
    for b in range(n_replicates):
        cols = column_np(np.uint64(seed), np.uint64(b), d, np.uint64(n))
        counts[b] = np.bincount(col2pat[cols.astype(np.int64)], minlength=len(weights))
    assert np.all(counts.sum(axis=1) == n)
    sums = counts @ site_lnl.T
    winner = np.argmax(sums, axis=1)            # the first of equals
    if sums.shape[1] > 1:
        top = np.sort(sums, axis=1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(n_replicates, np.inf)
    m = sums.max(axis=1, keepdims=True)
    e = np.exp(sums - m)
    elw = (e / e.sum(axis=1, keepdims=True)).mean(axis=0)
    return sums, winner, gap, elw


def random_walk_matrix(rows, patterns, seed):
    """negative site lnLs; a row is a random walk away from its neighbour, per-site steps of 0.02"""
    rng = np.random.default_rng(seed)
    m = np.empty((rows, patterns))
    m[0] = -rng.uniform(1.0, 12.0, patterns)
    for i in range(1, rows):
        m[i] = np.minimum(m[i - 1] + rng.normal(0.0, 0.02, patterns), -1e-3)
    return m


def ten_matrix():
    """the 17 x 991 site lnLs of 10.fasta / 10.tree, one rate category, every root at alpha 0.5"""
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=1, seed=3)
    m.initialize_partitions()
    m.set_subst_rates(PARAMS3)
    weights, _ = m.site_patterns()
    return m.site_lnls([tree.root_location(i) for i in range(17)]), weights


def check_against_numpy(matrix, weights, n_replicates, seed, what):
    n = int(np.sum(weights))
    bp, elw, sums = rd.rell_bootstrap(matrix, weights, n_replicates, seed, return_sums=True)
    want, winner, gap, want_elw = reference(matrix, weights, n_replicates, seed)
    err = float(np.max(np.abs(sums - want) / np.abs(want)))
    print("%s: N = %d, largest relative error of the sums %.3e (bound %.3e)" % (what, n, err, 2 * n * U))
    assert err <= 2 * n * U
    near = gap < 4 * n * U * np.abs(want.max(axis=1))
    print("%s: %d of %d replicates left out as near-ties" % (what, int(near.sum()), n_replicates))
    assert near.sum() <= 0.01 * n_replicates
    mine = np.argmax(sums, axis=1)
    counts = bp * n_replicates
    assert np.array_equal(counts, np.round(counts)) and counts.sum() == n_replicates
    assert np.array_equal(counts, np.bincount(mine, minlength=matrix.shape[0]))    # (ties: the lowest row)
    assert np.array_equal(mine[~near], winner[~near])
    delta = 2 * n * U * float(np.max(np.abs(want)))
    print("%s: largest |elw - reference| %.3e (bound %.3e), sum - 1 = %.3e"
          % (what, float(np.max(np.abs(elw - want_elw))), 2 * delta, float(elw.sum() - 1.0)))
    assert np.max(np.abs(elw - want_elw)) <= 2 * delta
    assert abs(elw.sum() - 1.0) <= 1e-12
    return bp, elw, sums


def test_rell_bootstrap_matches_numpy_on_the_ten_taxon_matrix():
    matrix, weights = ten_matrix()
    assert matrix.shape == (17, 991) and int(weights.sum()) == 1000
    check_against_numpy(matrix, weights, 2000, 12345, "10.fasta, 17 x 991")


def test_rell_bootstrap_matches_numpy_on_a_random_walk_matrix():
    rng = np.random.default_rng(4)
    matrix = random_walk_matrix(197, 3000, 1)
    weights = rng.integers(1, 4, 3000).astype(np.uint32)
    bp, elw, _ = check_against_numpy(matrix, weights, 2000, 7, "random walk, 197 x 3000")
    assert bp.max() < 1.0 and np.count_nonzero(bp) > 1      # (a case in which support is shared)


def test_order_rule_equal_rows_prefixes_and_repeats():
    rng = np.random.default_rng(5)
    matrix = random_walk_matrix(197, 3000, 2)
    weights = rng.integers(1, 4, 3000).astype(np.uint32)
    # a row that beats every other row at every site, three times over
    matrix[3] = matrix.max(axis=0)
    matrix[0] = matrix[3]
    matrix[40] = matrix[3]
    bp, elw, sums = rd.rell_bootstrap(matrix, weights, 100, 99, return_sums=True)
    assert np.array_equal(sums[:, 0], sums[:, 3]) and np.array_equal(sums[:, 40], sums[:, 3])
    # every replicate is a three-way tie: all of it goes to the lowest index
    assert bp[0] == 1.0 and bp[3] == 0.0 and bp[40] == 0.0 and bp.sum() == 1.0
    assert elw[0] == elw[3] == elw[40]
    # B = 10 is the first 10 replicates of B = 100; a repeated call returns the same bits
    _, _, first = rd.rell_bootstrap(matrix, weights, 10, 99, return_sums=True)
    assert np.array_equal(first, sums[:10])
    bp2, elw2, again = rd.rell_bootstrap(matrix, weights, 100, 99, return_sums=True)
    assert np.array_equal(again, sums) and np.array_equal(bp2, bp) and np.array_equal(elw2, elw)
    # another seed is another sample
    assert not np.array_equal(rd.rell_bootstrap(matrix, weights, 10, 100, return_sums=True)[2], first)


def test_order_rule_is_independent_of_the_number_of_rows():
    """one order for every launch shape: 8, 16, 32 or 64 lanes per replicate, one, two or four
    rows per lane, several row chunks"""
    rng = np.random.default_rng(6)
    matrix = random_walk_matrix(300, 1237, 3)      # (a column count that is no multiple of any batch)
    weights = rng.integers(1, 4, 1237).astype(np.uint32)
    want = None
    for rows in (1, 5, 9, 17, 33, 63, 64, 65, 128, 129, 257, 300):
        bp, elw, sums = rd.rell_bootstrap(matrix[:rows], weights, 37, 3, return_sums=True)
        assert sums.shape == (37, rows)
        if want is None:
            want = sums[:, 0].copy()
            ref = reference(matrix[:1], weights, 37, 3)[0]
            assert np.max(np.abs(sums - ref) / np.abs(ref)) <= 2 * int(weights.sum()) * U
        assert np.array_equal(sums[:, 0], want), rows
        assert np.array_equal(sums[:, rows - 1],
                              rd.rell_bootstrap(matrix[rows - 1:rows], weights, 37, 3, return_sums=True)[2][:, 0])
        if rows == 1:
            assert bp[0] == 1.0 and elw[0] == 1.0


def test_a_pattern_of_weight_zero_is_never_drawn():
    rng = np.random.default_rng(7)
    matrix = random_walk_matrix(20, 500, 4)
    weights = rng.integers(1, 4, 500).astype(np.uint32)
    poisoned, w0 = matrix.copy(), weights.copy()
    for p in (0, 77, 499):
        poisoned[:, p] = np.nan
        w0[p] = 0
    keep = w0 > 0
    bp, elw, sums = rd.rell_bootstrap(poisoned, w0, 50, 11, return_sums=True)
    assert np.all(np.isfinite(sums))
    bp1, elw1, sums1 = rd.rell_bootstrap(matrix[:, keep], weights[keep], 50, 11, return_sums=True)
    assert np.array_equal(sums, sums1) and np.array_equal(bp, bp1) and np.array_equal(elw, elw1)


def test_bad_arguments_fail_with_an_error_number():
    matrix = random_walk_matrix(4, 10, 5)
    ones = np.ones(10, dtype=np.uint32)
    huge = np.full(10, 1 << 31, dtype=np.uint32)           # N = 10 * 2^31 >= 2^32
    for args in ((matrix, huge, 10), (matrix[:0], ones, 10), (matrix, ones, 0),
                 (matrix, np.zeros(10, dtype=np.uint32), 10)):
        with pytest.raises(rd.RdamdError):
            rd.rell_bootstrap(*args)
        assert rd.lib.rdamd_errno() == 62
    bp, elw = rd.rell_bootstrap(matrix, ones, 10)          # (and the library is fine afterwards)
    assert bp.sum() == 1.0


def _run(args, **kw):
    return subprocess.run([RD] + args, capture_output=True, text=True, timeout=600, **kw)


def test_rd_amd_rell_and_site_lh(tmp_path):
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--silent", "--rate-cats", "4",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(REF):
        common += ["--lbfgsb", REF]
    prefix = str(tmp_path / "rell")
    out = _run(common + ["--prefix", prefix, "--rell", "1000", "--site-lh"])
    assert out.returncode == 0, out.stdout + out.stderr
    records = rd.Checkpoint(prefix).read_results()
    assert sorted(r[0] for r in records) == list(range(17))

    # .sitelh: the records' site lnLs, pattern by pattern through pattern_of, value for value
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=4, seed=5)
    m.initialize_partitions()
    weights, pattern_of = m.site_patterns()
    rls = [tree.root_location(r[0]).with_ratio(r[2]) for r in records]
    matrix = m.site_lnls(rls, [r[3] for r in records])
    lines = open(prefix + ".sitelh").read().splitlines()
    assert lines[0].split() == ["17", "1000"] and len(lines) == 18
    for line, rec, row in zip(lines[1:], records, matrix):
        toks = line.split()
        assert toks[0] == "root%d" % rec[0] and len(toks) == 1001
        assert np.array_equal(np.array([float(t) for t in toks[1:]]), row[pattern_of])

    # .support.tsv: root_id llh lwr bp elw, sorted by id; bp / elw are rell_bootstrap's of that matrix
    bp, elw = rd.rell_bootstrap(matrix, weights, 1000, seed=5)
    rows = [l.split("\t") for l in open(prefix + ".support.tsv").read().splitlines()]
    assert rows[0] == ["root_id", "llh", "lwr", "bp", "elw"] and len(rows) == 18
    assert [int(r[0]) for r in rows[1:]] == list(range(17))
    by_id = {rec[0]: k for k, rec in enumerate(records)}
    llh = np.array([rec[1] for rec in records])
    lwr = np.exp(llh - llh.max()) / np.exp(llh - llh.max()).sum()
    for r in rows[1:]:
        k = by_id[int(r[0])]
        assert float(r[1]) == records[k][1]
        assert abs(float(r[2]) - lwr[k]) <= 1e-12
        assert float(r[3]) == bp[k] and float(r[4]) == elw[k]
    assert abs(sum(float(r[3]) for r in rows[1:]) - 1.0) <= 1e-12

    nw = open(prefix + ".lwr.tree").read()
    assert nw.count("LWR=") > 0
    assert nw.count("BP=") == nw.count("LWR=") and nw.count("ELW=") == nw.count("LWR=")
    annotated = rd.Tree.from_newick(nw)
    assert annotated.tip_count() == 10
    # --rell-seed: another sample of the same matrix; default: --seed
    other = str(tmp_path / "seeded")
    out2 = _run(common + ["--prefix", other, "--rell", "1000", "--rell-seed", "6"])
    assert out2.returncode == 0, out2.stdout + out2.stderr
    assert not os.path.exists(other + ".sitelh")
    assert open(other + ".support.tsv").read() != open(prefix + ".support.tsv").read()

    # without the options nothing new is written and the tree carries no new keys
    plain = str(tmp_path / "plain")
    out3 = _run(common + ["--prefix", plain])
    assert out3.returncode == 0, out3.stdout + out3.stderr
    assert not os.path.exists(plain + ".sitelh") and not os.path.exists(plain + ".support.tsv")
    assert "BP=" not in open(plain + ".lwr.tree").read()
    assert open(plain + ".rooted.tree").read() == open(prefix + ".rooted.tree").read()


@pytest.mark.parametrize("extra,word", [
    (["--exhaustive", "--site-shards", "2"], "--rell"),
    (["--exhaustive", "--no-checkpoint"], "--rell"),
    ([], "--rell"),
])
def test_rd_amd_refuses_rell_where_it_cannot_work(tmp_path, extra, word):
    out = _run(["--msa", MSA, "--tree", TREE, "--silent", "--prefix", str(tmp_path / "no"), "--rell", "100"] + extra)
    assert out.returncode != 0
    assert word in out.stdout + out.stderr
    assert not os.path.exists(str(tmp_path / "no") + ".support.tsv")
