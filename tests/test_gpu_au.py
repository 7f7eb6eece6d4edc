"""rell_multiscale / au_test (rdamd_rell_multiscale, csrc/kernels_rell.hip: the bootstrap's
rell_resample_kernel with a scale per wave) against the NumPy multiscale bootstrap of
tests/test_au_host.py, the order rule of the sums at every scale and launch shape, the bootstrap
itself at every launch shape, and `rd_amd --rell B --au`.

Bounds (derived, not tuned), u = 2**-53, scale k with M_k draws, S = the reference sums of the scale:
  sums    within 2 M_k u max|S|: M_k same-sign additions on the device, at most M_k roundings in
          the reference (the bound of test_gpu_rell.py with M_k in place of N);
  counts  a replicate is a near tie when its two largest reference sums differ by at most
          4 M_k u max|S| (either side may order those differently); a row's count may differ from
          the reference's by at most the near-tie replicates in which the row is within that width
          of the largest sum.  Condition on the inputs: at most 1 % of the replicates are near ties.
On walk40 and walk197 the reference alone shows NO near tie (smallest relative gaps 2.6e-8 and
5.2e-10 against widths of 1.5e-12 and 3.8e-12), so there the counts must equal the reference's."""
import os
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
import util
from test_au_host import CASES, case, counts_of, multiscale_reference
from test_gpu_rell import random_walk_matrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD = os.path.join(ROOT, "root_digger_amd", "bin", "rd_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
MSA, TREE = os.path.join(util.DATA, "10.fasta"), os.path.join(util.DATA, "10.tree")
U = 2.0 ** -53


def near_ties(ref_sums, n_draws):
    """-> involved[K][rows]: per scale and row the near-tie replicates that involve the row,
    near[K]: near-tie replicates per scale"""
    K, B, rows = ref_sums.shape
    involved, near = np.zeros((K, rows), dtype=np.int64), np.zeros(K, dtype=np.int64)
    if rows == 1:
        return involved, near
    for k in range(K):
        width = 4 * n_draws[k] * U * float(np.max(np.abs(ref_sums[k])))
        top = np.sort(ref_sums[k], axis=1)
        tie = top[:, -1] - top[:, -2] <= width
        near[k] = tie.sum()
        involved[k] = (ref_sums[k][tie] >= top[tie, -1:] - width).sum(axis=0)
    return involved, near


def check_counts(counts, ref_sums, n_draws, what):
    K, B, rows = ref_sums.shape
    assert counts.shape == (K, rows) and counts.dtype == np.uint32
    assert np.all(counts.sum(axis=1) == B)
    involved, near = near_ties(ref_sums, n_draws)
    want = counts_of(ref_sums)
    off = np.abs(counts.astype(np.int64) - want.astype(np.int64))
    print("%s: %d near ties in %d replicates, largest |count - reference| %d"
          % (what, int(near.sum()), K * B, int(off.max())))
    assert near.sum() <= 0.01 * K * B
    assert np.all(off <= involved)
    return want, near


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_sums_and_p_au_match_numpy(name):
    matrix, weights, n_draws, B, seed, ref = case(name)
    n = int(weights.sum())
    counts, sums = rd.rell_multiscale(matrix, weights, n_draws, B, seed, return_sums=True)
    assert rd.rell_last_multiscale_ms() > 0.0
    # sums by scale
    for k, m in enumerate(n_draws):
        bound = 2 * m * U * float(np.max(np.abs(ref[k])))
        err = float(np.max(np.abs(sums[k] - ref[k])))
        print("%s scale %d (M = %d): largest |sum - reference| %.3e (bound %.3e)" % (name, k, m, err, bound))
        assert err <= bound
    # the reference alone shows no near tie on these inputs: the counts are the reference's
    want, near = check_counts(counts, ref, n_draws, name)
    assert near.sum() == 0
    assert np.array_equal(counts, want)
    assert np.array_equal(counts, counts_of(sums))
    # without the sums: the same counts
    assert np.array_equal(rd.rell_multiscale(matrix, weights, n_draws, B, seed), counts)
    # the whole test is the fit of these counts, and the input is not degenerate
    fit = rd.au_fit(want, n_draws, n, B)
    got = rd.au_test(matrix, weights, B, seed)
    assert got["n_draws"] == n_draws and np.array_equal(got["counts"], counts)
    for key in ("p_au", "se", "d", "c", "rss", "used", "df"):
        assert np.array_equal(got[key], fit[key]), key
    fitted = int((got["used"] >= 2).sum())
    print("%s: %d of %d rows fitted, %d kept at 0.05" % (name, fitted, len(fit["used"]), int((got["p_au"] >= 0.05).sum())))
    assert fitted == {"walk40": 31, "walk197": 75}[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_scale_of_the_alignment_is_the_bootstrap(name):
    matrix, weights, n_draws, B, seed, _ = case(name)
    assert n_draws[5] == int(weights.sum())
    counts, sums = rd.rell_multiscale(matrix, weights, n_draws, B, seed, return_sums=True)
    bp, _, plain = rd.rell_bootstrap(matrix, weights, B, seed=rd.rell_scale_seed(seed, 5), return_sums=True)
    assert np.array_equal(sums[5], plain)
    assert np.array_equal(counts[5], np.rint(bp * B)) and np.all(np.abs(bp * B - counts[5]) < 1e-9)


def test_every_launch_shape_of_a_scale_is_the_bootstrap():
    """the bootstrap and the multiscale bootstrap are one kernel template: at every lane count and
    rows per lane, and in the chunked path beyond 256 rows, the scale that draws N columns has the
    bootstrap's bits and its winners (no tolerance: equal, or the two tails have diverged)"""
    matrix = random_walk_matrix(300, 1237, 3)
    weights = np.random.default_rng(6).integers(1, 4, 1237).astype(np.uint32)
    n, B, seed = int(weights.sum()), 37, 3
    n_draws = [n // 2, n, 7 * n // 5]
    for rows in (1, 5, 9, 17, 33, 64, 65, 129, 257, 300):
        counts, sums = rd.rell_multiscale(matrix[:rows], weights, n_draws, B, seed, return_sums=True)
        bp, _, plain = rd.rell_bootstrap(matrix[:rows], weights, B, seed=rd.rell_scale_seed(seed, 1), return_sums=True)
        assert np.array_equal(sums[1], plain), rows
        assert np.array_equal(counts[1], np.rint(bp * B)), rows


def test_launch_shapes_give_the_same_bits():
    """8, 16, 32 or 64 lanes per replicate, one, two or four rows per lane, one wave per replicate
    up to 256 rows and chunk waves with the second kernel beyond"""
    matrix = random_walk_matrix(300, 1237, 3)
    weights = np.random.default_rng(6).integers(1, 4, 1237).astype(np.uint32)
    n, B, seed = int(weights.sum()), 200, 3
    n_draws = [n // 2, n, 7 * n // 5]
    ref = multiscale_reference(matrix, weights, n_draws, B, seed)
    whole = None
    for rows in (300, 257, 256, 129, 65, 64, 17, 5, 1):
        counts, sums = rd.rell_multiscale(matrix[:rows], weights, n_draws, B, seed, return_sums=True)
        assert sums.shape == (3, B, rows)
        if whole is None:
            whole = sums
            for k, m in enumerate(n_draws):
                assert np.max(np.abs(sums[k] - ref[k])) <= 2 * m * U * float(np.max(np.abs(ref[k])))
        assert np.array_equal(sums, whole[:, :, :rows]), rows
        check_counts(counts, ref[:, :, :rows], n_draws, "%d rows" % rows)
        assert np.array_equal(counts, counts_of(sums)), rows
        if rows == 1:
            assert np.all(counts == B)
            assert np.all(rd.au_fit(counts, n_draws, n, B)["p_au"] == 1.0)
            assert rd.au_test(matrix[:1], weights, B, seed)["p_au"][0] == 1.0


def test_ties_go_to_the_lowest_row():
    matrix = random_walk_matrix(197, 3000, 2)
    weights = np.random.default_rng(5).integers(1, 4, 3000).astype(np.uint32)
    # a row that beats every other row at every site, three times over
    matrix[3] = matrix.max(axis=0)
    matrix[0] = matrix[3]
    matrix[40] = matrix[3]
    n_draws = rd.au_scales(int(weights.sum()))
    for rows in (197, 41):      # (four rows per lane: rows 0 and 3 share a lane; one row per lane)
        counts, sums = rd.rell_multiscale(matrix[:rows], weights, n_draws, 60, 99, return_sums=True)
        assert np.array_equal(sums[:, :, 0], sums[:, :, 3]) and np.array_equal(sums[:, :, 40], sums[:, :, 3])
        assert np.all(counts[:, 0] == 60) and counts.sum() == 600
        got = rd.au_test(matrix[:rows], weights, 60, 99)
        assert got["p_au"][0] == 1.0 and got["p_au"][3] == 0.0 and got["p_au"][40] == 0.0
    # beyond 256 rows the winner is picked among chunks: the same row in the first and the last chunk
    tall = random_walk_matrix(300, 700, 8)
    tall[290] = tall.max(axis=0)
    tall[7] = tall[290]
    tall[260] = tall[290]
    w = np.ones(700, dtype=np.uint32)
    counts = rd.rell_multiscale(tall, w, [350, 700, 980], 50, 4)
    assert np.all(counts[:, 7] == 50) and counts.sum() == 150


def test_a_pattern_of_weight_zero_is_never_drawn():
    rng = np.random.default_rng(7)
    matrix = random_walk_matrix(20, 500, 4)
    weights = rng.integers(1, 4, 500).astype(np.uint32)
    poisoned, w0 = matrix.copy(), weights.copy()
    for p in (0, 77, 499):
        poisoned[:, p] = np.nan
        w0[p] = 0
    keep = w0 > 0
    n_draws = rd.au_scales(int(w0.sum()))
    counts, sums = rd.rell_multiscale(poisoned, w0, n_draws, 50, 11, return_sums=True)
    assert np.all(np.isfinite(sums))
    counts1, sums1 = rd.rell_multiscale(matrix[:, keep], weights[keep], n_draws, 50, 11, return_sums=True)
    assert np.array_equal(sums, sums1) and np.array_equal(counts, counts1)


def test_repeats_and_prefixes():
    matrix, weights, n_draws, _, seed, _ = case("walk40")
    counts, sums = rd.rell_multiscale(matrix, weights, n_draws, 200, seed, return_sums=True)
    counts2, sums2 = rd.rell_multiscale(matrix, weights, n_draws, 200, seed, return_sums=True)
    assert np.array_equal(sums2, sums) and np.array_equal(counts2, counts)
    counts1, first = rd.rell_multiscale(matrix, weights, n_draws, 100, seed, return_sums=True)
    assert np.array_equal(first, sums[:, :100])
    assert np.array_equal(counts1, counts_of(sums[:, :100]))
    # a scale's sums do not depend on the other scales of the call, only on its index and length
    _, three = rd.rell_multiscale(matrix, weights, [n_draws[0], 17, n_draws[2]], 100, seed, return_sums=True)
    assert np.array_equal(three[0], first[0]) and np.array_equal(three[2], first[2])
    assert not np.array_equal(rd.rell_multiscale(matrix, weights, n_draws, 100, seed + 1, return_sums=True)[1], first)


def test_bad_arguments_fail_with_an_error_number():
    matrix = random_walk_matrix(4, 10, 5)
    ones = np.ones(10, dtype=np.uint32)
    huge = np.full(10, 1 << 31, dtype=np.uint32)           # N = 10 * 2^31 >= 2^32
    for w, n_draws, B in ((ones, [10], 10), (ones, [5, 0, 10], 10), (ones, [5, 10, 5], 10), (ones, [5, 10], 0),
                          (ones, [5, 1 << 32], 10), (ones, list(range(1, 66)), 10), (huge, [5, 10], 10),
                          (np.zeros(10, dtype=np.uint32), [5, 10], 10)):
        with pytest.raises(rd.RdamdError):
            rd.rell_multiscale(matrix, w, n_draws, B)
        assert rd.lib.rdamd_errno() == 62
    with pytest.raises(rd.RdamdError):
        rd.rell_multiscale(matrix[:0], ones, [5, 10], 10)
    assert rd.lib.rdamd_errno() == 62
    counts = rd.rell_multiscale(matrix, ones, [5, 10], 10)  # (and the library is fine afterwards)
    assert counts.shape == (2, 4) and np.all(counts.sum(axis=1) == 10)


def _run(args, **kw):
    return subprocess.run([RD] + args, capture_output=True, text=True, timeout=600, **kw)


def test_rd_amd_au(tmp_path):
    # the flags of test_rd_amd_root_tests: one candidate after the other, two runs are compared byte for byte
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--rate-cats", "4", "--lockstep", "0", "--threads", "0",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(REF):
        common += ["--lbfgsb", REF]
    prefix = str(tmp_path / "au")
    out = _run(common + ["--prefix", prefix, "--rell", "1000", "--au", "--root-tests"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Root tests:" in out.stdout and os.path.exists(prefix + ".roottests.tsv")
    records = rd.Checkpoint(prefix).read_results()
    assert sorted(r[0] for r in records) == list(range(17))

    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=4, seed=5)
    m.initialize_partitions()
    weights, _ = m.site_patterns()
    rls = [tree.root_location(r[0]).with_ratio(r[2]) for r in records]
    matrix = m.site_lnls(rls, [r[3] for r in records])
    got = rd.au_test(matrix, weights, 1000, seed=5)
    print("10.fasta: p_au %s" % " ".join("%.3f" % v for v in got["p_au"]))
    kept = int((got["p_au"] >= 0.05).sum())
    assert "AU test: %d of 17 roots kept at 0.05" % kept in out.stdout

    rows = [l.split("\t") for l in open(prefix + ".au.tsv").read().splitlines()]
    assert rows[0] == ["root_id", "llh", "p_au", "se", "d", "c", "rss", "df", "used"] and len(rows) == 18
    assert [int(r[0]) for r in rows[1:]] == list(range(17))
    by_id = {rec[0]: k for k, rec in enumerate(records)}
    for r in rows[1:]:
        k = by_id[int(r[0])]
        assert float(r[1]) == records[k][1]
        for col, key in zip(r[2:7], ("p_au", "se", "d", "c", "rss")):
            assert float(col) == got[key][k], key
        assert int(r[7]) == got["df"][k] and int(r[8]) == got["used"][k]
    nw = open(prefix + ".lwr.tree").read()
    assert nw.count("LWR=") > 0
    for key in ("pAU=", "BP=", "ELW=", "pKH="):
        assert nw.count(key) == nw.count("LWR="), key
    assert rd.Tree.from_newick(nw).tip_count() == 10

    # --rell alone, the same seeds: what it writes is what it wrote, and nothing new
    plain = str(tmp_path / "plain")
    out2 = _run(common + ["--prefix", plain, "--rell", "1000"])
    assert out2.returncode == 0, out2.stdout + out2.stderr
    assert "AU test:" not in out2.stdout
    assert not os.path.exists(plain + ".au.tsv")
    assert "pAU=" not in open(plain + ".lwr.tree").read()
    for ext in (".support.tsv", ".rooted.tree"):
        assert open(plain + ext, "rb").read() == open(prefix + ext, "rb").read(), ext


@pytest.mark.parametrize("extra", [[], ["--rell", "1"], ["--rell", "100", "--site-shards", "2"],
                                   ["--rell", "100", "--no-checkpoint"]])
def test_rd_amd_au_needs_rell(tmp_path, extra):
    out = _run(["--msa", MSA, "--tree", TREE, "--silent", "--exhaustive", "--prefix", str(tmp_path / "no"), "--au"]
               + extra)
    assert out.returncode != 0
    assert ("--au" if len(extra) < 3 else "--rell") in out.stdout + out.stderr
    assert not os.path.exists(str(tmp_path / "no") + ".au.tsv")
