"""rell_tests (rdamd_rell_tests, csrc/kernels_rell_tests.hip): the KH, SH and weighted-SH tests of
candidate roots against a NumPy re-implementation of their definitions in
include/root_digger_amd.h, properties that hold exactly on the device's own output, and the
`rd_amd --rell B --root-tests` outputs.

The reference computes S = counts @ site_lnl.T (the resampled sums), centres it, and counts with
broadcasts.  Every p-value is a count of comparisons `statistic >= observed`; device and reference
can only disagree on a comparison whose two sides are closer than the sum of both sides' errors (a
NEAR TIE), so per row and test the device's count may differ from the reference's by at most the
number of near ties in that row.  A comparison whose two sides are both exactly 0 in the reference
is exact on the device as well (x - x = 0, and a maximum that contains the zero term) and is never
a near tie.

Bounds (derived, not tuned).  u = 2**-53, N columns, B replicates,
delta = 2 N u max|S_ref|: the bound of test_gpu_rell.py for one resampled sum, and it also bounds
an observed total (N weighted same-sign terms no larger) and a mean of sums (B values of that
error, plus B u relative for the averaging, which 2 N u covers for B <= N and which is far below
the unit otherwise).
  lnl      relative 2 N u: at most N roundings of same-sign partial sums on either side;
  KH, SH   a statistic is sum - mean - (sum - mean) and the observed value a difference of two
           totals: two sums, two means, two totals, each within delta -> near tie when
           |stat_ref - obs_ref| <= 8 delta;
  spread   s is the root mean square of d_b = c[b][i] - c[b][j]; each d_b is off by at most
           4 delta (two sums, two means), which moves a root mean square by at most 4 delta
           (triangle inequality in l2 / sqrt(B - 1)); adding B squares in any order and a square
           root cost at most (B + 2) u relative on s^2, B u on s; the reference's own d_b carry the
           same errors -> |s - s_ref| <= 6 delta + 2 B u s_ref  (4 delta + slack for the two sides'
           roundings of the subtractions themselves);
  WSH      a term is (x_j - x_i) / s: its numerator is off by at most 4 delta, its denominator by
           e_s = 6 delta + 2 B u s_max, so the term moves by at most
           (4 delta + T_max e_s) / s_min, T_max the largest statistic of the reference and s_min,
           s_max its smallest positive and its largest spread (multiplying with the rounded
           reciprocal instead of dividing adds 2 u relative, far inside e_s / s); both sides of a
           comparison move -> near tie when |t_ref(c[b]) - t_ref(lnl)| <= 2 (4 delta + T_max e_s) / s_min.
Conditions on the inputs, not measurements: at most 1 % of the B n comparisons of a test may be
near ties, and the two largest lnl_ref must differ by more than 4 delta (else m is not defined
beyond rounding).  On the two inputs of the first test the reference alone shows ZERO near ties in
all three tests, so there the p-values must equal the reference's exactly."""
import functools
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


def random_walk_matrix(rows, patterns, seed):
    """negative site lnLs; a row is a random walk away from its neighbour, per-site steps of 0.02
    (the generator of test_gpu_rell.py, repeated here so that this file stands on its own)"""
    rng = np.random.default_rng(seed)
    m = np.empty((rows, patterns))
    m[0] = -rng.uniform(1.0, 12.0, patterns)
    for i in range(1, rows):
        m[i] = np.minimum(m[i - 1] + rng.normal(0.0, 0.02, patterns), -1e-3)
    return m


def resampled_sums(site_lnl, weights, n_replicates, seed):
    """S[B][rows] = counts @ site_lnl.T from the definition of the draws"""
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
    return counts @ site_lnl.T


def reference_tests(S, lnl, n_columns):
    """the three tests from the resampled sums S[B][n] and the observed totals lnl[n] -> dict:
    counts and near-tie counts per row of every test, the spreads, and the figures of the bounds"""
    B, n = S.shape
    delta = 2 * n_columns * U * float(np.max(np.abs(S)))
    m = int(np.argmax(lnl))                                   # the first of equals
    c = S - S.mean(axis=0)
    obs = lnl[m] - lnl
    out = {"m": m, "delta": delta, "B": B}

    def count(stat, observed, width):
        near = (np.abs(stat - observed) <= width) & ~((stat == 0.0) & (observed == 0.0))
        return (stat >= observed).sum(axis=0), near.sum(axis=0)

    out["kh"], out["kh_near"] = count(c[:, [m]] - c, obs, 8 * delta)
    out["sh"], out["sh_near"] = count(c.max(axis=1, keepdims=True) - c, obs, 8 * delta)
    spread = np.empty((n, n))
    for i in range(n):
        spread[i] = np.sqrt(((c[:, [i]] - c) ** 2).sum(axis=0) / (B - 1))
    out["spread"] = spread
    positive = spread > 0.0
    t_obs, t_rep = np.zeros(n), np.zeros((B, n))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            if positive[i].any():
                t_obs[i] = max(0.0, float(np.max((lnl[positive[i]] - lnl[i]) / spread[i, positive[i]])))
                t_rep[:, i] = np.maximum(0.0, np.max((c[:, positive[i]] - c[:, [i]]) / spread[i, positive[i]], axis=1))
    if positive.any():
        s_min, s_max = float(spread[positive].min()), float(spread.max())
        t_max = max(float(t_obs.max()), float(t_rep.max()))
        width = 2 * (4 * delta + t_max * (6 * delta + 2 * B * U * s_max)) / s_min
    else:
        s_min = s_max = t_max = width = 0.0
    out.update(s_min=s_min, s_max=s_max, t_max=t_max, wsh_width=width)
    out["wsh"], out["wsh_near"] = count(t_rep, t_obs, width)
    top = np.sort(lnl)
    out["lnl_gap"] = float(top[-1] - top[-2]) if n > 1 else np.inf
    return out


def check_against_reference(got, ref, lnl_ref, n_columns, what, spread=None):
    B, n = ref["B"], len(lnl_ref)
    delta = ref["delta"]
    print("%s: B = %d, n = %d, delta %.3e, smallest positive spread %.4g, largest %.4g, T_max %.4g, WSH tie "
          "width %.3e, gap of the two largest lnl %.3e" % (what, B, n, delta, ref["s_min"], ref["s_max"], ref["t_max"],
                                                          ref["wsh_width"], ref["lnl_gap"]))
    assert ref["lnl_gap"] > 4 * delta
    err = float(np.max(np.abs(got["lnl"] - lnl_ref) / np.abs(lnl_ref)))
    print("%s: largest relative error of lnl %.3e (bound %.3e)" % (what, err, 2 * n_columns * U))
    assert err <= 2 * n_columns * U
    assert int(np.argmax(got["lnl"])) == ref["m"]
    if spread is not None:
        bound = 6 * delta + 2 * B * U * ref["spread"]
        worst = float(np.max(np.abs(spread - ref["spread"]) - bound))
        print("%s: largest |spread - reference| %.3e (bound from %.3e), worst excess over the bound %.3e"
              % (what, float(np.max(np.abs(spread - ref["spread"]))), 6 * delta, worst))
        assert np.all(np.abs(spread - ref["spread"]) <= bound)
        assert np.array_equal(spread, spread.T) and np.all(np.diag(spread) == 0.0)
    for key in ("kh", "sh", "wsh"):
        counts = np.round(got["p_" + key] * B)                   # ((k / B) * B need not be k in floating point)
        assert np.array_equal(counts / B, got["p_" + key]), key    # p is an integer count over B, exactly
        near = ref[key + "_near"]
        share = near.sum() / float(B * n)
        print("%s: %s: %d near ties of %d comparisons (%.4f %%), %d rows with p >= 0.05, %d distinct p-values, "
              "largest |count - reference| %d" % (what, key.upper(), int(near.sum()), B * n, 100.0 * share,
                                                 int((got["p_" + key] >= 0.05).sum()), len(np.unique(got["p_" + key])),
                                                 int(np.max(np.abs(counts - ref[key])))))
        assert share <= 0.01, key
        assert np.all(np.abs(counts - ref[key]) <= near), key


@functools.lru_cache(maxsize=None)
def case(name):
    """-> matrix, weights, B, seed, S_ref, lnl_ref, reference (computed once per session)"""
    if name == "walk197":
        matrix = random_walk_matrix(197, 3000, 1)
        weights = np.random.default_rng(4).integers(1, 4, 3000).astype(np.uint32)
        B, seed = 2000, 7
    elif name == "walk40":
        matrix = random_walk_matrix(40, 1237, 3)
        weights = np.random.default_rng(6).integers(1, 4, 1237).astype(np.uint32)
        B, seed = 500, 3
    else:
        raise KeyError(name)
    S = resampled_sums(matrix, weights, B, seed)
    lnl = matrix @ weights.astype(np.float64)
    return matrix, weights, B, seed, S, lnl, reference_tests(S, lnl, int(weights.sum()))


@pytest.mark.parametrize("name,keep,distinct", [("walk197", (144, 188, 145), 160), ("walk40", None, 32)])
def test_rell_tests_match_numpy(name, keep, distinct):
    matrix, weights, B, seed, S, lnl, ref = case(name)
    got = rd.rell_tests(matrix, weights, B, seed, return_spread=True)
    assert sorted(got) == ["bp", "elw", "lnl", "p_kh", "p_sh", "p_wsh", "spread"]
    check_against_reference(got, ref, lnl, int(weights.sum()), name, got["spread"])
    # the reference alone shows no near tie on these inputs: the p-values are the reference's
    for key in ("kh", "sh", "wsh"):
        assert ref[key + "_near"].sum() == 0
        assert np.array_equal(got["p_" + key], ref[key] / float(B)), key
        assert len(np.unique(got["p_" + key])) >= distinct, key         # (the inputs are not degenerate)
    if keep:
        assert tuple(int((got["p_" + k] >= 0.05).sum()) for k in ("kh", "sh", "wsh")) == keep


def test_bp_elw_and_sums_are_the_bootstraps():
    for name in ("walk197", "walk40"):
        matrix, weights, B, seed = case(name)[:4]
        bp, elw, sums = rd.rell_bootstrap(matrix, weights, B, seed, return_sums=True)
        got = rd.rell_tests(matrix, weights, B, seed, return_sums=True)
        assert np.array_equal(got["bp"], bp) and np.array_equal(got["elw"], elw)
        assert np.array_equal(got["sums"], sums)
        assert rd.rell_last_tests_ms() > 0.0 and rd.rell_last_resample_ms() > 0.0
        bp2, elw2 = rd.rell_bootstrap(matrix, weights, B, seed)         # (and the bootstrap after the tests)
        assert np.array_equal(bp2, bp) and np.array_equal(elw2, elw)


def test_properties_that_hold_exactly():
    matrix, weights, B, seed = case("walk40")[:4]
    got = rd.rell_tests(matrix, weights, B, seed)
    m = int(np.argmax(got["lnl"]))
    assert got["p_kh"][m] == 1.0 and got["p_sh"][m] == 1.0 and got["p_wsh"][m] == 1.0
    assert np.all(got["p_sh"] >= got["p_kh"])
    for key in ("p_kh", "p_sh", "p_wsh"):
        assert np.array_equal(np.round(got[key] * B) / B, got[key])       # an integer count over B, exactly
        assert np.all((got[key] >= 0.0) & (got[key] <= 1.0))
    # KH looks at two rows only: the pair {m, i} on its own gives the same p-value, and SH is KH there
    for i in (0, 7, 19, 39):
        if i == m:
            continue
        pair = rd.rell_tests(matrix[[m, i]], weights, B, seed)
        assert pair["lnl"][0] == got["lnl"][m] and pair["lnl"][1] == got["lnl"][i]
        assert pair["p_kh"][1] == got["p_kh"][i], i
        assert np.array_equal(pair["p_sh"], pair["p_kh"])
        assert pair["p_kh"][0] == 1.0
    again = rd.rell_tests(matrix, weights, B, seed)
    for key in got:
        assert np.array_equal(again[key], got[key]), key
    one = rd.rell_tests(matrix[:1], weights, B, seed, return_spread=True)
    assert one["p_kh"][0] == 1.0 and one["p_sh"][0] == 1.0 and one["p_wsh"][0] == 1.0
    assert one["bp"][0] == 1.0 and one["spread"].shape == (1, 1) and one["spread"][0, 0] == 0.0


def test_duplicated_rows():
    rng = np.random.default_rng(5)
    matrix = random_walk_matrix(197, 3000, 2)
    weights = rng.integers(1, 4, 3000).astype(np.uint32)
    # a row that beats every other row at every site, three times over
    matrix[3] = matrix.max(axis=0)
    matrix[0] = matrix[3]
    matrix[40] = matrix[3]
    got = rd.rell_tests(matrix, weights, 100, 99, return_sums=True, return_spread=True)
    sums, spread = got["sums"], got["spread"]
    assert np.array_equal(sums[:, 0], sums[:, 3]) and np.array_equal(sums[:, 40], sums[:, 3])
    assert got["lnl"][0] == got["lnl"][3] == got["lnl"][40] == got["lnl"].max()
    assert int(np.argmax(got["lnl"])) == 0                      # m: the lowest of the three
    for a in (0, 3, 40):
        for b in (0, 3, 40):
            assert spread[a, b] == 0.0
    others = [i for i in range(197) if i not in (0, 3, 40)]
    assert np.all(spread[0, others] > 0.0)
    assert np.array_equal(spread[0], spread[3]) and np.array_equal(spread[0], spread[40])
    for key in ("p_kh", "p_sh", "p_wsh"):
        assert got[key][0] == got[key][3] == got[key][40] == 1.0, key
    # the copies change nothing for the other rows: without rows 3 and 40 they get the same p-values
    keep = [i for i in range(197) if i not in (3, 40)]
    fewer = rd.rell_tests(matrix[keep], weights, 100, 99)
    for key in ("p_kh", "p_sh", "p_wsh"):
        assert np.array_equal(fewer[key], got[key][keep]), key


def test_a_pattern_of_weight_zero_changes_nothing():
    rng = np.random.default_rng(7)
    matrix = random_walk_matrix(20, 500, 4)
    weights = rng.integers(1, 4, 500).astype(np.uint32)
    poisoned, w0 = matrix.copy(), weights.copy()
    for p in (0, 77, 499):
        poisoned[:, p] = np.nan
        w0[p] = 0
    keep = w0 > 0
    got = rd.rell_tests(poisoned, w0, 50, 11, return_sums=True, return_spread=True)
    for key in got:
        assert np.all(np.isfinite(got[key])), key
    # the same patterns holding numbers instead of NaN: the same bits everywhere
    clean = rd.rell_tests(matrix, w0, 50, 11, return_sums=True, return_spread=True)
    for key in got:
        assert np.array_equal(got[key], clean[key]), key
    # the patterns removed: the sums are the same bits (their order depends on the columns alone);
    # lnl is summed in an order that depends on the pattern count, so it may move in its last
    # bits, and with it nothing else unless a comparison is a near tie -- the reference says none is
    less = rd.rell_tests(matrix[:, keep], weights[keep], 50, 11, return_sums=True, return_spread=True)
    for key in ("sums", "bp", "elw", "spread"):
        assert np.array_equal(got[key], less[key]), key
    n = int(weights[keep].sum())
    lnl = matrix[:, keep] @ weights[keep].astype(np.float64)
    ref = reference_tests(resampled_sums(matrix[:, keep], weights[keep], 50, 11), lnl, n)
    for result, what in ((got, "weight 0, NaN"), (less, "patterns removed")):
        check_against_reference(result, ref, lnl, n, what, result["spread"])
    for key in ("kh", "sh", "wsh"):
        if ref[key + "_near"].sum() == 0:
            assert np.array_equal(got["p_" + key], less["p_" + key]), key


def test_every_launch_shape_gives_the_same_answers():
    """1, 5, 17, 64, 65, 129 and 300 rows of one matrix whose best row comes first: p_kh of the pair
    {0, 1} is the same whatever else is there, and everything agrees with the reference"""
    rng = np.random.default_rng(6)
    matrix = random_walk_matrix(300, 1237, 3)
    weights = rng.integers(1, 4, 1237).astype(np.uint32)
    n = int(weights.sum())
    B, seed = 200, 3
    lnl = matrix @ weights.astype(np.float64)
    best = int(np.argmax(lnl))
    order = [best] + [i for i in range(300) if i != best]
    matrix, lnl = matrix[order], lnl[order]
    S = resampled_sums(matrix, weights, B, seed)
    want = None
    for rows in (1, 5, 17, 64, 65, 129, 300):
        got = rd.rell_tests(matrix[:rows], weights, B, seed, return_sums=True, return_spread=True)
        assert got["sums"].shape == (B, rows) and got["spread"].shape == (rows, rows)
        if rows == 1:
            assert got["p_kh"][0] == 1.0 and got["p_sh"][0] == 1.0 and got["p_wsh"][0] == 1.0
            assert abs(got["lnl"][0] - lnl[0]) <= 2 * n * U * abs(lnl[0])
            continue
        check_against_reference(got, reference_tests(S[:, :rows], lnl[:rows], n), lnl[:rows], n, "%d rows" % rows,
                                got["spread"])
        if want is None:
            want = (got["p_kh"][1], got["lnl"][:2].copy(), got["spread"][0, 1])
        assert got["p_kh"][1] == want[0], rows
        assert np.array_equal(got["lnl"][:2], want[1]) and got["spread"][0, 1] == want[2], rows


def test_bad_arguments_fail_with_an_error_number():
    matrix = random_walk_matrix(4, 10, 5)
    ones = np.ones(10, dtype=np.uint32)
    with pytest.raises(rd.RdamdError):
        rd.rell_tests(matrix, ones, 1)                         # B = 1: no spread
    assert rd.lib.rdamd_errno() == 62
    with pytest.raises(rd.RdamdError):
        rd.rell_tests(matrix, ones, 0)
    assert rd.lib.rdamd_errno() == 62
    # a missing pointer (p_kh), through the C interface
    buf = [np.zeros(4) for _ in range(5)]
    ptr = [b.ctypes.data_as(rd.api._pd) for b in buf]
    args = (matrix.ctypes.data_as(rd.api._pd), 4, 10, ones.ctypes.data_as(rd.api._pu), 10, 1)
    assert rd.lib.rdamd_rell_tests(*args, ptr[0], ptr[1], ptr[2], None, ptr[3], ptr[4], None, None) != 1
    assert rd.lib.rdamd_errno() == 62
    assert rd.lib.rdamd_rell_tests(*args, ptr[0], None, ptr[2], ptr[1], ptr[3], ptr[4], None, None) != 1
    assert rd.lib.rdamd_errno() == 62
    # 8 193 rows: refused when the pair table is asked for, fine without it (lnl and p_wsh may be NULL)
    tall = np.repeat(random_walk_matrix(3, 2, 6), 2731, axis=0)
    assert tall.shape == (8193, 2)
    two = np.array([2, 3], dtype=np.uint32)
    with pytest.raises(rd.RdamdError):
        rd.rell_tests(tall, two, 10)
    assert rd.lib.rdamd_errno() == 62
    big = [np.zeros(8193) for _ in range(4)]
    bptr = [b.ctypes.data_as(rd.api._pd) for b in big]
    assert rd.lib.rdamd_rell_tests(tall.ctypes.data_as(rd.api._pd), 8193, 2, two.ctypes.data_as(rd.api._pu), 10, 1,
                                   None, bptr[0], bptr[1], bptr[2], bptr[3], None, None, None) == 1
    assert abs(big[0].sum() - 1.0) <= 1e-12 and np.all(big[3] >= big[2]) and big[2].max() == 1.0
    got = rd.rell_tests(tall[:8192], two, 10)                  # (the largest table that is allowed)
    assert got["p_wsh"].max() == 1.0
    got = rd.rell_tests(matrix, ones, 10)                      # (and the library is fine afterwards)
    assert got["bp"].sum() == 1.0 and got["p_kh"].max() == 1.0


def _run(args, **kw):
    return subprocess.run([RD] + args, capture_output=True, text=True, timeout=600, **kw)


def test_rd_amd_root_tests(tmp_path):
    # one candidate after the other (--lockstep 0 --threads 0): free-running replicas leave the
    # records' last digits to the order in which they finish, and two runs are compared byte for byte below
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--rate-cats", "4", "--lockstep", "0", "--threads", "0",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(REF):
        common += ["--lbfgsb", REF]
    prefix = str(tmp_path / "tests")
    out = _run(common + ["--prefix", prefix, "--rell", "1000", "--root-tests"])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Root tests:" in out.stdout
    records = rd.Checkpoint(prefix).read_results()
    assert sorted(r[0] for r in records) == list(range(17))

    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=4, seed=5)
    m.initialize_partitions()
    weights, _ = m.site_patterns()
    rls = [tree.root_location(r[0]).with_ratio(r[2]) for r in records]
    matrix = m.site_lnls(rls, [r[3] for r in records])
    got = rd.rell_tests(matrix, weights, 1000, seed=5)
    in95 = rd.elw_confidence_set(got["elw"])
    for key in ("p_kh", "p_sh", "p_wsh"):
        print("10.fasta: %s %s" % (key, " ".join("%.3f" % v for v in got[key])))

    rows = [l.split("\t") for l in open(prefix + ".roottests.tsv").read().splitlines()]
    assert rows[0] == ["root_id", "llh", "lwr", "bp", "elw", "p_kh", "p_sh", "p_wsh", "in_elw95"] and len(rows) == 18
    assert [int(r[0]) for r in rows[1:]] == list(range(17))
    by_id = {rec[0]: k for k, rec in enumerate(records)}
    support = [l.split("\t") for l in open(prefix + ".support.tsv").read().splitlines()]
    for r, s in zip(rows[1:], support[1:]):
        k = by_id[int(r[0])]
        assert r[:5] == s                                       # (the columns both files have)
        assert float(r[1]) == records[k][1]
        assert float(r[3]) == got["bp"][k] and float(r[4]) == got["elw"][k]
        assert float(r[5]) == got["p_kh"][k] and float(r[6]) == got["p_sh"][k] and float(r[7]) == got["p_wsh"][k]
        assert r[8] in ("0", "1") and int(r[8]) == int(in95[k])
    assert max(float(r[5]) for r in rows[1:]) == 1.0

    nw = open(prefix + ".lwr.tree").read()
    assert nw.count("LWR=") > 0
    for key in ("pKH=", "pSH=", "pWSH=", "BP=", "ELW="):
        assert nw.count(key) == nw.count("LWR="), key
    assert rd.Tree.from_newick(nw).tip_count() == 10

    # --rell alone, the same seeds: what it writes is what it wrote, and nothing new
    plain = str(tmp_path / "plain")
    out2 = _run(common + ["--prefix", plain, "--rell", "1000"])
    assert out2.returncode == 0, out2.stdout + out2.stderr
    assert "Root tests:" not in out2.stdout
    assert not os.path.exists(plain + ".roottests.tsv")
    assert "pKH=" not in open(plain + ".lwr.tree").read()
    for ext in (".support.tsv", ".rooted.tree"):
        assert open(plain + ext, "rb").read() == open(prefix + ext, "rb").read(), ext

    # --silent: no line
    quiet = str(tmp_path / "quiet")
    out3 = _run(common + ["--prefix", quiet, "--rell", "1000", "--root-tests", "--silent"])
    assert out3.returncode == 0, out3.stdout + out3.stderr
    assert "Root tests:" not in out3.stdout
    assert open(quiet + ".roottests.tsv", "rb").read() == open(prefix + ".roottests.tsv", "rb").read()


def test_rd_amd_root_tests_needs_rell(tmp_path):
    out = _run(["--msa", MSA, "--tree", TREE, "--silent", "--exhaustive", "--prefix", str(tmp_path / "no"),
                "--root-tests"])
    assert out.returncode != 0
    assert "--root-tests" in out.stdout + out.stderr
    assert not os.path.exists(str(tmp_path / "no") + ".roottests.tsv")
