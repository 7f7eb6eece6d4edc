"""Host side of the AU test (no GPU): au_fit (rdamd_au_fit) against a SciPy restatement of its
definition in include/root_digger_amd.h, constructed counts, the scale seed and the scales.

Tolerance of the SciPy comparison (derived, not tuned): both sides get the same integer counts, so
the only freedom is the quantile function and the rounding of sums of at most ten terms.  Perturbing
every quantile by 1e-13 relative moved p_au by at most 2.8e-12 on these inputs, an amplification of
about 30; AS 241 and scipy.special.ndtri are good to about 1e-16 relative.  1e-9 (absolute for p_au,
d, c; relative for rss, se) leaves four orders of margin, and a wrong weight or a swapped regressor
still fails.  rss is compared where it has degrees of freedom (used >= 3); with used = 2 it is exactly 0."""
import functools

import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import norm

import root_digger_amd as rd
from test_gpu_rell import random_walk_matrix
from test_rell_host import M64, column_np, sm_int


def multiscale_reference(site_lnl, weights, n_draws, n_replicates, seed):
    """-> sums[K][B][rows] from the definitions: scale seed, column_np, counts @ site_lnl.T"""
    site_lnl = np.asarray(site_lnl, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.int64)
    n = int(weights.sum())
    col2pat = np.repeat(np.arange(len(weights)), weights)
    sums = np.empty((len(n_draws), n_replicates, site_lnl.shape[0]))
    for k, m in enumerate(n_draws):
        d = np.arange(m, dtype=np.uint64)
        scale_seed = np.uint64(sm_int((seed + k + 1) & M64))
        hits = np.zeros((n_replicates, len(weights)), dtype=np.float64)
        for b in range(n_replicates):
            cols = column_np(scale_seed, np.uint64(b), d, np.uint64(n))
            hits[b] = np.bincount(col2pat[cols.astype(np.int64)], minlength=len(weights))
        assert np.all(hits.sum(axis=1) == m)
        sums[k] = hits @ site_lnl.T
    return sums


def counts_of(sums):
    """counts[K][rows]: replicates won, the first of equals"""
    rows = sums.shape[2]
    return np.stack([np.bincount(np.argmax(s, axis=1), minlength=rows) for s in sums]).astype(np.uint32)


CASES = {
    # name: rows, patterns, matrix seed, weights seed, B, seed
    "walk40": (40, 1237, 3, 6, 500, 3),
    "walk197": (197, 3000, 1, 4, 1000, 7),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> matrix, weights, n_draws, B, seed, reference sums (computed once; treat as read-only)"""
    rows, patterns, mseed, wseed, b, seed = CASES[name]
    matrix = random_walk_matrix(rows, patterns, mseed)
    weights = np.random.default_rng(wseed).integers(1, 4, patterns).astype(np.uint32)
    n_draws = rd.au_scales(int(weights.sum()))
    sums = multiscale_reference(matrix, weights, n_draws, b, seed)
    for a in (matrix, weights, sums):
        a.setflags(write=False)
    return matrix, weights, n_draws, b, seed, sums


def scipy_fit(counts, n_draws, n_columns, b):
    """the definitions in include/root_digger_amd.h, restated with SciPy"""
    counts = np.asarray(counts, dtype=np.int64)
    r = np.asarray(n_draws, dtype=np.float64) / float(n_columns)
    nearest = int(np.argmin(np.abs(np.asarray(n_draws, dtype=np.int64) - int(n_columns))))
    out = {k: np.zeros(counts.shape[1]) for k in ("p_au", "d", "c", "rss", "se")}
    out["used"] = np.zeros(counts.shape[1], dtype=np.int64)
    for i in range(counts.shape[1]):
        ok = (counts[:, i] > 0) & (counts[:, i] < b)
        out["used"][i] = ok.sum()
        if ok.sum() < 2:
            out["p_au"][i] = counts[nearest, i] / b
            continue
        p = counts[ok, i] / b
        z = -ndtri(p)
        w = norm.pdf(z) ** 2 * b / (p * (1.0 - p))
        x1, x2 = np.sqrt(r[ok]), 1.0 / np.sqrt(r[ok])
        a11, a12, a22 = np.sum(w * x1 * x1), np.sum(w * x1 * x2), np.sum(w * x2 * x2)
        t1, t2 = np.sum(w * x1 * z), np.sum(w * x2 * z)
        det = a11 * a22 - a12 * a12
        d, c = (a22 * t1 - a12 * t2) / det, (a11 * t2 - a12 * t1) / det
        out["d"][i], out["c"][i] = d, c
        out["p_au"][i] = norm.sf(d - c)
        out["rss"][i] = np.sum(w * (z - d * x1 - c * x2) ** 2)
        out["se"][i] = norm.pdf(d - c) * np.sqrt((a11 + a22 + 2.0 * a12) / det)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_au_fit_matches_the_scipy_restatement(name):
    matrix, weights, n_draws, b, seed, sums = case(name)
    n = int(weights.sum())
    counts = counts_of(sums)
    assert np.all(counts.sum(axis=1) == b)
    got = rd.au_fit(counts, n_draws, n, b)
    want = scipy_fit(counts, n_draws, n, b)
    fitted = want["used"] >= 2
    print("%s: %d of %d rows with at least two usable scales" % (name, int(fitted.sum()), len(fitted)))
    assert fitted.sum() >= 10
    assert np.array_equal(got["used"], want["used"])
    assert np.array_equal(got["df"], np.maximum(want["used"] - 2, 0))
    for key in ("p_au", "d", "c"):
        err = float(np.max(np.abs(got[key] - want[key])))
        print("%s: largest |%s - scipy| %.3e" % (name, key, err))
        assert err <= 1e-9
    # two usable scales are fitted exactly: rss is 0 by definition there and the restatement's
    # value is its own rounding residue (1e-28 here), against which no relative error exists
    exact = want["used"] == 2
    assert np.all(got["rss"][exact] == 0.0) and np.all(want["rss"][exact] <= 1e-20)
    for key, rows in (("rss", want["used"] >= 3), ("se", fitted)):
        err = float(np.max(np.abs(got[key][rows] - want[key][rows]) / np.abs(want[key][rows])))
        print("%s: largest relative error of %s %.3e over %d rows" % (name, key, err, int(rows.sum())))
        assert err <= 1e-9
        assert np.all(got[key][~fitted] == 0.0)
    assert np.all((got["p_au"] >= 0.0) & (got["p_au"] <= 1.0))


@pytest.mark.parametrize("d0,c0", [(1.0, 0.3), (-0.5, 0.2), (2.0, -0.4)])
def test_au_fit_recovers_the_normal_model(d0, c0):
    """exact counts of the model z = d sqrt(r) + c / sqrt(r); rounding a count moves z by at most
    1 / (2 B phi(z)), about 1e-5 here, so 1e-3 on p_au is wide"""
    b, n = 10 ** 6, 10000
    n_draws = rd.au_scales(n)
    r = np.array(n_draws) / n
    counts = np.round(b * norm.cdf(-(d0 * np.sqrt(r) + c0 / np.sqrt(r)))).astype(np.uint32)[:, None]
    assert np.all((counts > 0) & (counts < b))
    got = rd.au_fit(counts, n_draws, n, b)
    print("d0 %.1f c0 %.1f: p_au %.6f (model %.6f), d %.6f, c %.6f, rss %.3e, se %.3e"
          % (d0, c0, got["p_au"][0], norm.sf(d0 - c0), got["d"][0], got["c"][0], got["rss"][0], got["se"][0]))
    assert got["used"][0] == 10 and got["df"][0] == 8
    assert abs(got["p_au"][0] - norm.sf(d0 - c0)) <= 1e-3
    assert abs(got["d"][0] - d0) <= 1e-3 and abs(got["c"][0] - c0) <= 1e-3
    assert got["se"][0] > 0.0 and got["rss"][0] >= 0.0


def test_au_fit_without_two_usable_scales():
    b, n = 1000, 2000
    n_draws = rd.au_scales(n)
    counts = np.zeros((10, 4), dtype=np.uint32)
    counts[:, 1] = b                       # row 1 wins everything
    counts[:, 2] = 0
    counts[7, 2] = 17                      # row 2: one usable scale, not the nearest one
    counts[:, 3] = b
    counts[5, 3] = 900                     # row 3: one usable scale, the nearest one
    got = rd.au_fit(counts, n_draws, n, b)
    assert list(got["used"]) == [0, 0, 1, 1] and list(got["df"]) == [0, 0, 0, 0]
    assert list(got["p_au"]) == [0.0, 1.0, 0.0, 0.9]
    for key in ("d", "c", "rss", "se"):
        assert np.all(got[key] == 0.0)
    # the nearest scale, the lowest k among equals: 1900 and 2100 are equally far from 2000
    never, always = np.array([[0], [b]], dtype=np.uint32), np.array([[b], [0]], dtype=np.uint32)
    assert rd.au_fit(never, [1900, 2100], n, b)["p_au"][0] == 0.0
    assert rd.au_fit(always, [2100, 1900], n, b)["p_au"][0] == 1.0
    assert rd.au_fit(always, [1000, 2001], n, b)["p_au"][0] == 0.0


def test_au_fit_refuses_bad_arguments():
    ok = np.full((3, 2), 5, dtype=np.uint32)
    for counts, n_draws, n, b in ((ok[:1], [100], 100, 10), (ok, [50, 100, 0], 100, 10),
                                  (ok, [50, 100, 100], 100, 10), (ok, [50, 100, 150], 100, 0),
                                  (ok, [50, 100, 150], 0, 10), (ok, [50, 100, 1 << 32], 100, 10),
                                  (ok, [50, 100, 150], 100, 4)):
        with pytest.raises(rd.RdamdError):
            rd.au_fit(counts, n_draws, n, b)
        assert rd.lib.rdamd_errno() == 62
    assert rd.au_fit(ok, [50, 100, 150], 100, 10)["used"].tolist() == [3, 3]


def test_scale_seed_matches_its_definition():
    rng = np.random.default_rng(20261017)
    seeds = [int(s) for s in rng.integers(0, 1 << 64, 2000, dtype=np.uint64)] + [M64, M64 - 1, 0]
    ks = [int(k) for k in rng.integers(0, 64, len(seeds))]
    for seed, k in zip(seeds, ks):
        assert rd.rell_scale_seed(seed, k) == sm_int((seed + k + 1) & M64)
    assert rd.rell_scale_seed(M64, 0) == sm_int(0)
    assert len({rd.rell_scale_seed(1, k) for k in range(10)}) == 10


@pytest.mark.parametrize("n", [1, 2, 7, 10, 999, 1000, 3713, 50000, (1 << 32) - 1])
def test_au_scales(n):
    s = rd.au_scales(n)
    assert len(s) == 10 and s[5] == n
    assert all(isinstance(v, int) for v in s)
    if n >= 10:   # (steps of n / 10 >= 1; shorter alignments round two scales to the same count)
        assert all(a < b for a, b in zip(s, s[1:]))
    assert all(abs(v - n * (5 + k) / 10) <= 0.5 for k, v in enumerate(s))
