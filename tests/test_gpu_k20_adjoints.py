"""The adjoints of the pair sums on the matrix cores: the device route of rdamd_pair_sum_adjoints
(csrc/kernels_block_exp.hip, one (branch, rate) problem per wave, every 20 x 20 x 20 product as 20
v_mfma_f64_16x16x4_f64) against the host route, and Model.gradient / Model.substitutions for protein
data, which take the device route.

Figure and bound: max_ij |F_dev - F_host| / max_ij |F_host| <= 1e-11 per problem.  Both routes run the
same recurrences with the same number of squarings and differ only in the order inside dot products of
length 20; a NumPy restatement with two other orders put that difference at 1.2e-14 for rho tau <= 10,
8e-14 at rho tau = 100 and 3.1e-13 at rho tau = 400 (squaring amplifies it), and 1e-11 is this
project's bound for a device result against its restatement.  Every comparison prints its worst
figure.  Measured worst of the module: 7.2e-14 (one operation, R 4, two rate matrices: the length 100
at the top gamma rate); the largest call, 1040 problems, 1.7e-14.

A call's problem count is n_ops x 2 x R, so it is even; n_ops takes 1, 3, 4, 5 and 65 and R 1, 4 and 8
(2 .. 1040 problems: fewer than, equal to and more than a few waves, and many workgroups).  The lengths
0, 1e-6, 0.1, 1 and 100 alternate over the branches of one call, so waves with 0 to 13 and more
squarings run side by side.  Q is UNREST from 380 random rates of which some are 0; with two rate
matrices params_indices is [0, 1, 1, 0]; N spans 1e-12 .. 1e3 and every other problem has whole rows and
columns of zeros."""
import numpy as np
import pytest

import root_digger_amd as rd
import brlen_ref
import grad_ref
import subst_ref
import util
from test_gpu_ancestral import traverse
from test_gpu_brlen import TOL
from test_gpu_k20_brlen import protein_workload  # noqa: F401  (fixture)
from test_gpu_k20_pair_sums import protein_model

pytestmark = pytest.mark.gpu

BOUND = 1e-11
LENGTHS = (0.0, 1e-6, 0.1, 1.0, 100.0)
WORST = [0.0]
HOST = {}


def problems(n_ops, R, sets):
    """pair sums, lengths, rate-matrix sets, indices and rates of one call, and the host route's adjoints (made once)"""
    key = (n_ops, R, sets)
    if key not in HOST:
        rng = np.random.default_rng(100 * n_ops + 10 * R + sets)
        N = 10.0 ** rng.uniform(-12, 3, (n_ops, 2, R, 20, 20))
        flat = N.reshape(-1, 20, 20)
        flat[1::2, [3, 17], :] = 0.0   # whole rows and columns of zeros in every other problem
        flat[1::2, :, [0, 11]] = 0.0
        lengths = np.array([LENGTHS[(i + R) % 5] for i in range(2 * n_ops)]).reshape(n_ops, 2)
        subst = rng.uniform(0.1, 1.5, (sets, 380))
        subst[rng.random((sets, 380)) < 0.1] = 0.0
        assert (subst == 0).sum() >= 10
        freqs = rng.dirichlet(np.ones(20) * 4, sets)
        pidx = ([0, 1, 1, 0] * 2)[:R] if sets == 2 else [0] * R
        rates = np.array(rd.compute_gamma_cats(0.7, R)) if R > 1 else np.ones(1)
        args = (N, lengths, subst, freqs, pidx, rates)
        host = rd.pair_sum_adjoints(*args, where="host")
        for v in (N, lengths, subst, freqs, rates, host):
            v.setflags(write=False)
        HOST[key] = args, host
    return HOST[key]


def worst_of(dev, host):
    """the largest max|F_dev - F_host| / max|F_host| over the problems; a problem whose host result is 0 must be 0"""
    d, h = dev.reshape(-1, 400), host.reshape(-1, 400)
    scale = np.abs(h).max(axis=1)
    assert np.all(d[scale == 0] == 0)
    return float((np.abs(d - h).max(axis=1)[scale > 0] / scale[scale > 0]).max())


@pytest.mark.parametrize("n_ops,R,sets", [(n, R, sets) for n in (1, 3, 4, 5, 65) for R, sets in ((1, 1), (4, 2), (8, 1))]
                         + [(4, 4, 1), (3, 8, 2)])
def test_device_route_against_host_route(n_ops, R, sets):
    args, host = problems(n_ops, R, sets)
    before = [np.array(v, copy=True) for v in args]
    dev = rd.pair_sum_adjoints(*args, where="device")
    assert rd.pair_sum_adjoints_last_ms() > 0
    assert dev.shape == host.shape and np.all(np.isfinite(dev))
    worst = worst_of(dev, host)
    WORST[0] = max(WORST[0], worst)
    print("%d ops, R %d, %d rate matrices (%d problems): largest max|F_dev - F_host| / max|F_host| %.3e; worst so far %.3e" % (
        n_ops, R, sets, n_ops * 2 * R, worst, WORST[0]))
    assert worst <= BOUND
    assert dev.min() >= 0 and dev.max() > 0
    zero = args[1] == 0.0   # tau = 0: F = N exactly, on the device too
    assert dev[zero].tobytes() == np.ascontiguousarray(args[0][zero]).tobytes()
    # two calls, equal bytes; auto is the device route here; the inputs are only read
    assert rd.pair_sum_adjoints(*args, where="device").tobytes() == dev.tobytes()
    assert rd.pair_sum_adjoints(*args).tobytes() == dev.tobytes() and rd.pair_sum_adjoints_last_ms() > 0
    assert all(np.array_equal(a, b) for a, b in zip(before, args))
    # N = 0 gives 0 exactly
    assert np.all(rd.pair_sum_adjoints(np.zeros_like(args[0]), *args[1:], where="device") == 0.0)


def test_a_problem_depends_on_its_own_inputs_alone():
    """the same problem alone, and as one of 1040 in another place, has the same bits"""
    args, _ = problems(65, 8, 1)
    N, lengths, subst, freqs, pidx, rates = args
    dev = rd.pair_sum_adjoints(*args, where="device")
    for k in (0, 37, 64):
        alone = rd.pair_sum_adjoints(N[k:k + 1], lengths[k:k + 1], subst, freqs, pidx, rates, where="device")
        assert alone.tobytes() == np.ascontiguousarray(dev[k:k + 1]).tobytes()


def test_refusals_leave_no_time_and_a_usable_library():
    args, host = problems(3, 4, 2)
    rd.pair_sum_adjoints(*args, where="device")
    assert rd.pair_sum_adjoints_last_ms() > 0
    small = np.ones((3, 2, 4, 4, 4))
    with pytest.raises(rd.RdamdError, match="20 states, not 4"):
        rd.pair_sum_adjoints(small, args[1], np.ones((2, 12)), np.full((2, 4), 0.25), args[4], args[5], where="device")
    assert rd.lib.rdamd_errno() == 63 and rd.pair_sum_adjoints_last_ms() == 0
    with pytest.raises(rd.RdamdError, match="index out of range"):
        rd.pair_sum_adjoints(args[0], args[1], args[2], args[3], [0, 2, 1, 0], args[5], where="device")
    assert rd.lib.rdamd_errno() == 7 and rd.pair_sum_adjoints_last_ms() == 0
    assert worst_of(rd.pair_sum_adjoints(*args, where="device"), host) <= BOUND and rd.pair_sum_adjoints_last_ms() > 0


# ---- the model ------------------------------------------------------------------------------
def model_partition(wl, cmap, pp, rl):
    """a partition set up as the model sets its own, traversed at rl: the device's pair sums"""
    t2 = rd.Tree.from_newick(wl["newick"])
    f = np.asarray(pp["freqs"], dtype=np.float64)
    f = f / f.sum()
    rates = np.array(rd.compute_gamma_cats(pp["gamma_alpha"][0], 4, rd.GAMMA_RATES_MEDIAN))
    w = np.full(4, 0.25)
    p = rd.Partition.for_tree(t2, 20, len(next(iter(wl["seqs"].values()))), 4, rd.ATTRIB_NONREV)
    util.load_tips(p, t2, wl["seqs"], cmap)
    p.set_subst_params(0, pp["subst_rates"])
    p.set_frequencies(0, f)
    p.set_category_rates(rates)
    p.set_category_weights(w)
    sched = t2.generate_operations(rl)
    N, M, W = p.pair_sums(traverse(p, t2, rl))
    return (N, M, W), grad_ref.branch_lengths(*sched), f, rates, w


def test_model_gradient_protein_takes_the_device_route(protein_workload):
    wl, cmap, pp = protein_workload
    tree, m = protein_model(wl, cmap)
    rl = tree.root_location(3).with_ratio(0.27)
    grad, _ = m.gradient(rl, [pp])
    assert rd.pair_sum_adjoints_last_ms() > 0   # (this thread's last call: the model's)
    (N, M, W), lengths, f, rates, w = model_partition(wl, cmap, pp, rl)
    (d_subst, d_pi, d_rho, _), (c_subst, c_pi, c_rho, _) = grad_ref.gradient(
        N, M, W, lengths, [np.array(pp["subst_rates"])], [f], [0] * 4, [0] * 4, rates, w)
    err = np.abs(grad[0]["subst_rates"] - d_subst[0]) / c_subst[0]
    print("protein model, device adjoints: subst rates, largest |g - g_ref| / C %.3e" % err.max())
    assert np.all(np.abs(grad[0]["subst_rates"] - d_subst[0]) <= 10 * TOL * c_subst[0])   # test_gpu_k20_pair_sums.py's bound
    # pi = x / sum x: g_x = (g_pi - pi . g_pi) / sum x, and its companion likewise
    xsum = float(np.sum(pp["freqs"]))
    want = (d_pi[0] - f @ d_pi[0]) / xsum
    comp = (c_pi[0] + f @ c_pi[0]) / xsum
    print("protein model, device adjoints: freqs, largest |g - g_ref| / C %.3e" % (np.abs(grad[0]["freqs"] - want) / comp).max())
    assert np.all(np.abs(grad[0]["freqs"] - want) <= 10 * TOL * comp)
    # the category rates (the path to alpha: d_rates += tau <F, Q>), from the device adjoints of the same sums
    F = rd.pair_sum_adjoints(N, lengths, [pp["subst_rates"]], [f], [0] * 4, rates, where="device")
    g = rd.gradient_from_adjoints(F, M, W, lengths, [pp["subst_rates"]], [f], [0] * 4, [0] * 4, rates, w)
    print("protein model, device adjoints: category rates, largest |g - g_ref| / C %.3e" % (np.abs(g[2] - d_rho) / c_rho).max())
    assert np.all(np.abs(g[2] - d_rho) <= 10 * TOL * c_rho)


def test_model_substitutions_protein_takes_the_device_route(protein_workload):
    wl, cmap, pp = protein_workload
    tree, m = protein_model(wl, cmap)
    rl = tree.root_location(3).with_ratio(0.27)
    out = m.substitutions(rl, [pp], per_site=False)
    assert rd.pair_sum_adjoints_last_ms() > 0
    typed, lengths = out["typed"][0], out["lengths"]
    (N, _, _), _, f, rates, _ = model_partition(wl, cmap, pp, rl)
    q = brlen_ref.build_q(pp["subst_rates"], f)
    ref_typed, comp, _, _ = subst_ref.typed_counts(N, lengths, [q] * 4, rates)
    print("protein model, device adjoints: typed counts, largest |x - x_ref| / companion %.3e" % (
        np.abs(typed - ref_typed) / np.where(comp > 0, comp, 1.0)).max())
    assert np.all(np.abs(typed - ref_typed) <= 1e-11 * comp)
    total = float(m.site_patterns()[0].sum())
    dwell = np.trace(typed, axis1=2, axis2=3)
    print("protein model, device adjoints: identity D %.3e" % (np.abs(dwell - lengths * total) / (lengths * total)).max())
    assert np.all(np.abs(dwell - lengths * total) <= 1e-11 * lengths * total)   # D: trace(typed) = tau sum weights
