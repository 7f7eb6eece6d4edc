"""NumPy restatement of the branch pair sums of include/root_digger_amd.h (rdamd_branch_pair_sums)
and of the gradient assembled from them (rdamd_gradient_from_pair_sums), shared by
test_grad_reference.py, test_param_gradient_host.py and test_gpu_pair_sums.py.

For an operation with parent u and children a, b:  t = U_u (P_b L_b),  f0 = sum_r w t.(P_a L_a),
N[k][c][r][i][j] = sum_s weight w_r t[i] L_a[j] / f0;  at the root  froot = sum_r w pi.L,
M[r][i] = sum_s weight w_r L[i] / froot,  W[r] = sum_s weight (pi.L_r) / froot.  Every inner CLV and
every outer vector is divided by its largest entry over rates and states, per site, as brlen_ref.py
does: the ratios do not change.  Every term is non-negative: a sum is its own absolute-value
companion.

The gradient:  G_Q[m] = sum over branches and the rates r of set m of rho tau F((rho tau Q_m)^T, N),
F(X, E) the top-right block of scipy.linalg.expm([[X, E], [0, X]]);  d lnL / d rho_r =
sum_branches tau <N, Q P>;  then g = <G_Q, dQ/dx> with dQ/dx written out as a matrix for every
parameter x (quotient rule on Q = raw / mu), the root term M added to the frequencies.  Next to
every g comes its companion C: the same contraction with absolute values throughout."""
import numpy as np
from scipy.linalg import expm

from brlen_ref import build_q, children_of


def pair_sums(ops, tips, tipvec, pmat, pis, w, weights, smallest=None):
    """N[len(ops)][2][R][K][K], M[R][K], W[R]: branch (k, c) above child c of the parent of ops[n-1-k].
    pmat[m]: [R][K][K]; pis[r]: the frequencies of category r; w: [R]; weights: [S].
    smallest: a list that receives the smallest non-zero entry of every inner CLV and every outer
    vector, each relative to the largest entry of its site over all rates (which is 1 here)."""
    n, R = len(ops), len(w)
    pis = np.asarray(pis, dtype=np.float64)
    w, weights = np.asarray(w, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    K = pis.shape[1]
    S = next(iter(tipvec.values())).shape[0]
    L, PL = {}, {}

    def norm(v):
        v = v / v.max(axis=(1, 2), keepdims=True)
        if smallest is not None:
            smallest.append(v[v > 0].min())
        return v

    def clv(i):
        return np.broadcast_to(tipvec[i][:, None, :], (S, R, K)) if i < tips else L[i]

    for o in ops:
        for c, m in children_of(o):
            PL[c] = np.einsum("rij,srj->sri", pmat[m], clv(c))
        L[o.parent_clv_index] = norm(PL[o.child1_clv_index] * PL[o.child2_clv_index])
    root = L[ops[-1].parent_clv_index]
    froot = np.einsum("r,ri,sri->s", w, pis, root)
    M = np.einsum("s,r,sri->ri", weights / froot, w, root)
    W = np.einsum("s,ri,sri->r", weights / froot, pis, root)
    U = {ops[-1].parent_clv_index: np.broadcast_to(pis[None, :, :], (S, R, K))}
    N = np.zeros((n, 2, R, K, K))
    for k in range(n):
        o = ops[n - 1 - k]
        up = U.pop(o.parent_clv_index)
        (a, ma), (b, mb) = children_of(o)
        for c, (child, m, sibling) in enumerate(((a, ma, b), (b, mb, a))):
            t = up * PL[sibling]
            f0 = (w * (t * PL[child]).sum(axis=2)).sum(axis=1)
            N[k, c] = np.einsum("s,r,sri,srj->rij", weights / f0, w, t, clv(child))
            if child >= tips:
                U[child] = norm(np.einsum("sri,rij->srj", t, pmat[m]))
    return N, M, W


def branch_lengths(ops, pmi, brl):
    """lengths[len(ops)][2] of branch (k, c) from the schedule of Tree.generate_operations"""
    n = len(ops)
    place = {int(m): i for i, m in enumerate(pmi)}
    return np.array([[brl[place[m]] for _, m in children_of(ops[n - 1 - k])] for k in range(n)], dtype=np.float64)


def frechet(x, e):
    """F(X, E) = integral_0^1 exp(sX) E exp((1 - s)X) ds"""
    K = x.shape[0]
    blk = np.zeros((2 * K, 2 * K))
    blk[:K, :K] = x
    blk[K:, K:] = x
    blk[:K, K:] = e
    return expm(blk)[:K, K:]


def q_parts(subst, freqs):
    """raw (zero row sums, raw_ij = s_ij pi_j) and mu = -sum pi_i raw_ii"""
    freqs = np.asarray(freqs, dtype=np.float64)
    K = freqs.size
    raw = np.zeros((K, K))
    it = iter(np.asarray(subst, dtype=np.float64))
    for i in range(K):
        for j in range(K):
            if i != j:
                raw[i, j] = next(it) * freqs[j]
        raw[i, i] = -raw[i].sum()
    return raw, -(freqs * np.diag(raw)).sum()


def q_jacobian(subst, freqs):
    """dQ/ds[K K - K][K][K] and dQ/dpi[K][K][K] of Q = raw / mu, by the quotient rule"""
    subst, freqs = np.asarray(subst, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
    K = freqs.size
    raw, mu = q_parts(subst, freqs)

    def quotient(draw):
        np.fill_diagonal(draw, 0.0)
        np.fill_diagonal(draw, -draw.sum(axis=1))
        return draw, -(freqs * np.diag(draw)).sum()

    pairs = [(i, j) for i in range(K) for j in range(K) if i != j]
    ds, dpi = np.zeros((len(pairs), K, K)), np.zeros((K, K, K))
    for e, (i, j) in enumerate(pairs):
        draw = np.zeros((K, K))
        draw[i, j] = freqs[j]
        draw, dmu = quotient(draw)
        ds[e] = draw / mu - raw * dmu / mu ** 2
    for c in range(K):
        draw = np.zeros((K, K))
        for e, (i, j) in enumerate(pairs):
            if j == c:
                draw[i, j] = subst[e]
        draw, dmu = quotient(draw)
        dmu -= raw[c, c]   # pi_c as the weight of row c in mu
        dpi[c] = draw / mu - raw * dmu / mu ** 2
    return ds, dpi


def gradient(N, M, W, lengths, subst, freqs, pidx, fidx, rates, w):
    """(d_subst[sets][K K - K], d_freqs[sets][K], d_rates[R], d_weights[R]), and the four companions in
    the same order.  subst[m], freqs[m]: the rate-matrix sets; pidx, fidx: set per category."""
    N, M = np.asarray(N, dtype=np.float64), np.asarray(M, dtype=np.float64)
    n, _, R, K, _ = N.shape
    sets = len(subst)
    rates = np.asarray(rates, dtype=np.float64)
    q = [build_q(subst[m], freqs[m]) for m in range(sets)]
    G, GA = np.zeros((sets, K, K)), np.zeros((sets, K, K))
    d_rates, c_rates = np.zeros(R), np.zeros(R)
    for k in range(n):
        for c in range(2):
            tau = lengths[k][c]
            for r in range(R):
                m = pidx[r]
                a = rates[r] * tau * q[m]
                f = rates[r] * tau * frechet(a.T, N[k, c, r])
                G[m] += f
                GA[m] += np.abs(f)
                p = expm(a)
                d_rates[r] += tau * (N[k, c, r] * (q[m] @ p)).sum()
                c_rates[r] += tau * (N[k, c, r] * (np.abs(q[m]) @ np.abs(p))).sum()
    d_subst, c_subst = np.zeros((sets, K * K - K)), np.zeros((sets, K * K - K))
    d_freqs, c_freqs = np.zeros((sets, K)), np.zeros((sets, K))
    for m in range(sets):
        ds, dpi = q_jacobian(subst[m], freqs[m])
        d_subst[m] = np.einsum("ij,eij->e", G[m], ds)
        c_subst[m] = np.einsum("ij,eij->e", GA[m], np.abs(ds))
        d_freqs[m] = np.einsum("ij,eij->e", G[m], dpi)
        c_freqs[m] = np.einsum("ij,eij->e", GA[m], np.abs(dpi))
    for r in range(R):
        d_freqs[fidx[r]] += M[r]
        c_freqs[fidx[r]] += M[r]
    W = np.asarray(W, dtype=np.float64)
    return (d_subst, d_freqs, d_rates, W.copy()), (c_subst, c_freqs, c_rates, W.copy())
