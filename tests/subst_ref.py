"""NumPy/SciPy restatement of the substitution mapping of include/root_digger_amd.h
(rdamd_branch_substitutions, rdamd_substitution_counts_from_pair_sums), shared by
test_subst_reference.py, test_subst_host.py, test_gpu_subst.py and test_gpu_subst_cli.py.

For an operation with parent u and children a, b, branch (k, c) above a with length tau, and rate
category r with X = rho tau Q, P = exp(X):  t = U_u (P_b L_b),  f0 = sum_r w t.(P L_a),
  J[s][i][j] = sum_r w t[i] P[i][j] L_a[j] / f0        change = sum_{i != j} J
  n[s]       = sum_r w t^T C L_a / f0                  C = F(X, offdiag(X))
and from the pair sums N of grad_ref.pair_sums, with F_r = F(X^T, N[k][c][r]),
  E[i][j] = sum_r X[i][j] F_r[i][j]  (i != j)          D[i] = tau sum_r F_r[i][i].
Every inner CLV and every outer vector is divided by its largest entry over rates and states, per
site, as brlen_ref.py does: the ratios do not change.  F(X, E) is the top-right block of
scipy.linalg.expm([[X, E], [0, X]]) (grad_ref.frechet) throughout; the adjoint shortcut is not used.

Every term of J, n, E and D is non-negative: exp(xX) of a rate matrix has no negative entry, nor
have offdiag(X), N, t and L.  A sum is therefore its own absolute-value companion ("the same sum
with |X| and |N|"), and the companions returned here are computed as such: with |X[i][j]| as the
factor and |N| inside F."""
import numpy as np
from scipy.linalg import expm

from brlen_ref import children_of
import grad_ref


def count_matrix(x):
    """C = F(X, offdiag(X))"""
    e = x.copy()
    np.fill_diagonal(e, 0.0)
    return grad_ref.frechet(x, e)


def count_matrices(lengths, qs, rates):
    """C[n][2][R][K][K]; qs[r]: the rate matrix of category r"""
    lengths = np.asarray(lengths, dtype=np.float64)
    return np.array([[[count_matrix(rates[r] * lengths[k, c] * qs[r]) for r in range(len(rates))] for c in range(2)]
                     for k in range(lengths.shape[0])])


def site_maps(ops, tips, tipvec, pmat, cmat, pis, w):
    """J[len(ops)][2][S][K][K] and n[len(ops)][2][S]: branch (k, c) above child c of the parent of
    ops[n-1-k].  pmat[m]: [R][K][K]; cmat[k][c]: [R][K][K]; pis[r]: the frequencies of category r."""
    n, R = len(ops), len(w)
    pis, w = np.asarray(pis, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K = pis.shape[1]
    S = next(iter(tipvec.values())).shape[0]
    L, PL = {}, {}

    def norm(v):
        return v / v.max(axis=(1, 2), keepdims=True)

    def clv(i):
        return np.broadcast_to(tipvec[i][:, None, :], (S, R, K)) if i < tips else L[i]

    for o in ops:
        for c, m in children_of(o):
            PL[c] = np.einsum("rij,srj->sri", pmat[m], clv(c))
        L[o.parent_clv_index] = norm(PL[o.child1_clv_index] * PL[o.child2_clv_index])
    U = {ops[-1].parent_clv_index: np.broadcast_to(pis[None, :, :], (S, R, K))}
    J, cnt = np.zeros((n, 2, S, K, K)), np.zeros((n, 2, S))
    for k in range(n):
        o = ops[n - 1 - k]
        up = U.pop(o.parent_clv_index)
        (a, ma), (b, mb) = children_of(o)
        for c, (child, m, sibling) in enumerate(((a, ma, b), (b, mb, a))):
            t = up * PL[sibling]
            f0 = (w * (t * PL[child]).sum(axis=2)).sum(axis=1)
            J[k, c] = np.einsum("r,sri,rij,srj->sij", w, t, pmat[m], clv(child)) / f0[:, None, None]
            cnt[k, c] = np.einsum("r,sri,rij,srj->s", w, t, cmat[k][c], clv(child)) / f0
            if child >= tips:
                U[child] = norm(np.einsum("sri,rij->srj", t, pmat[m]))
    return J, cnt


def summaries(J):
    """change[...], top_pair[...] (code i K + j, the smallest at a tie), top_prob[...] and gap[...], the
    distance from the best to the second-best pair i != j, from J[..., K, K]"""
    K = J.shape[-1]
    off = np.array([i * K + j for i in range(K) for j in range(K) if i != j])
    flat = J.reshape(J.shape[:-2] + (K * K,))[..., off]
    order = np.sort(flat, axis=-1)
    best = np.argmax(flat, axis=-1)   # (the first maximum: the smallest code)
    gap = order[..., -1] - order[..., -2] if off.size > 1 else np.full(flat.shape[:-1], np.inf)
    return flat.sum(axis=-1), off[best].astype(np.uint8), order[..., -1], gap


def typed_counts(N, lengths, qs, rates):
    """typed[n][2][K][K] (E off the diagonal, D on it), its companion, and diag[n][2] =
    sum_r sum_i X[i][i] F_r[i][i] (identity C) with the companion of that sum.  qs[r]: the rate matrix
    of category r."""
    N = np.asarray(N, dtype=np.float64)
    n, _, R, K, _ = N.shape
    typed, comp = np.zeros((n, 2, K, K)), np.zeros((n, 2, K, K))
    diag, diag_comp = np.zeros((n, 2)), np.zeros((n, 2))
    eye = np.eye(K, dtype=bool)
    for k in range(n):
        for c in range(2):
            tau = lengths[k][c]
            for r in range(R):
                x = rates[r] * tau * qs[r]
                f = grad_ref.frechet(x.T, N[k, c, r])
                fa = grad_ref.frechet(x.T, np.abs(N[k, c, r]))
                typed[k, c] += np.where(eye, tau * f, x * f)
                comp[k, c] += np.where(eye, tau * fa, np.abs(x) * fa)
                diag[k, c] += (np.diag(x) * np.diag(f)).sum()
                diag_comp[k, c] += (np.abs(np.diag(x)) * np.diag(fa)).sum()
    return typed, comp, diag, diag_comp


def site_likelihoods(ops, tips, tipvec, pmat, pis, w):
    """f[S] = sum_r w pi . L_root without any renormalisation (small trees only)"""
    R = len(w)
    pis, w = np.asarray(pis, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K = pis.shape[1]
    S = next(iter(tipvec.values())).shape[0]
    L = {}

    def clv(i):
        return np.broadcast_to(tipvec[i][:, None, :], (S, R, K)) if i < tips else L[i]

    for o in ops:
        (a, ma), (b, mb) = children_of(o)
        L[o.parent_clv_index] = (np.einsum("rij,srj->sri", pmat[ma], clv(a)) * np.einsum("rij,srj->sri", pmat[mb], clv(b)))
    return np.einsum("r,ri,sri->s", w, pis, L[ops[-1].parent_clv_index])


def pmatrices_from_q(pmi, brl, qs, rates):
    """{matrix index: [R][K][K]} = expm(rho_r t Q_r)"""
    return {int(m): np.array([expm(qs[r] * rates[r] * t) for r in range(len(rates))]) for m, t in zip(pmi, brl)}
