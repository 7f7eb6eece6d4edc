"""NumPy restatement of the branch-length derivatives of include/root_digger_amd.h
(rdamd_branch_derivatives), shared by test_brlen_reference.py and test_gpu_brlen.py.

For an operation with parent u and children a, b:  t = U_u (P_b L_b),  y = P_a L_a,  z = Q y,
z2 = Q z;  f0 = sum_r w t.y,  f1 = sum_r w rho t.z,  f2 = sum_r w rho^2 t.z2;
d1 = sum_s weight f1/f0,  d2 = sum_s weight (f2/f0 - (f1/f0)^2).  Every inner CLV and every outer
vector is divided by its largest entry over rates and states, per site: the ratios do not change
and trees of any depth stay in range.

Next to d1 and d2 come their absolute-value companions A1 and A2: the same sums with |Q_ij| in
place of Q_ij and |.| around each site term.  The rounding error of a device sum is bounded by a
small multiple of 2^-53 (terms per sum) A."""
import numpy as np


def build_q(subst, freqs):
    """off-diagonals row-major, Q_ij = s_ij pi_j, zero row sums, one expected substitution per
    unit time under pi (csrc/kernels_pmatrix.hip, build_q_host)"""
    freqs = np.asarray(freqs, dtype=np.float64)
    K = freqs.size
    q = np.zeros((K, K))
    it = iter(np.asarray(subst, dtype=np.float64))
    for i in range(K):
        for j in range(K):
            if i != j:
                q[i, j] = next(it) * freqs[j]
        q[i, i] = -q[i].sum()
    return q / -(freqs * np.diag(q)).sum()


def children_of(o):
    return ((o.child1_clv_index, o.child1_matrix_index), (o.child2_clv_index, o.child2_matrix_index))


def tip_vectors(tree, seqs, cmap, K):
    """clv index -> [S][K] 0/1 code vectors"""
    return {tree.tip_index(label): np.array([[(cmap[ord(ch)] >> j) & 1 for j in range(K)] for ch in seq], dtype=np.float64)
            for label, seq in seqs.items()}


def pmatrices(part, ops):
    """the partition's own P-matrices of the list, read back: exp(Qt) is not under test"""
    return {m: part.get_pmatrix(m) for o in ops for _, m in children_of(o)}


def branch_derivatives(ops, tips, tipvec, pmat, qs, pis, w, rates, weights):
    """d1, d2, A1, A2, each [len(ops)][2]: branch (k, c) above child c of the parent of ops[n-1-k].
    pmat[m]: [R][K][K]; qs[r], pis[r]: rate matrix and frequencies of category r; w, rates: [R];
    weights: [S]."""
    n, R = len(ops), len(w)
    qs, pis = np.asarray(qs, dtype=np.float64), np.asarray(pis, dtype=np.float64)
    w, rates, weights = (np.asarray(v, dtype=np.float64) for v in (w, rates, weights))
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
    out = np.zeros((4, n, 2))
    qa = np.abs(qs)
    for k in range(n):
        o = ops[n - 1 - k]
        up = U.pop(o.parent_clv_index)
        (a, ma), (b, mb) = children_of(o)
        for c, (child, m, sibling) in enumerate(((a, ma, b), (b, mb, a))):
            t, y = up * PL[sibling], PL[child]

            def sums(q):
                z = np.einsum("rij,srj->sri", q, y)
                z2 = np.einsum("rij,srj->sri", q, z)
                return ((w * rates * (t * z).sum(axis=2)).sum(axis=1), (w * rates ** 2 * (t * z2).sum(axis=2)).sum(axis=1))

            f0 = (w * (t * y).sum(axis=2)).sum(axis=1)
            f1, f2 = sums(qs)
            a1, a2 = sums(qa)
            out[0, k, c] = (weights * (f1 / f0)).sum()
            out[1, k, c] = (weights * (f2 / f0 - (f1 / f0) ** 2)).sum()
            out[2, k, c] = (weights * np.abs(a1 / f0)).sum()
            out[3, k, c] = (weights * np.abs(a2 / f0 - (a1 / f0) ** 2)).sum()
            if child >= tips:
                U[child] = norm(np.einsum("sri,rij->srj", t, pmat[m]))
    return out[0], out[1], out[2], out[3]


def predicted_gain(x, g, h, lo, hi):
    """the optimiser's stopping quantity (csrc/brlen_opt.hpp): sum over free b of g_b^2 / (2 c_b)"""
    x, g, h = (np.asarray(v, dtype=np.float64).ravel() for v in (x, g, h))
    free = ~(((x <= lo) & (g <= 0)) | ((x >= hi) & (g >= 0)))
    c = np.where(h < 0, -h, np.abs(g) / np.maximum(x, lo))
    c = np.where(c > 0, c, 1.0)
    return float((g[free] ** 2 / (2 * c[free])).sum())
