"""Shared helpers for the parity tests: fixture readers, model set-up and the
compute_lh / compute_lh_root call sequences of the reference
(src/model.cpp:384-452) expressed over the partition API, so the same code
drives the oracle and the HIP library."""
import ctypes as C
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(GOLD, "data")


def golden(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path):
        line = line.strip()
        if not line:
            continue
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = ""
        else:
            seqs[name] += line
    return seqs


def read_phylip(path):
    toks = open(path).read().split()
    n, length = int(toks[0]), int(toks[1])
    seqs, i = {}, 2
    for _ in range(n):
        name = toks[i]
        i += 1
        s = ""
        while len(s) < length:
            s += toks[i]
            i += 1
        seqs[name] = s
    return seqs


def compress(seqs):
    """site-pattern compression -> (compressed seqs, weights); order = first seen."""
    names = list(seqs)
    cols = {}
    order = []
    n = len(seqs[names[0]])
    for s in range(n):
        col = "".join(seqs[k][s] for k in names)
        if col not in cols:
            cols[col] = 0
            order.append(col)
        cols[col] += 1
    out = {k: "".join(col[i] for col in order) for i, k in enumerate(names)}
    return out, np.array([cols[c] for c in order], dtype=np.uint32)


def make_map(alphabet, extra=None):
    m = (C.c_uint64 * 256)()
    for i, ch in enumerate(alphabet):
        m[ord(ch)] = 1 << i
    for ch, v in (extra or {}).items():
        m[ord(ch)] = v
    return m


def load_tips(part, tree, seqs, cmap, weights=None):
    """model_t::set_tip_states (src/model.cpp:302-325)."""
    for label, seq in seqs.items():
        idx = tree.tip_index(label)
        assert idx >= 0, label
        part.set_tip_states(idx, cmap, seq)
    if weights is not None:
        part.set_pattern_weights(weights)


def compute_lh(part, tree, rl):
    """model_t::compute_lh (src/model.cpp:384-413) for one partition."""
    ops, pmi, brl = tree.generate_operations(rl)
    part.update_prob_matrices(pmi, brl)
    part.update_clvs(ops)
    return part.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())


def compute_lh_root(part, tree, rl):
    """model_t::compute_lh_root (src/model.cpp:415-452)."""
    op, pmi, brl = tree.generate_derivative_operations(rl)
    part.update_prob_matrices(pmi, brl)
    part.update_clvs([op])
    return part.compute_root_loglikelihood(tree.root_clv_index(), tree.root_scaler_index())


def move_root(part, tree, rl):
    """model_t::move_root (src/model.cpp:823-854)."""
    ops, pmi, brl = tree.generate_root_update_operations(rl)
    if len(ops) == 0:
        return
    part.update_prob_matrices(pmi, brl)
    part.update_clvs(ops)


def find_root(tree, near_tips, far_tips, alpha):
    """Root location whose branch splits the tips as the golden entry says;
    alpha is re-expressed relative to the side rl.edge names."""
    near, far = sorted(near_tips), sorted(far_tips)
    for rl in tree.roots():
        side = sorted(tree.side_tips(rl))
        if side == near:
            return rl.with_ratio(alpha)
        if side == far:
            return rl.with_ratio(1.0 - alpha)
    raise KeyError("no root location matches the golden split")


def odd_cells(rng, seqs, odd, share=0.2):
    """the same sequences with about `share` of the cells replaced by a character of `odd` (gaps,
    ambiguity codes); no column ends up without a single plain character"""
    names = list(seqs)
    cells = np.array([list(seqs[k]) for k in names])
    hit = rng.random(cells.shape) < share
    hit[rng.integers(len(names), size=cells.shape[1]), np.arange(cells.shape[1])] = False
    cells[hit] = rng.choice(list(odd), size=int(hit.sum()))
    return {k: "".join(row) for k, row in zip(names, cells)}


def mixture_params(rng, states, rate_matrices):
    """`rate_matrices` independent (subst, freqs) draws, each as synth.workload draws its one set:
    exchange rates U(1e-4, 1) (the reference's random_params), frequencies Dirichlet(10, ..., 10)"""
    subst = [rng.uniform(1e-4, 1.0, states * states - states) for _ in range(rate_matrices)]
    freqs = [rng.dirichlet(np.ones(states) * 10) for _ in range(rate_matrices)]
    return subst, freqs


def set_mixture(parts, subst, freqs, rates, weights):
    """parameter set m of every partition := (subst[m], freqs[m]); the categories' rates and weights"""
    for p in parts:
        for m, (s, f) in enumerate(zip(subst, freqs)):
            p.set_subst_params(m, s)
            p.set_frequencies(m, f)
        p.set_category_rates(rates)
        p.set_category_weights(weights)


def restated_pmatrices(subst, freqs, pidx, rates, lengths):
    """[branch][category][K][K]: Q per rate matrix as synth.build_q builds it, scipy.linalg.expm per
    (branch, category)"""
    from scipy.linalg import expm
    from root_digger_amd import synth
    q = [synth.build_q(s, f) for s, f in zip(subst, freqs)]
    return np.array([[expm(q[pidx[r]] * rates[r] * t) for r in range(len(rates))] for t in lengths])


def restated_site_lnls(tree, ops, pmat_of, seqs, cmap, K, freqs, fidx, cat_weights, pattern_weights):
    """plain Felsenstein pruning per category in NumPy, no rescaling.
    pmat_of: matrix index -> [R][K][K].  -> per-site lnL (pattern weight applied)"""
    S, R = len(next(iter(seqs.values()))), len(cat_weights)
    clv = {}
    for label, seq in seqs.items():
        bits = np.array([[(cmap[ord(ch)] >> j) & 1 for j in range(K)] for ch in seq], dtype=np.float64)
        clv[tree.tip_index(label)] = np.broadcast_to(bits[:, None, :], (S, R, K))
    for op in ops:
        a = np.einsum("rij,srj->sri", pmat_of[op.child1_matrix_index], clv[op.child1_clv_index])
        b = np.einsum("rij,srj->sri", pmat_of[op.child2_matrix_index], clv[op.child2_clv_index])
        clv[op.parent_clv_index] = a * b
    root = clv[ops[len(ops) - 1].parent_clv_index]
    site = np.zeros(S)
    for r in range(R):
        site += cat_weights[r] * root[:, r, :] @ np.asarray(freqs[fidx[r]])
    return pattern_weights * np.log(site)


# ---- alignments that fill a partition's table of state masks (64 entries outside DNA) -----------
PRINTABLE = "".join(chr(c) for c in range(33, 127))
CODE_TABLE = 64


def full_table_map(rng, K, plain=None):
    """-> (plain characters, odd characters, map): a map of min(64, 2^K - 1) distinct masks.
    The plain states first -- all K of them up to 48 states, beyond that 48 of them, states 0 and K - 1
    among them, because the table has to keep room for masks of several states --, then the all-ones
    mask, two pairs with state K - 1, and random subsets of 2 .. K - 1 states of which
    about every second one is given state K - 1.  `plain`: the plain states' characters (default: the first
    printable ones)."""
    total = min(CODE_TABLE, 2 ** K - 1)
    if plain is None:
        plain = PRINTABLE[:K]
    assert len(plain) == K and len(set(plain)) == K
    keep = list(range(K)) if K <= 48 else [0, K - 1] + sorted(int(j) for j in rng.choice(np.arange(1, K - 1), 46, replace=False))
    used = "".join(plain[j] for j in keep)
    top = 1 << (K - 1)
    masks = [(1 << K) - 1]
    if K > 2:
        masks += [top | 1, top | 2 if K > 3 else 3]
    seen = {1 << j for j in range(K)} | set(masks)
    assert len(seen) == K + len(masks)
    while len(used) + len(masks) < total:
        size = int(rng.integers(2, K)) if len(masks) % 3 else int(rng.integers(max(2, K // 2), K))
        m = sum(1 << int(j) for j in rng.choice(K, size, replace=False))
        if rng.random() < 0.5:
            m |= top
        if m not in seen:
            seen.add(m)
            masks.append(m)
    odd = "".join(ch for ch in PRINTABLE if ch not in plain)[:len(masks)]
    assert len(odd) == len(masks)
    return used, odd, make_map(plain, dict(zip(odd, masks)))


def place_characters(rng, seqs, plain, odd, pair, late):
    """the same sequences with every character of `plain` and of `odd` in them: the last `late` odd
    characters stand in the two tips of `pair` only, at the same sites of both (one step to the
    right in the second), the others are dealt out over the other tips.  -> sequences with the
    pair's tips LAST, so that a partition that numbers masks as it meets them gives the late
    characters its highest codes."""
    names = [k for k in seqs if k not in pair] + list(pair)
    cells = np.array([list(seqs[k]) for k in names])
    n, S = cells.shape
    early, tail = odd[:len(odd) - late], odd[len(odd) - late:]
    free = [(i, s) for i in range(n - 2) for s in range(S)]
    assert len(plain) + len(early) <= len(free) and 0 < late <= S
    for row in range(n):       # odd characters that the caller's random cells put where they may not stand
        for s in range(S):
            if cells[row, s] in (tail if row < n - 2 else odd):
                cells[row, s] = plain[(row + s) % len(plain)]
    picks = rng.permutation(len(free))
    for ch, k in zip(plain + early, picks):
        cells[free[k]] = ch
    for s in range(late):
        cells[n - 2, s] = tail[s]
        cells[n - 1, s] = tail[(s + 1) % late]
    return {k: "".join(row) for k, row in zip(names, cells)}


def tip_codes(seqs, cmap):
    """the code every cell gets in a non-DNA partition that is given `seqs` in this order: masks are
    numbered as they are met.  -> ({label: codes}, the masks in code order)"""
    table, out = [], {}
    for label, seq in seqs.items():
        row = []
        for ch in seq:
            m = int(cmap[ord(ch)])
            if m not in table:
                table.append(m)
            row.append(table.index(m))
        out[label] = np.array(row)
    return out, table


def tip_tip_pair(tree, ops):
    """labels of the two tips of the first operation over two tips"""
    for op in ops:
        if op.child1_clv_index < tree.tip_count() and op.child2_clv_index < tree.tip_count():
            return tree.tip_label(op.child1_clv_index), tree.tip_label(op.child2_clv_index)
    raise KeyError("no operation over two tips")


def balanced_newick(n_tips, rng):
    """a perfectly balanced unrooted tree over t0 .. t<n_tips - 1> (3 x 2^k tips, or 2^k: the top
    node then joins one half and two quarters), random branch lengths: the deepest evaluator stacks
    a tree of its size can ask for"""
    nodes = ["t%d:%.5f" % (i, rng.uniform(0.02, 0.3)) for i in range(n_tips)]
    while len(nodes) > 3:
        pairs = 1 if len(nodes) == 4 else len(nodes) // 2
        nodes = ["(%s,%s):%.5f" % (nodes[2 * i], nodes[2 * i + 1], rng.uniform(0.02, 0.3))
                 for i in range(pairs)] + nodes[2 * pairs:]
    return "(" + ",".join(nodes) + ");"


def rel_err(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)
