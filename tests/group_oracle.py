"""PERMANOVA and ANOSIM with every operation order fixed (test helper, numpy
only).

This file is the specification the GPU kernels (rna_clique_amd/csrc/groups.hip)
and the host route (rna_clique_amd.groups.group_test_host) are compared
against bit for bit. Float64 throughout.

Input: D[N][N], of which only i < j is read (mirrored, zero diagonal); labels
g[i] in 0..a-1 with no group empty, 2 <= a < N; P permuted label vectors, each
a rearrangement of g. M = N (N - 1) / 2 pairs, n_g = size of group g,
m_W = sum of n_g (n_g - 1) / 2.

 1. v[i][j] = D[i][j] * D[i][j] (PERMANOVA), or twice the average rank of
    D[i][j] among the M distances, 2 #{d < D[i][j]} + #{d == D[i][j]} + 1, an
    integer (ANOSIM).
 2. For a label vector g: t[i] = the sum over j = 0, 1, ..., N - 1, added left
    to right, of (v[j][i] if g[j] == g[i] else 0); the diagonal is 0.
 3. x[i] = t[i] / (2.0 * n_g[i]) (PERMANOVA), x[i] = t[i] (ANOSIM).
 4. S(g) = x padded with zeros to the next power of two w >= N, then halved
    until one value is left: x = x[0:h] + x[h:2h] for h = w / 2, w / 4, ..., 1.
    S(g) depends only on the partition g describes.
 5. PERMANOVA: SS_W = S(g); SS_T = S(one group of everything), that is
    x[i] = t[i] / (2.0 * N) over whole rows; SS_A = SS_T - SS_W;
    F = (SS_A / (a - 1)) / (SS_W / (N - a)).
    ANOSIM: W2 = S(g) / 2 (an integer); r_W = W2 / (2 m_W);
    r_B = (M (M + 1) - W2) / (2 (M - m_W)); R = (r_B - r_W) / (M / 2).
 6. n_ge = the number of permutations with F_perm >= F_observed (false when
    either is NaN), or with W2_perm <= W2_observed.
A matrix with a non-finite entry above its diagonal is invalid: statistic,
total, within and the permutations' statistics NaN, n_ge 0, valid 0.
"""
from __future__ import annotations

import numpy as np

NAN = np.float64(np.nan)


def halving_sum(x):
    """Step 4 along the last axis."""
    x = np.asarray(x)
    n = x.shape[-1]
    w = 1
    while w < n:
        w *= 2
    y = np.zeros(x.shape[:-1] + (w,), dtype=x.dtype)
    y[..., :n] = x
    while w > 1:
        w //= 2
        y = y[..., :w] + y[..., w:2 * w]
    return y[..., 0]


def mirrored(D):
    U = np.triu(np.asarray(D, dtype=np.float64), 1)
    return U + U.T


def is_valid(D):
    D = np.asarray(D, dtype=np.float64)
    return bool(np.isfinite(D[np.triu_indices(len(D), 1)]).all())


_RANKS = {}   # the last few matrices' ranks: a test asks for the same matrix under many labellings


def twice_ranks(D):
    """Step 1 of ANOSIM by counting: an int64 (N, N) matrix, zero diagonal."""
    D = np.asarray(D, dtype=np.float64)
    n = len(D)
    iu = np.triu_indices(n, 1)
    d = D[iu]
    key = d.tobytes()
    if key not in _RANKS:
        r2 = np.zeros(len(d), dtype=np.int64)
        for k0 in range(0, len(d), 512):
            dk = d[k0:k0 + 512, None]
            r2[k0:k0 + 512] = 2 * (d[None, :] < dk).sum(axis=1) + (d[None, :] == dk).sum(axis=1) + 1
        if len(_RANKS) >= 16:
            _RANKS.clear()
        _RANKS[key] = r2
    out = np.zeros((n, n), dtype=np.int64)
    out[iu] = _RANKS[key]
    return out + out.T


def row_sums(V, G):
    """Step 2 for every row of G (K, N): t (K, N)."""
    G = np.asarray(G)
    same = G[:, :, None] == G[:, None, :]              # [k, j, i]
    return np.cumsum(np.where(same, V[None], V.dtype.type(0)), axis=1)[:, -1, :]


def group_sizes(labels):
    return np.bincount(np.asarray(labels))


def check(labels, perm_labels, n):
    labels = np.asarray(labels, dtype=np.int64)
    sizes = group_sizes(labels)
    a = len(sizes)
    assert len(labels) == n and labels.min() >= 0 and (sizes > 0).all() and 2 <= a < n
    perm_labels = np.asarray(perm_labels, dtype=np.int64).reshape(-1, n)
    for row in perm_labels:
        assert np.array_equal(np.sort(row), np.sort(labels))
    return labels, perm_labels, sizes


def permanova(D, labels, perm_labels=()):
    """(F, n_ge, SS_T, SS_W, F of every permutation, valid) of one matrix."""
    D = np.asarray(D, dtype=np.float64)
    n = len(D)
    labels, perms, sizes = check(labels, perm_labels, n)
    P, a = len(perms), len(sizes)
    if not is_valid(D):
        return NAN, 0, NAN, NAN, np.full(P, NAN), 0
    A = mirrored(D)
    V = A * A
    with np.errstate(all="ignore"):
        sst = halving_sum(row_sums(V, np.zeros((1, n), dtype=np.int64))[0] / (2.0 * n))
        G = np.concatenate([labels[None], perms])
        ssw = np.zeros(len(G))
        for k0 in range(0, len(G), 64):
            g = G[k0:k0 + 64]
            ssw[k0:k0 + 64] = halving_sum(row_sums(V, g) / (2.0 * sizes[g]))
        F = ((sst - ssw) / np.float64(a - 1)) / (ssw / np.float64(n - a))
        n_ge = int((F[1:] >= F[0]).sum())
    return F[0], n_ge, sst, ssw[0], F[1:], 1


def anosim_r(w2, M, mw):
    w2 = np.asarray(w2, dtype=np.int64)
    rw = w2.astype(np.float64) / np.float64(2 * mw)
    rb = (M * (M + 1) - w2).astype(np.float64) / np.float64(2 * (M - mw))
    return (rb - rw) / (np.float64(M) / 2.0)


def anosim(D, labels, perm_labels=()):
    """(R, n_ge, M (M + 1), W2, R of every permutation, valid) of one matrix."""
    D = np.asarray(D, dtype=np.float64)
    n = len(D)
    labels, perms, sizes = check(labels, perm_labels, n)
    P = len(perms)
    if not is_valid(D):
        return NAN, 0, NAN, NAN, np.full(P, NAN), 0
    M = n * (n - 1) // 2
    mw = int((sizes * (sizes - 1) // 2).sum())
    V = twice_ranks(D)
    G = np.concatenate([labels[None], perms])
    w2 = np.zeros(len(G), dtype=np.int64)
    for k0 in range(0, len(G), 64):
        g = G[k0:k0 + 64]
        w2[k0:k0 + 64] = halving_sum(row_sums(V, g)) // 2
    R = anosim_r(w2, M, mw)
    n_ge = int((w2[1:] <= w2[0]).sum())
    return R[0], n_ge, np.float64(M * (M + 1)), np.float64(w2[0]), R[1:], 1


TESTS = {"permanova": permanova, "anosim": anosim}


def batch(Ds, labels, perm_labels, method):
    """The test of every matrix: (stat, n_ge, total, within, perm_stat, valid)
    arrays with a leading replicate axis."""
    n = len(labels)
    perms = np.asarray(perm_labels).reshape(-1, n)
    rows = [TESTS[method](D, labels, perms) for D in Ds]
    stat, n_ge, total, within, ps, valid = zip(*rows)
    return (np.array(stat, dtype=np.float64), np.array(n_ge, dtype=np.uint32), np.array(total, dtype=np.float64),
            np.array(within, dtype=np.float64), np.array(ps, dtype=np.float64).reshape(len(Ds), len(perms)),
            np.array(valid, dtype=np.uint8))
