"""The Mantel test with every operation order fixed (test helper, numpy only).

This file is the specification the GPU kernel (rna_clique_amd/csrc/mantel.hip)
and the host route (rna_clique_amd.mantel.mantel_host) are compared against bit
for bit.

Input: X[N][N] and Y[N][N], of which only i < j is read (mirrored, zero
diagonal), N >= 3; P permutations of 0..N-1. M = N (N - 1) / 2. Permutation p
rearranges X's rows and columns together: r(p) = corr(X[p(i)][p(j)], Y[i][j])
over i < j, and the identity gives the observed r. Every sum below runs over
j = 0, 1, ..., N - 1, added left to right from zero; H is the halving sum of
tests/group_oracle.py.

pearson (float64):
 1. rs[i] = sum of X[j][i]; mx = H(rs) / (N (N - 1)).
 2. xc[i][j] = X[i][j] - mx for i != j, 0 on the diagonal.
 3. q[i] = sum of xc[j][i] * xc[j][i]; sxx = H(q). yc and syy from Y likewise.
 4. c[i] = sum of xc[p(j)][p(i)] * yc[j][i]; C(p) = H(c).
 5. r(p) = C(p) / sqrt(sxx * syy): exactly 1 for Y = X, as sqrt(s * s) is s.
 6. If every entry above X's diagonal equals X[0][1], or Y's likewise, there is
    no correlation: r is NaN for every permutation.
 7. n_ge, n_le, n_abs_ge = the permutations with r(p) >= r_obs, r(p) <= r_obs,
    |r(p)| >= |r_obs|, on r as computed (false when NaN).
spearman (integers, exact in any order):
 1. a, b = the twice-ranks of X and Y (group_oracle.twice_ranks).
 2. Sab(p) = the sum over i < j of a[p(i)][p(j)] * b[i][j]; Sa, Sb, Saa, Sbb the
    sums of a, b, a^2, b^2 over i < j (a permutation does not change them).
 3. num(p) = M Sab(p) - Sa Sb; vx = M Saa - Sa^2; vy = M Sbb - Sb^2 (int64).
 4. r(p) = float(num(p)) / sqrt(float(vx) * float(vy)); NaN for every
    permutation when vx or vy is 0 (a constant matrix).
 5. The counts compare num(p) with num_obs: exact, with ties too.
An X with a non-finite entry above its diagonal is invalid: statistic and the
permutations' statistics NaN, counts 0, valid 0. Y must be finite.
"""
from __future__ import annotations

import numpy as np

import group_oracle as go

NAN = go.NAN
METHODS = ("pearson", "spearman")


def check(X, Y, perms):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = len(X)
    assert n >= 3 and X.shape == Y.shape == (n, n) and go.is_valid(Y)
    perms = np.asarray(perms, dtype=np.int64).reshape(-1, n)
    for row in perms:
        assert np.array_equal(np.sort(row), np.arange(n))
    return X, Y, perms, n


def column_sums(A):
    """The sum of every column over the rows ascending."""
    return np.cumsum(A, axis=0)[-1]


def centred(D):
    """Steps 1 to 3 of pearson: (xc, sxx, constant)."""
    n = len(D)
    A = go.mirrored(D)
    iu = np.triu_indices(n, 1)
    constant = bool((A[iu] == A[0, 1]).all())
    mx = go.halving_sum(column_sums(A)) / (np.float64(n) * np.float64(n - 1))
    xc = A - mx
    xc[np.diag_indices(n)] = 0.0
    return xc, go.halving_sum(column_sums(xc * xc)), constant


def pearson(X, Y, perms=()):
    """(r, n_ge, n_le, n_abs_ge, r of every permutation, valid) of one X."""
    X, Y, perms, n = check(X, Y, perms)
    P = len(perms)
    if not go.is_valid(X):
        return NAN, 0, 0, 0, np.full(P, NAN), 0
    with np.errstate(all="ignore"):
        xc, sxx, xconst = centred(X)
        yc, syy, yconst = centred(Y)
        if xconst or yconst:
            return NAN, 0, 0, 0, np.full(P, NAN), 1
        scale = np.sqrt(sxx * syy)
        rows = np.concatenate([np.arange(n)[None], perms])
        r = np.zeros(len(rows))
        for k, p in enumerate(rows):
            r[k] = go.halving_sum(column_sums(xc[np.ix_(p, p)] * yc)) / scale
    return (r[0], int((r[1:] >= r[0]).sum()), int((r[1:] <= r[0]).sum()),
            int((np.abs(r[1:]) >= np.abs(r[0])).sum()), r[1:], 1)


def spearman_sums(X, Y, perms=()):
    """(M, Sa, Sb, Saa, Sbb, Sab of the identity and of every permutation) as Python ints / int64."""
    X, Y, perms, n = check(X, Y, perms)
    iu = np.triu_indices(n, 1)
    a, b = go.twice_ranks(X), go.twice_ranks(Y)
    rows = np.concatenate([np.arange(n)[None], perms])
    sab = np.array([int((a[np.ix_(p, p)][iu] * b[iu]).sum()) for p in rows], dtype=np.int64)
    au, bu = a[iu], b[iu]
    return n * (n - 1) // 2, int(au.sum()), int(bu.sum()), int((au * au).sum()), int((bu * bu).sum()), sab


def spearman(X, Y, perms=()):
    """(r, n_ge, n_le, n_abs_ge, r of every permutation, valid) of one X."""
    X, Y, perms, n = check(X, Y, perms)
    P = len(perms)
    if not go.is_valid(X):
        return NAN, 0, 0, 0, np.full(P, NAN), 0
    M, sa, sb, saa, sbb, sab = spearman_sums(X, Y, perms)
    vx, vy = M * saa - sa * sa, M * sbb - sb * sb
    if vx == 0 or vy == 0:
        return NAN, 0, 0, 0, np.full(P, NAN), 1
    num = M * sab - sa * sb                       # int64: below 2^63 for N <= 128
    r = num.astype(np.float64) / np.sqrt(np.float64(vx) * np.float64(vy))
    return (r[0], int((num[1:] >= num[0]).sum()), int((num[1:] <= num[0]).sum()),
            int((np.abs(num[1:]) >= abs(num[0])).sum()), r[1:], 1)


TESTS = {"pearson": pearson, "spearman": spearman}


def batch(Xs, Y, perms, method):
    """The test of every X: (stat, n_ge, n_le, n_abs_ge, perm_stat, valid)
    arrays with a leading replicate axis."""
    n = len(Y)
    perms = np.asarray(perms).reshape(-1, n)
    rows = [TESTS[method](X, Y, perms) for X in Xs]
    stat, n_ge, n_le, n_abs, ps, valid = zip(*rows)
    u32 = lambda x: np.array(x, dtype=np.uint32)   # noqa: E731
    return (np.array(stat, dtype=np.float64), u32(n_ge), u32(n_le), u32(n_abs),
            np.array(ps, dtype=np.float64).reshape(len(Xs), len(perms)), np.array(valid, dtype=np.uint8))


def perm_rows(n, P, seed=0):
    """P permutations of 0..n-1 (int32 (P, n)); row 0 is the identity when P > 0."""
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.permutation(n) for _ in range(P)]) if P else np.zeros((0, n), dtype=np.int32)
    if P:
        rows[0] = np.arange(n)
    return np.ascontiguousarray(rows, dtype=np.int32)
