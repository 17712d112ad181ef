"""PERMDISP (Anderson 2006, centroid form) with every operation order fixed
(test helper, numpy only).

This file is the specification the GPU kernel
(rna_clique_amd/csrc/dispersion.hip) and the host route
(rna_clique_amd.groups.dispersion_host) are compared against bit for bit.
Float64 throughout; inputs and checks as tests/group_oracle.py.

 1. v[i][j] = D[i][j] * D[i][j], mirrored, zero diagonal.
 2. For a label vector g, n_g[i] = the size of i's group. Every sum below runs
    over j = 0, 1, ..., N - 1, added left to right from 0.0, and takes the
    term when g[j] == g[i] and 0.0 otherwise (own_sums):
      t[i] = sum of v[j][i]         (group_oracle.row_sums)
      b[i] = sum of t[j]            (twice the sum of v inside i's group)
 3. z2[i] = t[i] / n_g[i] - b[i] / (2.0 * n_g[i] * n_g[i])
    z[i]  = sqrt(|z2[i]|): the distance to the group centroid in the full
    principal-coordinate space, imaginary axes subtracted (vegan's betadisper
    takes sqrt(abs()) as well). A singleton has t = b = 0, so z = 0.
 4. s[i] = sum of z[j] (own group, as in 2); m[i] = s[i] / n_g[i].
 5. SS_W = H((z - m)^2), zbar = H(z) / N, SS_T = H((z - zbar)^2), with H the
    halving sum of group_oracle (step 4 there).
 6. F = ((SS_T - SS_W) / (a - 1)) / (SS_W / (N - a)); SS_W == 0 gives what IEEE
    arithmetic gives.
 7. n_ge = the number of permutations with F_perm >= F_observed (false when
    either is NaN); a permutation recomputes steps 2 to 6 from its labels.
Every lane of the kernel gets its own group's sums with no loop over groups, so
the result depends on the partition g describes and on nothing else.
A matrix with a non-finite entry above its diagonal is invalid: statistic,
total, within, the permutations' statistics and the distances NaN, n_ge 0,
valid 0.
"""
from __future__ import annotations

import numpy as np

import group_oracle as go

NAN = go.NAN


def own_sums(G, X):
    """out[k, i] = the sum over j ascending of (X[k, j] if G[k, j] == G[k, i] else 0)."""
    G = np.asarray(G)
    same = G[:, :, None] == G[:, None, :]              # [k, j, i]
    return np.cumsum(np.where(same, X[:, :, None], np.float64(0)), axis=1)[:, -1, :]


def distances(V, G, sizes):
    """Steps 2 and 3 for every row of G (K, N) on the squared distances V: z (K, N), z2 (K, N)."""
    t = go.row_sums(V, G)
    b = own_sums(G, t)
    ng = sizes[G].astype(np.float64)
    z2 = t / ng - b / (2.0 * ng * ng)
    return np.sqrt(np.abs(z2)), z2


def anova(z, G, sizes, a):
    """Steps 4 to 6: (F, SS_T, SS_W) for every row."""
    n = z.shape[1]
    ng = sizes[G].astype(np.float64)
    m = own_sums(G, z) / ng
    dw = z - m
    ssw = go.halving_sum(dw * dw)
    zbar = go.halving_sum(z) / np.float64(n)
    dt = z - zbar[:, None]
    sst = go.halving_sum(dt * dt)
    F = ((sst - ssw) / np.float64(a - 1)) / (ssw / np.float64(n - a))
    return F, sst, ssw


def centroid_distances(D, labels):
    """(z, z2) of the observed labels of one valid matrix."""
    D = np.asarray(D, dtype=np.float64)
    labels, _, sizes = go.check(labels, (), len(D))
    A = go.mirrored(D)
    with np.errstate(all="ignore"):
        z, z2 = distances(A * A, labels[None], sizes)
    return z[0], z2[0]


def permdisp(D, labels, perm_labels=()):
    """(F, n_ge, SS_T, SS_W, F of every permutation, valid, z) of one matrix."""
    D = np.asarray(D, dtype=np.float64)
    n = len(D)
    labels, perms, sizes = go.check(labels, perm_labels, n)
    P, a = len(perms), len(sizes)
    if not go.is_valid(D):
        return NAN, 0, NAN, NAN, np.full(P, NAN), 0, np.full(n, NAN)
    A = go.mirrored(D)
    V = A * A
    G = np.concatenate([labels[None], perms])
    F, sst, ssw = np.zeros(len(G)), np.zeros(len(G)), np.zeros(len(G))
    z0 = None
    with np.errstate(all="ignore"):
        for k0 in range(0, len(G), 64):
            g = G[k0:k0 + 64]
            z, _ = distances(V, g, sizes)
            if k0 == 0:
                z0 = z[0]
            F[k0:k0 + 64], sst[k0:k0 + 64], ssw[k0:k0 + 64] = anova(z, g, sizes, a)
        n_ge = int((F[1:] >= F[0]).sum())
    return F[0], n_ge, sst[0], ssw[0], F[1:], 1, z0


def batch(Ds, labels, perm_labels):
    """PERMDISP of every matrix: (stat, n_ge, total, within, perm_stat, valid,
    dist) arrays with a leading replicate axis."""
    n = len(labels)
    perms = np.asarray(perm_labels).reshape(-1, n)
    rows = [permdisp(D, labels, perms) for D in Ds]
    stat, n_ge, total, within, ps, valid, dist = zip(*rows)
    return (np.array(stat, dtype=np.float64), np.array(n_ge, dtype=np.uint32), np.array(total, dtype=np.float64),
            np.array(within, dtype=np.float64), np.array(ps, dtype=np.float64).reshape(len(Ds), len(perms)),
            np.array(valid, dtype=np.uint8), np.array(dist, dtype=np.float64).reshape(len(Ds), n))


def six_sample_expected(D, labels, perms):
    """The count by enumeration for six samples in two groups of three: F of
    each of the 10 partitions (group_cases.six_sample_partitions) once, then the
    rows whose partition's F is >= the observed one."""
    import group_cases
    stat = {k: permdisp(D, g)[0] for k, g in group_cases.six_sample_partitions().items()}
    key = lambda row: frozenset(np.flatnonzero(row == row[0]).tolist())   # noqa: E731
    obs = stat[key(labels)]
    return sum(bool(stat[key(row)] >= obs) for row in perms)
