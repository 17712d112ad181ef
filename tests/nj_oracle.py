"""Neighbour joining with every operation order fixed (test helper, numpy only).

This file is the specification the GPU kernel (rna_clique_amd/csrc/nj.hip) is
compared against bit for bit. Saitou & Nei's algorithm in float64:

Input D[N][N]: only i < j is read; the matrix is mirrored and its diagonal is 0.
State: n active slots 0..n-1, a symmetric matrix over them, per slot a node id
(leaves 0..N-1, internal nodes N, N+1, ... in creation order) and a leaf bitmask.

While n > 3:
 1. r[i] = sum of D[k][i] over k = 0..n-1 in ascending k, added left to right.
 2. q(i, j) = ((double)(n - 2) * D[i][j] - r[i]) - r[j] for i < j; the minimum,
    ties to the lowest i, then the lowest j.
 3. li = 0.5 * D[i][j] + (r[i] - r[j]) / (2.0 * (n - 2)); lj = D[i][j] - li
    (not clamped).
 4. join t = N - n: children (node[i], node[j], -1), lengths (li, lj, 0.0),
    split leaves[i] | leaves[j].
 5. every other slot k: 0.5 * ((D[i][k] + D[j][k]) - D[i][j]) goes into slot i
    (new node id, merged mask); slot n - 1 moves into slot j when j != n - 1;
    n decreases by 1.
Last join: children node[0], node[1], node[2]; lengths 0.5 * ((D01 + D02) - D12),
0.5 * ((D01 + D12) - D02), 0.5 * ((D02 + D12) - D01).

A split is a bitmask over positions 0..N-1 in W = ceil(N / 64) 64-bit words,
complemented within N bits when bit 0 is set. A matrix with a non-finite entry
in its upper triangle is invalid: joins -1, lengths NaN, splits 0, valid 0.
"""
from __future__ import annotations

import numpy as np


def words(n):
    return (n + 63) // 64


def _mask_words(mask, n):
    """Python int bitmask -> canonical W uint64 words."""
    if mask & 1:
        mask = ~mask & ((1 << n) - 1)
    return [(mask >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(words(n))]


def nj(D):
    """(joins (N-2, 3) int32, lengths (N-2, 3) float64, splits (N-3, W) uint64,
    valid) of one matrix."""
    D = np.asarray(D, dtype=np.float64)
    N = D.shape[0]
    if D.ndim != 2 or D.shape[1] != N or N < 3:
        raise ValueError("need a square matrix of at least 3 samples")
    W = words(N)
    joins = np.full((N - 2, 3), -1, dtype=np.int32)
    lengths = np.full((N - 2, 3), np.nan, dtype=np.float64)
    splits = np.zeros((N - 3, W), dtype=np.uint64)
    if not np.isfinite(D[np.triu_indices(N, 1)]).all():
        return joins, lengths, splits, 0
    A = np.triu(D, 1)
    A = A + A.T
    node = list(range(N))
    leaves = [1 << i for i in range(N)]
    n = N
    while n > 3:
        V = A[:n, :n]
        r = np.cumsum(V, axis=0)[-1]
        Q = (np.float64(n - 2) * V - r[:, None]) - r[None, :]
        Q[np.tril_indices(n)] = np.inf
        i, j = (int(x) for x in np.unravel_index(int(np.argmin(Q)), Q.shape))
        dij = V[i, j]
        li = 0.5 * dij + (r[i] - r[j]) / (2.0 * (n - 2))
        lj = dij - li
        t = N - n
        joins[t] = (node[i], node[j], -1)
        lengths[t] = (li, lj, 0.0)
        merged = leaves[i] | leaves[j]
        splits[t] = _mask_words(merged, N)
        new = 0.5 * ((V[i] + V[j]) - dij)
        new[i] = 0.0
        A[i, :n] = new
        A[:n, i] = new
        node[i] = N + t
        leaves[i] = merged
        if j != n - 1:
            row = A[n - 1, :n].copy()
            row[j] = 0.0
            A[j, :n] = row
            A[:n, j] = row
            node[j] = node[n - 1]
            leaves[j] = leaves[n - 1]
        n -= 1
    d01, d02, d12 = A[0, 1], A[0, 2], A[1, 2]
    joins[N - 3] = (node[0], node[1], node[2])
    lengths[N - 3] = (0.5 * ((d01 + d02) - d12), 0.5 * ((d01 + d12) - d02), 0.5 * ((d02 + d12) - d01))
    return joins, lengths, splits, 1


def nj_batch(Ds):
    """nj() over a stack of matrices: arrays with a leading replicate axis."""
    out = [nj(D) for D in Ds]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], dtype=np.uint8))


def split_ints(splits):
    """(.., W) uint64 words -> Python ints, one per split."""
    s = np.asarray(splits, dtype=np.uint64)
    return [sum(int(row[w]) << (64 * w) for w in range(s.shape[-1])) for row in s.reshape(-1, s.shape[-1])]


def split_sets(splits, labels):
    """The splits as treecheck._split writes them: frozensets of labels."""
    return {frozenset(labels[b] for b in range(len(labels)) if m >> b & 1) for m in split_ints(splits)}


def support_counts(ref_splits, rep_splits, valid):
    """support[k] = number of valid replicates whose tree has reference split
    k; and the number of valid replicates."""
    ref = split_ints(ref_splits)
    counts = [0] * len(ref)
    nv = 0
    for r in range(len(rep_splits)):
        if not valid[r]:
            continue
        nv += 1
        have = set(split_ints(rep_splits[r]))
        for k, m in enumerate(ref):
            counts[k] += m in have
    return np.array(counts, dtype=np.uint32), nv
