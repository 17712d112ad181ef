"""Inputs of the group tests (test helper): the distance matrices of
tests/nj_cases.py per sample count, groupings and permuted label rows."""
from __future__ import annotations

import itertools

import numpy as np

import group_oracle as go
import nj_cases

SIZES = (3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 127, 128)
NAMES = ("noisy", "integer", "equal", "random", "garbage", "noisy2")
PERM_CHUNK = 120   # permutations per workgroup (groups.hip: GROUP_PERM_CHUNK, groups.GPU_PERM_CHUNK)


def matrices(n, seed=None):
    """Six valid matrices of n samples, in NAMES order: noisy additive, integer
    additive (tied distances, so tied ranks), all-equal, random non-metric, the
    first with garbage below and on its diagonal, another noisy additive one."""
    seed = n if seed is None else seed
    noisy = nj_cases.noisy_additive(n, seed)[0]
    return np.stack([noisy, nj_cases.additive(n, seed + 1, integer=True)[0], nj_cases.all_equal(n),
                     nj_cases.random_symmetric(n, seed + 2), nj_cases.with_garbage(noisy, seed + 3),
                     nj_cases.noisy_additive(n, seed + 4)[0]])


def with_nan(Ds, r=2):
    """The batch with a NaN above the diagonal of matrix r."""
    out = np.array(Ds)
    n = out.shape[1]
    out[r, 0, n - 1] = np.nan
    return out


def groupings(n):
    """{name: labels int32 (n,)}: two balanced groups, unbalanced groups with a
    singleton, n // 2 pairs (and a singleton for odd n), n - 1 groups (one
    pair). Fewer where n is too small for a design to differ or to be valid
    (2 <= groups < n)."""
    rng = np.random.default_rng(1000 + n)
    out = {"balanced": np.arange(n) % 2}
    if n >= 4:
        g = np.zeros(n, dtype=np.int64)
        g[n - 1] = 2                      # the singleton
        g[(n - 1) // 3:n - 1] = 1
        out["singleton"] = g
        out["pairs"] = np.arange(n) // 2
    one_pair = np.arange(n)
    one_pair[n - 1] = 0                   # samples 0 and n - 1 share a group
    one_pair[1:n - 1] = np.arange(1, n - 1)
    out["one_pair"] = one_pair
    shuffled = {}
    for k, g in out.items():
        g = rng.permutation(g)
        # number the groups by first occurrence, as encode_grouping does
        _, first, inv = np.unique(g, return_index=True, return_inverse=True)
        shuffled[k] = np.argsort(np.argsort(first))[inv].astype(np.int32)
    return shuffled


def perm_rows(labels, P, seed=0):
    """P permuted rows (int32 (P, n)); row 0 is the identity when P > 0."""
    labels = np.asarray(labels, dtype=np.int32)
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.permutation(labels) for _ in range(P)]) if P else np.zeros((0, len(labels)), dtype=np.int32)
    if P:
        rows[0] = labels
    return np.ascontiguousarray(rows, dtype=np.int32)


def renumberings(labels, seed=0):
    """Maps old group number -> new one (int32 (a,) each): three random ones
    and a rotation. m[labels] describes the partition of `labels`."""
    a = int(np.max(labels)) + 1
    rng = np.random.default_rng(seed)
    return [rng.permutation(a).astype(np.int32) for _ in range(3)] + [((np.arange(a) + 1) % a).astype(np.int32)]


def same_partition_rows(labels, seed=0):
    """Rearrangements of `labels` that describe its partition: groups of equal
    size exchange their numbers (what a permutation test draws when samples
    move within their groups or two equal groups swap as wholes)."""
    labels = np.asarray(labels, dtype=np.int32)
    sizes = np.bincount(labels)
    rng = np.random.default_rng(seed)
    rows = [labels]
    for _ in range(3):
        m = np.arange(len(sizes))
        for s in np.unique(sizes):
            idx = np.flatnonzero(sizes == s)
            m[idx] = rng.permutation(idx)
        rows.append(m.astype(np.int32)[labels])
    return np.stack(rows)


def six_sample_partitions():
    """The 10 partitions of 6 samples into two groups of three, as label vectors
    keyed by the group that holds sample 0."""
    out = {}
    for rest in itertools.combinations(range(1, 6), 2):
        g = np.ones(6, dtype=np.int32)
        g[[0, *rest]] = 0
        out[frozenset((0, *rest))] = g
    return out


def six_sample_expected(D, labels, perms, method):
    """The count by enumeration: the statistic of each of the 10 partitions
    once, then the rows whose partition's statistic is >= the observed one."""
    parts = six_sample_partitions()
    stat = {k: go.TESTS[method](D, g)[0] for k, g in parts.items()}
    key = lambda row: frozenset(np.flatnonzero(row == row[0]).tolist())   # noqa: E731
    obs = stat[key(labels)]
    return sum(bool(stat[key(row)] >= obs) for row in perms)
