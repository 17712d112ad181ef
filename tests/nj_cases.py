"""Distance matrices for the neighbour-joining tests (test helper): additive
trees from simulate.birth_death_tree with and without noise, tie-heavy and
non-metric matrices."""
from __future__ import annotations

import numpy as np


def tree_distances(parent, blen, leaves):
    """Path lengths between the leaves of a parent-array tree."""
    def path(v):
        out = []
        while v >= 0:
            out.append(v)
            v = int(parent[v])
        return out
    paths = [path(x) for x in leaves]
    n = len(leaves)
    D = np.zeros((n, n))
    for i in range(n):
        si = set(paths[i])
        for j in range(i + 1, n):
            sj = set(paths[j])
            D[i, j] = D[j, i] = sum(blen[v] for v in paths[i] if v not in sj) + \
                sum(blen[v] for v in paths[j] if v not in si)
    return D


def additive(n, seed, integer=False):
    """(D, parent, leaves) of a birth-death tree with n leaves; with `integer`
    the branch lengths are small integers, so that q has exact ties."""
    from rna_clique_amd.simulate import birth_death_tree
    rng = np.random.default_rng(seed)
    parent, blen, leaves = birth_death_tree(n, rng)
    blen = np.asarray(blen, dtype=np.float64)
    if integer:
        blen = rng.integers(1, 4, size=len(blen)).astype(np.float64)
    return tree_distances(parent, blen, leaves), parent, leaves


def noisy(D, seed, frac=0.02):
    """D plus symmetric noise below frac of its shortest distance: tie-free."""
    rng = np.random.default_rng(seed)
    n = len(D)
    amp = frac * D[np.triu_indices(n, 1)].min()
    E = np.triu(rng.uniform(-amp, amp, size=(n, n)), 1)
    return D + E + E.T


def jitter(D, seed, rel=0.3):
    """Every distance scaled by its own factor in [1 - rel, 1 + rel]: replicates
    of one tree whose topologies differ."""
    rng = np.random.default_rng(seed)
    n = len(D)
    F = np.triu(rng.uniform(1.0 - rel, 1.0 + rel, size=(n, n)), 1)
    return D * (F + F.T)


def noisy_additive(n, seed):
    D, parent, leaves = additive(n, seed)
    return noisy(D, seed + 1000), parent, leaves


def all_equal(n, value=0.25):
    return np.full((n, n), value) - value * np.eye(n)


def random_symmetric(n, seed):
    """Not a metric: neighbour joining gives negative branch lengths."""
    rng = np.random.default_rng(seed)
    E = np.triu(rng.uniform(0.01, 1.0, size=(n, n)), 1)
    return E + E.T


def with_garbage(D, seed):
    """The same upper triangle; NaN, infinities and noise below it and on the
    diagonal (which neighbour joining must not read)."""
    rng = np.random.default_rng(seed)
    n = len(D)
    G = rng.uniform(-5, 5, size=(n, n))
    G[rng.random((n, n)) < 0.2] = np.nan
    G[rng.random((n, n)) < 0.1] = np.inf
    out = np.array(D, dtype=np.float64)
    low = np.tril_indices(n)
    out[low] = G[low]
    return out
