"""The census of the splits of replicate trees, Robinson-Foulds distances,
consensus trees and midpoint rooting, restated in plain Python (test helper,
numpy only for the arrays).

This file is the specification that rna_clique_amd/csrc/splits.hip (census and
distances, exactly) and rna_clique_amd/tree.py (consensus, means, rooting) are
compared against. Nothing here imports either.

Census. The trees are nj_oracle's: splits (R, ns, W) uint64 with ns = N - 3,
valid (R,). An instance is (replicate r, join t), flat index r * ns + t; only
valid replicates count. The distinct splits are numbered in ascending order of
their first instance's flat index -- a dict filled in that order. counts[k]:
the valid replicates with split k (a tree's splits are distinct); ids[r][t]:
the number of that instance's split, -1 in an invalid replicate.

Robinson-Foulds distance: the size of the symmetric difference of two trees'
split sets; 0xFFFFFFFF where an invalid replicate is involved.

Consensus. "strict": count == n_valid; "majority": count > threshold *
n_valid; "greedy": by (descending count, ascending number), a split is taken
when it fits every split taken so far, until N - 3 are taken. Two splits fit
one tree iff one of the four intersections of their sides is empty.

Means. The length of split k's edge in replicate r is the branch length of the
child N + t in r's joins, t the join of that split; the consensus length is
the sum over the replicates that have k, added in ascending r, divided once by
their number. A leaf's: the sum over all valid replicates, divided by n_valid.

Midpoint. Over a tree given as edges (u, v, length), leaves 0..n-1: the path
length from leaf i to leaf j is the sum of the path's lengths added in walking
order from i. The rooted pair is the (i < j) of the largest, ties to the lowest
i, then j; the root lies on that path where the running sum from i first
reaches half of it.
"""
from __future__ import annotations

import numpy as np

INVALID = 0xFFFFFFFF


def ints(splits):
    """(.., W) uint64 words -> Python ints."""
    s = np.asarray(splits, dtype=np.uint64)
    return [sum(int(row[w]) << (64 * w) for w in range(s.shape[-1])) for row in s.reshape(-1, s.shape[-1])]


def words(mask, n):
    return [(mask >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range((n + 63) // 64)]


def census(splits, valid):
    """(masks, counts (K,) uint32, ids (R, ns) int32, n_valid): masks are the
    distinct splits as ints, in first-occurrence order."""
    splits = np.asarray(splits, dtype=np.uint64)
    R, ns = splits.shape[0], splits.shape[1]
    number, counts = {}, []
    ids = np.full((R, ns), -1, dtype=np.int32)
    nv = 0
    for r in range(R):
        if not valid[r]:
            continue
        nv += 1
        for t, m in enumerate(ints(splits[r])):
            if m not in number:
                number[m] = len(number)
                counts.append(0)
            ids[r, t] = number[m]
            counts[number[m]] += 1
    return list(number), np.array(counts, dtype=np.uint32), ids, nv


def census_words(masks, n):
    """The masks as a (K, W) uint64 array."""
    return np.array([words(m, n) for m in masks], dtype=np.uint64).reshape(len(masks), (n + 63) // 64)


def rf_to_ref(ref_splits, splits, valid):
    ref = set(ints(ref_splits))
    return np.array([len(ref ^ set(ints(splits[r]))) if valid[r] else INVALID for r in range(len(splits))],
                    dtype=np.uint32)


def rf_pairwise(splits, valid):
    R = len(splits)
    sets = [set(ints(splits[r])) for r in range(R)]
    out = np.full((R, R), INVALID, dtype=np.uint32)
    for a in range(R):
        for b in range(R):
            if valid[a] and valid[b]:
                out[a, b] = len(sets[a] ^ sets[b])
    return out


def fits(a, b, n):
    """Two bipartitions of n positions (each given by one side) fit one tree."""
    full = (1 << n) - 1
    return not (a & b) or not (a & ~b & full) or not (~a & b & full) or not (~a & ~b & full)


def consensus_splits(masks, counts, n_valid, n, method, threshold=0.5):
    """Numbers of the chosen splits, ascending."""
    K = len(masks)
    if method == "strict":
        return [k for k in range(K) if int(counts[k]) == n_valid and n_valid]
    if method == "majority":
        return [k for k in range(K) if int(counts[k]) > threshold * n_valid]
    assert method == "greedy"
    taken = []
    for k in sorted(range(K), key=lambda k: (-int(counts[k]), k)):
        if len(taken) == n - 3:
            break
        if all(fits(masks[k], masks[j], n) for j in taken):
            taken.append(k)
    return sorted(taken)


def nesting(masks):
    """{mask: its smallest proper superset among masks, or None}."""
    out = {}
    for a in masks:
        above = [b for b in masks if b != a and a & b == a]
        out[a] = min(above, key=lambda b: bin(b).count("1")) if above else None
    return out


def mean_lengths(ids, joins, lengths, valid, chosen, n):
    """(split means for the chosen numbers, leaf means (n,)), each sum added
    in ascending replicate order."""
    sums, cnt = {k: 0.0 for k in chosen}, {k: 0 for k in chosen}
    leaf, nv = [0.0] * n, 0
    for r in range(len(ids)):
        if not valid[r]:
            continue
        nv += 1
        above = {}
        for t in range(n - 2):
            for c, length in zip(joins[r][t], lengths[r][t]):
                if c >= 0:
                    above[int(c)] = float(length)
        for t in range(n - 3):
            k = int(ids[r][t])
            if k in sums:
                sums[k] = sums[k] + above[n + t]
                cnt[k] += 1
        for b in range(n):
            leaf[b] = leaf[b] + above[b]
    return (np.array([sums[k] / cnt[k] for k in chosen], dtype=np.float64),
            np.array([x / nv for x in leaf], dtype=np.float64))


def conflicts(masks, counts, n_valid, n, tree_masks):
    """Per tree split: (number, frequency) of the most frequent census split
    that does not fit it, ties to the lowest number; (-1, 0.0) without one."""
    ids, freq = [], []
    for x in tree_masks:
        bad = [k for k in range(len(masks)) if not fits(x, masks[k], n)]
        if bad:
            k = min(bad, key=lambda k: (-int(counts[k]), k))
            ids.append(k)
            freq.append(int(counts[k]) / n_valid)
        else:
            ids.append(-1)
            freq.append(0.0)
    return np.array(ids, dtype=np.int64), np.array(freq, dtype=np.float64)


def nj_edges(joins, lengths):
    """Edges (child, parent, length) of one nj_oracle tree."""
    n = len(joins) + 2
    return [(int(c), n + t, float(length)) for t in range(n - 2) for c, length in zip(joins[t], lengths[t]) if c >= 0]


def _walk(edges, start):
    """Running path sums from `start` and the node before each."""
    nbr = {}
    for u, v, length in edges:
        nbr.setdefault(u, []).append((v, length))
        nbr.setdefault(v, []).append((u, length))
    total, before, todo = {start: 0.0}, {start: None}, [start]
    while todo:
        v = todo.pop()
        for c, length in nbr[v]:
            if c not in total:
                total[c] = total[v] + length
                before[c] = v
                todo.append(c)
    return total, before


def midpoint(n, edges):
    """(i, j, longest path, path nodes from i to j, running sums along it,
    index of the first path node whose running sum is >= half)."""
    best = None
    for i in range(n - 1):
        total, before = _walk(edges, i)
        for j in range(i + 1, n):
            if best is None or total[j] > best[0]:
                best = (total[j], i, j, total, before)
    longest, i, j, total, before = best
    path = [j]
    while path[-1] != i:
        path.append(before[path[-1]])
    path.reverse()
    sums = [total[v] for v in path]
    if not longest > 0:
        return i, j, longest, path, sums, None
    return i, j, longest, path, sums, next(k for k in range(1, len(path)) if sums[k] >= 0.5 * longest)
