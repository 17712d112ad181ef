"""Neighbour-joining trees as the engine returns them (rc_nj,
rc_resample_trees): joins, branch lengths and splits, with Newick output.

The reference's tutorial ends in Biopython's DistanceTreeConstructor().nj and
a Newick file (docs/tutorials/reads2tree/make_tree.py); NJTree.newick() writes
that unrooted tree, the last join as a trifurcation, which is what Biopython's
nj returns before rooting.
"""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np

# Arrays of a batch of trees: joins (R, N-2, 3) int32, lengths (R, N-2, 3)
# float64, splits (R, N-3, W) uint64, valid (R,) uint8; support (n_ref,) uint32
# or None, n_valid int.
NJResult = namedtuple("NJResult", "joins lengths splits valid support n_valid")

# The census of the splits of a batch of trees (Engine.split_census): splits
# (K, W) uint64, the distinct splits in ascending order of their first
# occurrence (replicate-major, then join order); counts (K,) uint32, the valid
# trees that have each; ids (R, N-3) int32, the number of split t of tree r, -1
# in an invalid tree; n_valid int.
SplitCensus = namedtuple("SplitCensus", "splits counts ids n_valid")

_PLAIN = re.compile(r"^[^\s()\[\]':;,_]+$")


def split_words(n):
    """64-bit words of a split over n positions."""
    return (n + 63) // 64


def _quote(label):
    s = str(label)
    if _PLAIN.match(s):
        return s
    return "'" + s.replace("'", "''") + "'"


class NJTree:
    """One neighbour-joining tree over `labels` (matrix order).

    joins (N-2, 3): children of internal node N + t (leaves are 0..N-1), the
    third -1 except in the last join, which joins the three remaining nodes;
    lengths: the children's branch lengths; splits (N-3, W) uint64: the leaves
    under join t as a bitmask over label positions, on the side without
    position 0; support: None or one value per split (join order)."""

    def __init__(self, labels, joins, lengths, splits, support=None):
        self.labels = list(labels)
        n = len(self.labels)
        if n < 3:
            raise ValueError("a tree needs at least 3 samples")
        self.joins = np.asarray(joins, dtype=np.int32).reshape(n - 2, 3)
        self.lengths = np.asarray(lengths, dtype=np.float64).reshape(n - 2, 3)
        self.splits = np.asarray(splits, dtype=np.uint64).reshape(n - 3, split_words(n))
        self.support = None if support is None else np.asarray(support, dtype=np.float64).reshape(n - 3)

    def split_masks(self):
        """The splits as Python ints (bit b = labels[b])."""
        return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in self.splits]

    def splits_as_sets(self):
        """The non-trivial bipartitions as frozensets of labels, each on the
        side without the first label, in join order."""
        n = len(self.labels)
        return [frozenset(self.labels[b] for b in range(n) if m >> b & 1) for m in self.split_masks()]

    def newick(self, support=True):
        """The unrooted tree in Newick format. Lengths are written with repr
        (they read back exactly); an internal node's label is its support as
        an integer percentage when the tree has support values; labels that
        need it are quoted."""
        n = len(self.labels)
        text = {i: _quote(l) for i, l in enumerate(self.labels)}
        for t in range(n - 2):
            kids = [f"{text.pop(int(c))}:{float(l)!r}" for c, l in zip(self.joins[t], self.lengths[t]) if c >= 0]
            label = ""
            if support and self.support is not None and t < n - 3:
                label = str(int(round(100.0 * float(self.support[t]))))
            text[n + t] = "(" + ",".join(kids) + ")" + label
        return text[2 * n - 3] + ";"

    def split_lengths(self):
        """(N-3,) float64: entry t is the length of the edge above join t, the
        edge of split t (the entry of `lengths` where `joins` is N + t)."""
        n = len(self.labels)
        out = np.zeros(n - 3, dtype=np.float64)
        pos = self.joins >= n
        out[self.joins[pos] - n] = self.lengths[pos]
        return out

    def leaf_lengths(self):
        """(N,) float64: the length of every leaf's edge."""
        n = len(self.labels)
        out = np.zeros(n, dtype=np.float64)
        pos = (self.joins >= 0) & (self.joins < n)
        out[self.joins[pos]] = self.lengths[pos]
        return out

    def __repr__(self):
        return f"NJTree({len(self.labels)} leaves{', support' if self.support is not None else ''})"


# ---------------------------------------------------------------------------
# consensus trees of counted splits
# ---------------------------------------------------------------------------

def mask_ints(splits):
    """(m, W) uint64 words -> Python ints, one per split (bit b = position b)."""
    s = np.asarray(splits, dtype=np.uint64)
    return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in s.reshape(-1, s.shape[-1])]


def compatible(a, b):
    """Two canonical splits (ints; neither holds position 0) fit into one
    tree iff they are disjoint or nested."""
    x = a & b
    return x == 0 or x == a or x == b


def consensus_splits(census, method="majority", threshold=0.5):
    """Indices into `census` (ascending) of a consensus tree's splits.
    "strict": the splits of every valid tree; "majority": those of more than
    threshold * n_valid trees (threshold in [0.5, 1): any two of them share a
    tree, so they are compatible); "greedy" (extended majority rule): the
    splits by descending count, ties by ascending number, each accepted when
    it is compatible with every split accepted before it, until N - 3 are."""
    counts = np.asarray(census.counts, dtype=np.int64)
    nv = int(census.n_valid)
    if method == "strict":
        return np.nonzero(counts == nv)[0] if nv else np.zeros(0, dtype=np.int64)
    if method == "majority":
        if not 0.5 <= threshold < 1:
            raise ValueError("threshold must lie in [0.5, 1)")
        return np.nonzero(counts > threshold * nv)[0]
    if method != "greedy":
        raise ValueError("method must be 'strict', 'majority' or 'greedy'")
    full = np.asarray(census.ids).shape[1]
    masks = mask_ints(census.splits)
    taken = []
    for k in np.lexsort((np.arange(len(counts)), -counts)):
        if len(taken) == full:
            break
        if all(compatible(masks[k], masks[j]) for j in taken):
            taken.append(int(k))
    return np.array(sorted(taken), dtype=np.int64)


def _newick_from(adj, root, n, labels):
    """Newick text of the tree `adj` (node -> [(neighbour, length or None,
    label of that edge)]) hung from `root`; nodes below n are the leaves.
    Children in ascending order of the lowest leaf position below them; an
    internal node carries the label of the edge to its parent."""
    order, parent = [root], {root: (None, None, "")}
    for v in order:   # grows while it is walked
        for c, length, label in adj[v]:
            if c != parent[v][0]:
                parent[c] = (v, length, label)
                order.append(c)
    low, text, kids = {}, {}, {v: [] for v in order}
    for v in reversed(order):
        if v < n and v != root:
            low[v], text[v] = v, _quote(labels[v])
        else:
            ks = sorted(kids[v], key=lambda c: low[c])
            low[v] = min([low[c] for c in ks] + ([v] if v < n else []))
            text[v] = "(" + ",".join(text[c] for c in ks) + ")" + parent[v][2]
        p, length, _ = parent[v]
        if p is not None:
            if length is not None:
                text[v] += f":{float(length)!r}"
            kids[p].append(v)
    return text[root] + ";"


def _percent(support, k):
    return str(int(round(100.0 * float(support[k]))))


class SplitTree:
    """An unrooted, possibly multifurcating tree over `labels` from pairwise
    compatible canonical splits (m, W) uint64 (bit b = labels[b]; none holds
    position 0 or is trivial). A split's parent is its smallest superset among
    the splits; the top node holds labels[0] and every split and leaf without
    one. support, lengths: None or one value per split (the length of the
    split's edge); leaf_lengths: None or one value per label. ValueError on an
    incompatible pair."""

    def __init__(self, labels, splits, support=None, lengths=None, leaf_lengths=None):
        self.labels = list(labels)
        n = len(self.labels)
        if n < 3:
            raise ValueError("a tree needs at least 3 samples")
        self.splits = np.asarray(splits, dtype=np.uint64).reshape(-1, split_words(n))
        m = len(self.splits)
        opt = lambda a, k: None if a is None else np.asarray(a, dtype=np.float64).reshape(k)   # noqa: E731
        self.support, self.lengths, self.leaf_lengths = opt(support, m), opt(lengths, m), opt(leaf_lengths, n)
        masks = self.split_masks()
        size = [bin(x).count("1") for x in masks]
        for x, c in zip(masks, size):
            if x & 1 or x >> n or c < 2 or c > n - 2:
                raise ValueError("not a canonical non-trivial split over these labels")
        # by ascending size: the first superset met is the smallest
        order = sorted(range(m), key=lambda i: (size[i], i))
        self._parent = np.full(m, -1, dtype=np.int64)
        for a, i in enumerate(order):
            for j in order[a + 1:]:
                x = masks[i] & masks[j]
                if x == masks[i] and size[j] > size[i]:
                    if self._parent[i] < 0:
                        self._parent[i] = j
                elif x:
                    raise ValueError("incompatible (or equal) splits")
        self._leaf_parent = np.full(n, -1, dtype=np.int64)
        for i in order:
            x = masks[i]
            for b in range(1, n):
                if x >> b & 1 and self._leaf_parent[b] < 0:
                    self._leaf_parent[b] = i

    def split_masks(self):
        """The splits as Python ints (bit b = labels[b])."""
        return mask_ints(self.splits)

    def splits_as_sets(self):
        """The splits as frozensets of labels, each on the side without the
        first label, in the order given."""
        n = len(self.labels)
        return [frozenset(self.labels[b] for b in range(n) if m >> b & 1) for m in self.split_masks()]

    def _adjacency(self, support, need_lengths=False):
        """(adj, top): leaves 0..n-1, split i is node n + i, the top n + m."""
        n, m = len(self.labels), len(self.splits)
        if need_lengths and (self.lengths is None or self.leaf_lengths is None):
            raise ValueError("the tree has no branch lengths")
        adj = {v: [] for v in range(n + m + 1)}

        def edge(child, parent, length, label):
            adj[child].append((parent, length, label))
            adj[parent].append((child, length, label))
        for b in range(n):
            p = self._leaf_parent[b]
            edge(b, n + (m if p < 0 else int(p)), None if self.leaf_lengths is None else self.leaf_lengths[b], "")
        for i in range(m):
            p = self._parent[i]
            label = _percent(self.support, i) if support and self.support is not None else ""
            edge(n + i, n + (m if p < 0 else int(p)), None if self.lengths is None else self.lengths[i], label)
        return adj, n + m

    def newick(self, support=True):
        """The unrooted tree in Newick format, written from the top node, a
        node's children in ascending order of their lowest label position;
        quoting, lengths and support labels as NJTree.newick writes them
        (no lengths when the tree has none)."""
        adj, top = self._adjacency(support)
        return _newick_from(adj, top, len(self.labels), self.labels)

    def __repr__(self):
        return f"SplitTree({len(self.labels)} leaves, {len(self.splits)} splits)"


def _valid_rows(joins):
    return np.asarray(joins)[:, 0, 0] >= 0


def consensus_tree(census, labels, lengths=None, joins=None, method="majority", threshold=0.5):
    """The SplitTree of consensus_splits(census, method, threshold) with
    support = count / n_valid. With the replicates' `lengths` and `joins`
    (R, N-2, 3; NJResult's), a split's edge length is the mean of its edge's
    lengths over the replicates that have it and a leaf's the mean over the
    valid replicates: each sum is added in ascending replicate order in
    float64 and divided once."""
    labels = list(labels)
    n = len(labels)
    idx = consensus_splits(census, method, threshold)
    counts = np.asarray(census.counts, dtype=np.int64)
    nv = int(census.n_valid)
    support = counts[idx] / float(nv) if nv else np.zeros(len(idx))
    mean = leaf = None
    if (lengths is None) != (joins is None):
        raise ValueError("lengths and joins go together")
    if lengths is not None:
        joins = np.asarray(joins, dtype=np.int32).reshape(-1, n - 2, 3)
        lengths = np.asarray(lengths, dtype=np.float64).reshape(-1, n - 2, 3)
        ok = _valid_rows(joins)
        joins, lengths = joins[ok], lengths[ok]
        rv = len(joins)
        if rv != nv:
            raise ValueError("the replicates are not those of the census")
        rows = np.arange(rv)[:, None, None]
        # per replicate: the edge length of every split (join order) and leaf
        sl = np.zeros((rv, n - 3), dtype=np.float64)
        inner = joins >= n
        sl[np.broadcast_to(rows, joins.shape)[inner], joins[inner] - n] = lengths[inner]
        ll = np.zeros((rv, n), dtype=np.float64)
        outer = (joins >= 0) & (joins < n)
        ll[np.broadcast_to(rows, joins.shape)[outer], joins[outer]] = lengths[outer]
        # np.bincount adds in input order: replicate-major, so ascending replicate
        ids = np.asarray(census.ids)[ok]
        sums = np.bincount(ids.ravel(), weights=sl.ravel(), minlength=len(counts))
        mean = sums[idx] / counts[idx]
        leaf = np.bincount(np.tile(np.arange(n), rv), weights=ll.ravel(), minlength=n) / float(nv)
    return SplitTree(labels, np.asarray(census.splits, dtype=np.uint64)[idx], support, mean, leaf)


def conflicts(census, tree):
    """For every split k of `tree` (an NJTree or a SplitTree): the number and
    the frequency (count / n_valid) of the most frequent census split that is
    incompatible with it, ties to the lowest number; (-1, 0.0) when every
    census split fits. What the replicates prefer where a split is weak.
    Returns (ids (m,) int64, frequency (m,) float64)."""
    counts = np.asarray(census.counts, dtype=np.int64)
    masks = mask_ints(census.splits)
    ranked = [int(k) for k in np.lexsort((np.arange(len(counts)), -counts))]
    mine = tree.split_masks()
    ids = np.full(len(mine), -1, dtype=np.int64)
    freq = np.zeros(len(mine), dtype=np.float64)
    for i, x in enumerate(mine):
        for k in ranked:
            if not compatible(x, masks[k]):
                ids[i] = k
                freq[i] = counts[k] / float(census.n_valid)
                break
    return ids, freq


# ---------------------------------------------------------------------------
# midpoint rooting
# ---------------------------------------------------------------------------

def _nj_adjacency(tree, support):
    n = len(tree.labels)
    adj = {v: [] for v in range(2 * n - 2)}
    for t in range(n - 2):
        for c, length in zip(tree.joins[t], tree.lengths[t]):
            if c < 0:
                continue
            c = int(c)
            label = _percent(tree.support, c - n) if c >= n and support and tree.support is not None else ""
            adj[c].append((n + t, float(length), label))
            adj[n + t].append((c, float(length), label))
    return adj


def _distances_from(adj, start):
    """Path length from `start` to every node, each path's edges added in
    walking order from `start`; and the node before each on that path."""
    dist, before, todo = {start: 0.0}, {start: None}, [start]
    while todo:
        v = todo.pop()
        for c, length, _ in adj[v]:
            if c not in dist:
                dist[c] = dist[v] + length
                before[c] = v
                todo.append(c)
    return dist, before


def midpoint_newick(tree, support=True):
    """`tree` (an NJTree, or a SplitTree with lengths) rooted at its midpoint,
    in Newick format: the tutorial's root_at_midpoint(). Path lengths between
    leaves use the branch lengths as they are (negative ones are not clamped),
    added along the path from the lower leaf position. The pair (i < j) of the
    largest path length is taken, ties to the lowest i, then the lowest j; the
    root sits on that path at half its length from i, as a new node with two
    children that divides the edge it falls in (both halves keep the edge's
    support label), or at the node it falls on exactly. ValueError when the
    largest path length is not positive. Labels, quoting and lengths as in
    newick(); children in ascending order of their lowest label position."""
    n = len(tree.labels)
    if isinstance(tree, NJTree):
        adj = _nj_adjacency(tree, support)
    else:
        adj = tree._adjacency(support, need_lengths=True)[0]
        adj = {v: [(c, float(length), label) for c, length, label in e] for v, e in adj.items()}
    best, bi, bj, walk = -np.inf, -1, -1, None
    for i in range(n - 1):
        dist, before = _distances_from(adj, i)
        for j in range(i + 1, n):
            if dist[j] > best:
                best, bi, bj, walk = dist[j], i, j, (dist, before)
    if not best > 0:
        raise ValueError("the longest path between two leaves is not positive")
    dist, before = walk
    path = [bj]
    while path[-1] != bi:
        path.append(before[path[-1]])
    path.reverse()
    half = 0.5 * best
    k = next(k for k in range(1, len(path)) if dist[path[k]] >= half)
    a, b = path[k - 1], path[k]
    if dist[b] == half:
        root = b
    else:
        root = max(adj) + 1
        label = next(lab for c, _, lab in adj[a] if c == b)
        adj[a] = [e for e in adj[a] if e[0] != b] + [(root, half - dist[a], label)]
        adj[b] = [e for e in adj[b] if e[0] != a] + [(root, dist[b] - half, label)]
        adj[root] = [(a, half - dist[a], label), (b, dist[b] - half, label)]
    return _newick_from(adj, root, n, tree.labels)
