"""Per-component tables and resampling, restated in plain Python and numpy
(test helper: no GPU, no engine).

From a gene matches graph (nodes, edges), the table rows as records and the
sample count it computes what rc_ideal_components, rc_component_sums and
rc_resample must return:

* the ideal components through post_oracle.components / ideal_nodes, numbered
  in ascending order of their lowest node -- nodes are (sample index, gene),
  so this is the engine's lowest global gene index (genes are numbered
  sample-major in ascending gene id);
* the members of each, ascending;
* the [C][P] sums: a record (u, v, nident, den) counts iff both endpoints are
  ideal nodes and goes to the component of its higher-sample endpoint (the
  table's qsample / qgene), at the pair's index in the engine's single-shard
  pair numbering (post_cases.pair_index);
* resample(W) = W.astype(object) @ S in Python integers;
* distances as float(1 - Fraction(num, den)) and as (den - num) / den in
  float64 (equal while den < 2^53).

Samples are indices in the engine's order; use `index_nodes` for labelled
graphs.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from oracle import post_oracle as po


def pair_index(a, b):
    """Single-shard pair numbering (post_cases.pair_index)."""
    a, b = min(a, b), max(a, b)
    return b * (b - 1) // 2 + a


class ComponentTables:
    """members: [C] lists of S (sample, gene) nodes, ascending; num / den:
    object arrays (C, P) of Python integers."""

    def __init__(self, records, nodes, edges, sample_count, n_samples):
        nodes, edges = set(nodes), set(edges)
        self.n_samples = n_samples
        self.n_pairs = n_samples * (n_samples - 1) // 2
        self.sample_count = sample_count
        valid = po.ideal_nodes(nodes, edges, sample_count) if sample_count else set()
        # (a component is ideal as a whole: the components of the ideal nodes alone)
        comps, _ = po.components(valid, {e for e in edges if e[0] in valid})
        self.members = sorted((sorted(c) for c in comps), key=lambda c: c[0])
        self.valid = valid
        comp_of = {v: i for i, c in enumerate(self.members) for v in c}
        C = len(self.members)
        self.num = np.zeros((C, self.n_pairs), dtype=object)
        self.den = np.zeros((C, self.n_pairs), dtype=object)
        self.crossing = 0   # counted records whose endpoints lie in two different components
        for u, v, nident, den in records:
            if u in valid and v in valid:
                b = u if u[0] > v[0] else v
                assert u[0] != v[0]
                c, p = comp_of[b], pair_index(u[0], v[0])
                self.num[c, p] += int(nident)
                self.den[c, p] += int(den)
                self.crossing += comp_of[u] != comp_of[v]

    @property
    def n_components(self):
        return len(self.members)

    def member_arrays(self):
        """(sample, gene) int32 arrays (C, S), as Engine.ideal_components()."""
        S = self.sample_count
        s = np.array([[v[0] for v in c] for c in self.members], dtype=np.int32).reshape(len(self.members), S)
        g = np.array([[v[1] for v in c] for c in self.members], dtype=np.int32).reshape(len(self.members), S)
        return s, g

    def sums_int64(self):
        return self.num.astype(np.int64), self.den.astype(np.int64)

    def pair_sums(self):
        """{(a, b): (num, den)}: the table summed over the components."""
        tn = self.num.sum(axis=0) if self.n_components else [0] * self.n_pairs
        td = self.den.sum(axis=0) if self.n_components else [0] * self.n_pairs
        return {(a, b): (int(tn[pair_index(a, b)]), int(td[pair_index(a, b)]))
                for b in range(self.n_samples) for a in range(b)}

    def resample(self, W):
        """(num, den) object arrays (R, P): W @ S in Python integers."""
        W = np.asarray(W)
        assert W.ndim == 2 and W.shape[1] == self.n_components
        Wo = W.astype(object)
        if not self.n_components or not self.n_pairs:
            z = np.zeros((W.shape[0], self.n_pairs), dtype=object)
            return z, z.copy()
        return Wo @ self.num, Wo @ self.den

    def distances(self, W, order, exact=False):
        """(R, M, M) float64 for sample indices `order`: (den - num) / den in
        float64, or float(1 - Fraction(num, den)) when `exact`; 0 on the
        diagonal, NaN where den == 0."""
        num, den = self.resample(W)
        return distances_from_sums(num, den, order, exact)


def distances_from_sums(num, den, order, exact=False):
    R, M = num.shape[0], len(order)
    out = np.zeros((R, M, M), dtype=np.float64)
    for r in range(R):
        for i, a in enumerate(order):
            for j, b in enumerate(order):
                if a == b:
                    continue
                n_, d_ = int(num[r, pair_index(a, b)]), int(den[r, pair_index(a, b)])
                if d_ == 0:
                    out[r, i, j] = np.nan
                elif exact:
                    out[r, i, j] = float(1 - Fraction(n_, d_))
                else:
                    out[r, i, j] = np.float64(d_ - n_) / np.float64(d_)
    return out


def index_nodes(samples, nodes, edges):
    """A labelled graph -> (sample index, gene) nodes and sorted edges."""
    ix = {s: i for i, s in enumerate(samples)}
    n2 = {(ix[s], int(g)) for s, g in nodes}
    e2 = {tuple(sorted(((ix[u[0]], int(u[1])), (ix[v[0]], int(v[1]))))) for u, v in edges}
    return n2, e2


def records_from_tables(samples, tables):
    """Gene matches tables {(t1 label, t2 label): rows with sgene, qgene,
    nident, length, gaps} -> records ((t1, sgene), (t2, qgene), nident,
    length - gaps)."""
    ix = {s: i for i, s in enumerate(samples)}
    for (t1, t2), rows in tables.items():
        for r in rows:
            yield ((ix[t1], int(r["sgene"])), (ix[t2], int(r["qgene"])), int(r["nident"]),
                   int(r["length"]) - int(r["gaps"]))


def records_from_case(case):
    """A post_cases.GraphCase's edge and sums-only records."""
    for kind, u, v, nident, den in case.recs:
        if kind != 2:   # post_cases.NODE_ONLY
            yield (u, v, nident, den)


def from_case(case):
    nodes, edges = case.graph()
    sc = case.sample_count if case.sample_count else po.sample_count(nodes)
    return ComponentTables(records_from_case(case), nodes, edges, sc, len(case.genes))
