"""Graph record cases for the component census (post_cases.GraphCase), shared
by tests/test_census_host.py and tests/test_gpu_census.py. A plain module: no
fixtures, no GPU."""
from __future__ import annotations

import itertools

import numpy as np

from post_cases import EDGE, NODE_ONLY, GraphCase, _w


class _Graph:
    """Genes are handed out per sample in ascending order; clique() joins one
    new gene of each given sample (or the given genes) all to all."""

    def __init__(self, n_samples, seed):
        self.rng = np.random.default_rng(seed)
        self.nxt = [0] * n_samples
        self.recs = []

    def gene(self, s):
        self.nxt[s] += 1
        return (s, self.nxt[s])

    def edge(self, u, v):
        self.recs.append((EDGE, u, v, *_w(self.rng)))

    def clique(self, samples):
        vs = [self.gene(s) for s in samples]
        for u, v in itertools.combinations(vs, 2):
            self.edge(u, v)
        return vs

    def node(self, s):
        v = self.gene(s)
        self.recs.append((NODE_ONLY, v, v, 0, 0))
        return v

    def case(self, name, sample_count=None):
        return GraphCase(name, self.nxt, self.recs, sample_count)


def pairs_case(n):
    """Exactly n two-node components over two samples: n roots in the scan
    and n rows in the scatter (n around 64 and 256: a wave and a block)."""
    g = _Graph(2, 40 + n)
    for _ in range(n):
        g.clique([0, 1])
    return g.case(f"pairs{n}")


# (sample lacking, how many complete cliques over the other S - 1 samples lack it)
MISSING = {0: 3, 2: 5, 4: 2}


def missing_sample_case():
    """Five samples and a sixth whose only node is a node-only record: P = 6,
    so the ideal test has S = 6 and finds nothing, and the four 5-cliques are
    the one_short components, all lacking sample 5. The complete cliques over
    four of the first five samples (lacking the first, a middle and the last
    3, 5 and 2 times) are two short here; missing_sample_case5 has their
    counts."""
    g = _Graph(6, 51)
    for skip, times in MISSING.items():
        for _ in range(times):
            g.clique([s for s in range(5) if s != skip])
    for _ in range(4):
        g.clique(range(5))
    g.node(5)
    return g.case("missing-sample-6")


def missing_sample_case5():
    """Five samples (P = S = 5): four ideal cliques; complete four-sample
    cliques lacking sample 0 three times, sample 2 five times and sample 4
    twice (one_short: missing_sample_counts is exactly MISSING); a four-node
    component with three genes of sample 1 and one of sample 3 (nodes == P - 1
    but not single-copy, and not complete); a four-clique missing one edge; a
    sample-3 gene that is a node-only record; interleaved so that sample
    boundaries fall at every position of a member slice."""
    g = _Graph(5, 52)
    todo = [skip for skip, times in MISSING.items() for _ in range(times)]
    order = g.rng.permutation(len(todo))
    for i, k in enumerate(order.tolist()):
        g.clique([s for s in range(5) if s != todo[k]])
        if i % 3 == 0:
            g.clique(range(5))
    a, b, c, d = g.gene(1), g.gene(1), g.gene(1), g.gene(3)
    for u in (a, b, c):
        g.edge(u, d)
    vs = [g.gene(s) for s in (0, 1, 2, 3)]
    for u, v in list(itertools.combinations(vs, 2))[:-1]:
        g.edge(u, v)
    g.node(3)
    return g.case("missing-sample-5")


def wide_case():
    """70 samples (more than a wave has lanes): one 70-clique, one 69-clique
    lacking sample 64, one 69-clique lacking sample 0."""
    g = _Graph(70, 53)
    g.clique(range(70))
    g.clique([s for s in range(70) if s != 64])
    g.clique([s for s in range(70) if s != 0])
    return g.case("wide70")


def hand_case():
    """The hand-written 3-sample graph of test_census_host (every derived
    column is written out there). Components in id order:
      0  triangle (0,1) (1,1) (2,1)            ideal
      1  pair (0,2)-(1,2)                      one_short, lacks sample 2
      2  pair (0,3)-(2,2)                      one_short, lacks sample 1
      3  path (0,4)-(1,3)-(2,3)                three samples, one edge short
      4  pair (0,5)-(1,6)                      one_short, lacks sample 2
      5  node (1,4)                            one node, density NaN
      6  (1,5)-(2,4), (1,5)-(2,5)              three nodes of two samples"""
    e = lambda u, v: (EDGE, u, v, 90, 100)   # noqa: E731
    recs = [e((0, 1), (1, 1)), e((0, 1), (2, 1)), e((1, 1), (2, 1)),
            e((0, 2), (1, 2)), e((0, 3), (2, 2)),
            e((0, 4), (1, 3)), e((1, 3), (2, 3)),
            e((0, 5), (1, 6)), (NODE_ONLY, (1, 4), (1, 4), 0, 0),
            e((1, 5), (2, 4)), e((1, 5), (2, 5))]
    return GraphCase("hand", [5, 6, 5], recs)


def new_cases():
    """Every new case that is small enough for the host cross-checks."""
    out = [pairs_case(n) for n in (63, 64, 65, 255, 256, 257)]
    out += [missing_sample_case(), missing_sample_case5(), wide_case(), hand_case()]
    return {c.name: c for c in out}
