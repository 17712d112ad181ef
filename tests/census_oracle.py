"""The component census restated in plain Python (test helper: no GPU, no
engine).

From a gene matches graph (nodes, edges) and the sample count it states what
rc_components and rc_component_members must return: the connected components
of post_oracle.components over all nodes, numbered in ascending order of their
lowest node -- nodes are (sample index, gene), so this is the engine's lowest
global gene index --, per component the root, the member and edge counts and
the distinct samples, and the members of each in ascending order.

Samples are indices in the engine's order; use component_oracle.index_nodes
for labelled graphs.
"""
from __future__ import annotations

import numpy as np

from oracle import post_oracle as po


class Census:
    """members: [K] sorted lists of (sample, gene); edges: [K] edge counts."""

    def __init__(self, nodes, edges, sample_count):
        nodes, edges = set(nodes), {tuple(sorted(e)) for e in edges}
        assert all(u in nodes and v in nodes and u != v for u, v in edges)
        comps, _ = po.components(nodes, edges)
        self.members = sorted((sorted(c) for c in comps), key=lambda c: c[0])
        comp_of = {v: i for i, c in enumerate(self.members) for v in c}
        self.edges = [0] * len(self.members)
        for u, v in edges:
            assert comp_of[u] == comp_of[v]
            self.edges[comp_of[u]] += 1
        self.sample_count = int(sample_count)
        self.present_samples = len({s for s, _ in nodes})

    def __len__(self):
        return len(self.members)

    def arrays(self):
        """The columns as Engine.components() returns them."""
        return {"root_sample": np.array([c[0][0] for c in self.members], dtype=np.int32),
                "root_gene": np.array([c[0][1] for c in self.members], dtype=np.int32),
                "nodes": np.array([len(c) for c in self.members], dtype=np.int64),
                "edges": np.array(self.edges, dtype=np.int64),
                "samples": np.array([len({s for s, _ in c}) for c in self.members], dtype=np.int32)}

    def member_arrays(self):
        """(sample, gene) int32 arrays, as Engine.component_members()."""
        flat = [v for c in self.members for v in c]
        return (np.array([v[0] for v in flat], dtype=np.int32), np.array([v[1] for v in flat], dtype=np.int32))

    def ideal_ids(self):
        S = self.sample_count
        return [i for i, c in enumerate(self.members) if len(c) == S and 2 * self.edges[i] == S * (S - 1)]

    def statistics(self):
        """(S, K, components with at least S members, ideal components)."""
        S = self.sample_count
        return (S, len(self), sum(len(c) >= S for c in self.members), len(self.ideal_ids()))

    def multiset(self):
        """Sorted [(members as a tuple, edges)]: what two enumerations of the
        same components agree on."""
        return sorted((tuple(c), e) for c, e in zip(self.members, self.edges))

    def table(self, labels):
        """census.ComponentTable over these arrays (no engine)."""
        from rna_clique_amd.census import ComponentTable
        a = self.arrays()
        ms, mg = self.member_arrays()
        return ComponentTable(a["root_sample"], a["root_gene"], a["nodes"], a["edges"], a["samples"],
                              self.sample_count, labels, ms, mg)


def from_case(case):
    """The census of a post_cases.GraphCase (as component_oracle.from_case)."""
    nodes, edges = case.graph()
    sc = case.sample_count if case.sample_count else po.sample_count(nodes)
    return Census(nodes, edges, sc)
