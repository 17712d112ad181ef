"""The component census of a gene matches graph: one row per connected
component, ideal or not, and the members of each.

The integers come from the engine (Engine.components(),
Engine.component_members(): the census is built on the GPU from the finished
graph phase); everything else here is derived from them on the host. It is the
data behind the reference's plot_component_sizes -- the component size
histogram, the represented-sample-count histogram, the samples / size ratio,
the component density and the four numbers of its --statistics -- plus the
answer to "which sample keeps components from being ideal". Drawing is left to
the caller.

Components are numbered in ascending order of their lowest (sample id, gene
id) node in the engine's sample order, the rule of the ideal component ids;
not the reference's order (networkx follows insertion order).
"""
from __future__ import annotations

import numpy as np


class ComponentTable:
    """root_sample, root_gene, nodes, edges, samples: arrays of length K (one
    row per component); sample_count: the S of the ideal test; labels: the
    sample label of each sample id; member_sample, member_gene: every graph
    node sorted by (component, sample id, gene id), so component c owns
    offsets[c]:offsets[c + 1]."""

    def __init__(self, root_sample, root_gene, nodes, edges, samples, sample_count, labels, member_sample,
                 member_gene):
        self.root_sample = np.asarray(root_sample, dtype=np.int32)
        self.root_gene = np.asarray(root_gene, dtype=np.int32)
        self.nodes = np.asarray(nodes, dtype=np.int64)
        self.edges = np.asarray(edges, dtype=np.int64)
        self.samples = np.asarray(samples, dtype=np.int32)
        self.sample_count = int(sample_count)
        self.labels = [str(x) for x in labels]
        self.member_sample = np.asarray(member_sample, dtype=np.int32)
        self.member_gene = np.asarray(member_gene, dtype=np.int32)
        k = len(self.nodes)
        if not (len(self.root_sample) == len(self.root_gene) == len(self.edges) == len(self.samples) == k):
            raise ValueError("the component columns differ in length")
        if len(self.member_sample) != len(self.member_gene) or len(self.member_sample) != int(self.nodes.sum()):
            raise ValueError("the members are not the sum of the component sizes")
        self.offsets = np.concatenate([[0], np.cumsum(self.nodes)]).astype(np.int64)

    @classmethod
    def from_engine(cls, engine):
        """The census of a finished engine (after run(), finish() on one
        shard, or import_edges())."""
        t = engine.components()
        ms, mg = engine.component_members()
        return cls(t["root_sample"], t["root_gene"], t["nodes"], t["edges"], t["samples"],
                   engine.stats()["sample_count"], engine.labels, ms, mg)

    def __len__(self):
        return len(self.nodes)

    # ------------------------------------------------------ derived columns
    @property
    def present_samples(self):
        """P: the number of distinct samples among the graph's nodes."""
        return len(np.unique(self.member_sample))

    @property
    def complete(self):
        """Every pair of members is joined: 2 edges == nodes (nodes - 1)."""
        return 2 * self.edges == self.nodes * (self.nodes - 1)

    @property
    def single_copy(self):
        """No sample has two members: samples == nodes."""
        return self.samples.astype(np.int64) == self.nodes

    @property
    def ideal(self):
        """The engine's ideal test: nodes == sample_count and complete."""
        return (self.nodes == self.sample_count) & self.complete

    @property
    def large(self):
        """At least as many members as samples (the reference's "Components
        >= samples")."""
        return self.nodes >= self.sample_count

    @property
    def one_short(self):
        """A complete single-copy component over all present samples but
        one."""
        return self.complete & self.single_copy & (self.nodes == self.present_samples - 1)

    @property
    def ratio(self):
        """samples / nodes."""
        return self.samples / self.nodes

    @property
    def density(self):
        """2 edges / (nodes (nodes - 1)), the true division of the two
        integers; NaN for a one-node component."""
        out = np.full(len(self), np.nan)
        d = self.nodes * (self.nodes - 1)
        ok = d != 0
        out[ok] = (2 * self.edges[ok]) / d[ok]
        return out

    # ------------------------------------------------------------ summaries
    def statistics(self):
        """(samples, total components, components with at least as many
        members as samples, ideal components): the reference's --statistics,
        in its order."""
        return (self.sample_count, len(self), int(self.large.sum()), int(self.ideal.sum()))

    def size_histogram(self):
        """hist[n] = components with n members, n from 0 to the largest size
        (the bar to highlight is sample_count)."""
        return np.bincount(self.nodes) if len(self) else np.zeros(1, dtype=np.int64)

    def sample_histogram(self):
        """hist[k] = components with members of k distinct samples."""
        return np.bincount(self.samples) if len(self) else np.zeros(1, dtype=np.int64)

    def missing_sample_counts(self):
        """Series by sample label: the number of one_short components that
        lack that sample -- a lower bound on the ideal components gained by
        dropping it (the exact gain needs the graph of the remaining
        samples)."""
        import pandas as pd
        counts = np.zeros(len(self.labels), dtype=np.int64)
        present = np.unique(self.member_sample)
        for c in np.flatnonzero(self.one_short):
            have = self.member_sample[self.offsets[c]:self.offsets[c + 1]]
            missing = np.setdiff1d(present, have)
            assert len(missing) == 1
            counts[missing[0]] += 1
        return pd.Series(counts, index=self.labels, name="one_short")

    # --------------------------------------------------------------- tables
    def members_of(self, ids=None):
        """DataFrame component, sample (label), gene of the given components
        (ids in the order given, or a boolean mask such as `ideal`; default:
        all)."""
        import pandas as pd
        ids = np.arange(len(self)) if ids is None else np.atleast_1d(np.asarray(ids))
        ids = np.flatnonzero(ids) if ids.dtype == bool else ids.astype(np.int64)
        idx = [np.arange(self.offsets[c], self.offsets[c + 1]) for c in ids.tolist()]
        idx = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
        comp = np.repeat(ids, self.nodes[ids]) if len(ids) else np.zeros(0, dtype=np.int64)
        return pd.DataFrame({"component": comp.astype(np.int64),
                             "sample": [self.labels[i] for i in self.member_sample[idx].tolist()],
                             "gene": self.member_gene[idx].astype(np.int64)}, columns=["component", "sample", "gene"])

    def to_frame(self):
        """One row per component: the root, the integers and every derived
        column."""
        import pandas as pd
        return pd.DataFrame({
            "component": np.arange(len(self), dtype=np.int64),
            "root_sample": [self.labels[i] for i in self.root_sample.tolist()],
            "root_gene": self.root_gene.astype(np.int64), "nodes": self.nodes, "edges": self.edges,
            "samples": self.samples.astype(np.int64), "complete": self.complete, "single_copy": self.single_copy,
            "ideal": self.ideal, "large": self.large, "one_short": self.one_short, "ratio": self.ratio,
            "density": self.density})
