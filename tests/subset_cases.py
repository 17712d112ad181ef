"""Subsets of samples and their expected results, shared by
tests/test_subsets_host.py and tests/golden/make_golden_subsets.py. A plain
module: no fixtures, no GPU.

What the reference computes for a subset of the samples (make_subset.py:166-201:
link the gene matches tables whose two samples are both kept; then build_graph
over those tables and SampleSimilarity on that graph, subset_comparisons.py:
45-73) is not a sub-matrix of the full run: components are those of the
induced graph, the ideal test's sample count is the distinct samples among
that graph's nodes, so other components are ideal. The oracle's statement of
it is post_oracle.run_pipeline on the subset's samples only, in their input
order (`oracle_subset`).
"""
from __future__ import annotations

import itertools

from oracle import post_oracle as po

# (top_matches, keep_all) of the recorded subset results: one keep_all and one
# keep-first setting of post_alignment_ties.json
SUBSET_SETTINGS = [(3, True), (3, False)]


def all_subsets(n, smallest=2):
    """Every subset of range(n) with at least `smallest` members, by size."""
    return [list(c) for k in range(smallest, n + 1) for c in itertools.combinations(range(n), k)]


def subset_key(ids):
    return "-".join(str(i) for i in ids)


def oracle_subset(samples, hits, ids, top, keep):
    """The oracle on the subset's samples only: {"sample_count", "nodes",
    "edges", "components", "valid" [[label, gene]] sorted, "sums" / "usums"
    {"a-b" sample indices: [num, den]}, "matrix" {"labels", "values"} or None}."""
    labs = [samples[i] for i in ids]
    res = po.run_pipeline(labs, hits, po.default_parse_id, top, keep)
    comps, _ = po.components(set(res["nodes"]), set(res["edges"]))
    key = lambda t1, t2: f"{samples.index(t1)}-{samples.index(t2)}"   # noqa: E731
    try:
        labels, values = po.distance_matrix(labs, res["sums"])
        matrix = {"labels": labels, "values": values}
    except po.NoIdealComponentsError:
        matrix = None
    return {"sample_count": res["sample_count"], "nodes": len(res["nodes"]), "edges": len(res["edges"]),
            "components": len(comps), "valid": sorted([s, g] for s, g in res["valid"]),
            "sums": {key(*k): list(v) for k, v in res["sums"].items()},
            "usums": {key(*k): [sum(r["nident"] for r in rows), sum(r["length"] - r["gaps"] for r in rows)]
                      for k, rows in res["tables"].items()},
            "matrix": matrix}
