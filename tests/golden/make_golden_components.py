"""Capture the reference's connected components of the gene matches graph.

TEST INFRASTRUCTURE ONLY -- run where the reference is available, as
make_golden.py:

    python tests/golden/make_golden_components.py

For every case of tests/post_cases.py `fixture_cases()` and the settings
(top_matches, keep_all) of SETTINGS below, the gene matches tables of all pairs
are made by the reference's HomologFinder (make_golden_subsets.reference_tables)
and its build_graph makes the graph. Then the reference's own

  rna_clique.graph.component_subgraphs(graph)           graph.py:9-23
  filtered_distance.get_ideal_components(graph, S)      filtered_distance.py:30-39

run, and tests/golden/component_stats.json gets, per case and setting:
sample_count (distinct samples among the graph's nodes), per component the
sorted [sample index, gene] members and len(component.edges), and the number of
ideal components. The components are stored in the reference's enumeration
order (networkx insertion order); comparisons are between multisets. Data only;
no reference source is copied.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (first: it fixes numpy's sort dispatch before numpy is imported)
import make_golden_subsets  # noqa: E402
import ref_harness  # noqa: E402

import post_cases  # noqa: E402

SETTINGS = [(1, True), (3, True), (3, False)]

# the totals the capture must reproduce: (case, setting) -> (components, ideal components)
EXPECTED_TOTALS = {("threshold-duplicates", "3-True"): (15, 3), ("tie-across-genes", "1-True"): (8, 4),
                   ("family-s2-4x4x3x2", "1-True"): (3, 2)}


def reference_components(case, top_matches, keep_all):
    ref = ref_harness.reference_modules()
    from rna_clique.graph import component_subgraphs
    six = {s: i for i, s in enumerate(case.samples)}
    tables = make_golden_subsets.reference_tables(case, top_matches, keep_all)
    graph = ref.build_graph.build_graph(iter(tables.values()))
    sample_count = len({n[0] for n in graph.nodes})
    comps = [{"members": sorted([six[str(s)], int(g)] for s, g in c.nodes), "edges": len(c.edges)}
             for c in component_subgraphs(graph)]
    ideal = len(list(ref.filtered_distance.get_ideal_components(graph, sample_count)))
    return {"sample_count": sample_count, "components": comps, "ideal_components": ideal}


def main():
    cases = {}
    for case in post_cases.fixture_cases():
        cases[case.name] = {"samples": case.samples,
                            "expected": {f"{t}-{k}": reference_components(case, t, k) for t, k in SETTINGS}}
    for (name, setting), (n_comp, n_ideal) in EXPECTED_TOTALS.items():
        e = cases[name]["expected"][setting]
        assert (len(e["components"]), e["ideal_components"]) == (n_comp, n_ideal), (name, setting)
    path = os.path.join(HERE, "component_stats.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/make_golden_components.py",
                   "reference": "actapia/rna_clique (stub-imported post-alignment modules; build_graph, "
                                "graph.component_subgraphs, filtered_distance.get_ideal_components)",
                   "settings": [list(s) for s in SETTINGS], "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(e["components"]) for c in cases.values() for e in c["expected"].values())
    print(f"wrote {path}: {n} components, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
