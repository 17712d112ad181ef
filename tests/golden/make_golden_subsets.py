"""Capture the reference's results on subsets of samples.

TEST INFRASTRUCTURE ONLY -- run where the reference is available, as
make_golden.py:

    python tests/golden/make_golden_subsets.py

For the 4-sample tie fixture of tests/post_cases.py (`fixture_cases()`, the
case stored in post_alignment_ties.json) and the two settings of
subset_cases.SUBSET_SETTINGS, the gene matches tables of all six pairs are made
once by the reference's HomologFinder. Then, for every subset of at least two
samples, the reference's own subset workflow runs on the tables whose two
samples are both kept (what make_subset links, make_subset.py:166-201):

  build_graph(kept tables)                        build_graph.py:40-68
  SampleSimilarity(graph, kept tables)            filtered_distance.py:162-247
    .sample_count / .valid / .restricted(table) / .get_dissimilarity_df()

and tests/golden/subsets.json gets, per setting and subset (keyed by the
sample indices, "0-2-3"): sample_count, the valid nodes as [sample index,
gene], the restricted sums per kept pair and the matrix (null where the
reference raises NoIdealComponentsError). Data only; no reference source is
copied.
"""
from __future__ import annotations

import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (first: it fixes numpy's sort dispatch before numpy is imported)
import ref_harness  # noqa: E402

import post_cases  # noqa: E402
import subset_cases  # noqa: E402


def reference_tables(case, top_matches, keep_all):
    """{(t1, t2): the reference's gene matches table}, every pair of the case."""
    import pandas as pd
    ref = ref_harness.reference_modules()
    ref_harness.FAKE_BLAST_DB.clear()
    for (q, s), rows in case.hits.items():
        ref_harness.FAKE_BLAST_DB[(q, s)] = pd.DataFrame(rows, columns=make_golden.HSP_COLUMNS)
    parser = ref.transcripts.TranscriptID.parser_from_re(ref.transcripts.default_gene_re)
    tables = {}
    for t1, t2 in itertools.combinations(case.samples, 2):
        table = ref.find_homologs.HomologFinder(parser, top_matches, 1e-99, keep_all).get_match_table(t1, t2)
        table["ssample"] = str(t1)   # find_all_pairs.py:82-86
        table["qsample"] = str(t2)
        tables[(t1, t2)] = table
    return tables


def reference_subset(case, tables, ids):
    ref = ref_harness.reference_modules()
    six = {s: i for i, s in enumerate(case.samples)}
    kept = [(t1, t2, t) for (t1, t2), t in tables.items() if six[t1] in ids and six[t2] in ids]
    graph = ref.build_graph.build_graph(t for _, _, t in kept)
    sim = ref.filtered_distance.SampleSimilarity(graph, [(frozenset((t2, t1)), t) for t1, t2, t in kept])
    out = {"sample_count": int(sim.sample_count),
           "valid": sorted([six[str(s)], int(g)] for s, g in sim.valid.itertuples(index=False)), "sums": {}}
    for t1, t2, t in kept:
        r = sim.restricted(t)
        out["sums"][f"{six[t1]}-{six[t2]}"] = [int(r["nident"].sum()), int(r["length"].sum() - r["gaps"].sum())]
    try:
        df = sim.get_dissimilarity_df()
        out["matrix"] = {"labels": [six[str(x)] for x in df.index], "values": df.values.tolist()}
    except ref.filtered_distance.NoIdealComponentsError:
        out["matrix"] = None
    return out


def main():
    case = next(c for c in post_cases.fixture_cases() if c.name.startswith("family") and len(c.samples) == 4)
    expected = {}
    for top_matches, keep_all in subset_cases.SUBSET_SETTINGS:
        tables = reference_tables(case, top_matches, keep_all)
        expected[f"{top_matches}-{keep_all}"] = {
            subset_cases.subset_key(ids): reference_subset(case, tables, ids)
            for ids in subset_cases.all_subsets(len(case.samples))}
    path = os.path.join(HERE, "subsets.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/make_golden_subsets.py",
                   "reference": "actapia/rna_clique (stub-imported post-alignment modules; build_graph + "
                                "SampleSimilarity over the kept tables of each subset)",
                   "fixture": case.name, "samples": case.samples,
                   "settings": [list(s) for s in subset_cases.SUBSET_SETTINGS], "expected": expected}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {sum(len(v) for v in expected.values())} subsets, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
