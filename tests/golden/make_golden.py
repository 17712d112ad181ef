"""Capture golden vectors for the post-alignment stage from the reference.

TEST INFRASTRUCTURE ONLY -- run in the build container, where /root/reference
exists:

    python tests/golden/make_golden.py

It builds synthetic BLAST-style HSP tables (outfmt 6 columns + gaps nident
sstrand, as `find_homologs.py:124,209` request), feeds them through the
reference's own code (stub-imported by ref_harness.py):

  HomologFinder.get_match_table      find_homologs.py:215-302
  (ssample/qsample labelling)        find_all_pairs.py:82-86
  build_graph                        build_graph.py:40-68
  SampleSimilarity(...).valid        filtered_distance.py:184-196
  SampleSimilarity.restricted        filtered_distance.py:199-210
  get_dissimilarity_df               similarity_computer.py:367-375

and writes inputs + outputs to tests/golden/post_alignment.json. The fixture is
data (inputs and expected outputs); no reference source is copied.

A second file, tests/golden/post_alignment_ties.json, holds the reference's
output on the tie-heavy and crafted cases of tests/post_cases.py
(`fixture_cases()`): groups of up to 16 HSPs with few distinct scores,
top_matches 1, 3 and 5, several rows and edges per item, duplicates at the
nlargest threshold. Each case's hits and transcripts are stored once, with one
`expected` per (top_matches, keep_all) setting.

    python tests/golden/make_golden.py --only ties   # the second file alone
    python tests/golden/make_golden.py --only base   # post_alignment.json alone

Tie order (reference quirk Q2). For a group of at most `n` rows pandas'
nlargest(n) falls back to Series.sort_values, i.e. numpy's default quicksort.
Up to 16 elements that is an insertion sort, which keeps tied rows in frame
order -- unless numpy dispatches to its AVX2 / AVX-512 sorting networks, which
do not: there the order of tied rows (hence the labels after reset_index, and
the row that keep="first" picks) depends on the CPU the reference runs on.
The oracle, post_fast and the engine follow the portable rule (ties in frame
order, the rule of nlargest's own n < len(group) branch), so this script
records the reference with numpy's SIMD sorts switched off
(NPY_DISABLE_CPU_FEATURES, set below before numpy is imported) and, for the
second file, lists under "reference_quirks" the (case, setting) whose tables
come out differently with this machine's SIMD sort.
"""
from __future__ import annotations

import itertools
import json
import math
import os
import sys

PORTABLE_SORT = "AVX2 AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL"
if "--simd-sort" not in sys.argv:
    assert "numpy" not in sys.modules, "run as a script: numpy must not be imported yet"
    os.environ["NPY_DISABLE_CPU_FEATURES"] = PORTABLE_SORT

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # oracle.post_oracle (transcript id parsing)
import ref_harness  # noqa: E402

HSP_COLUMNS = ["qseqid", "sseqid", "pident", "length", "mismatch", "gapopen",
               "qstart", "qend", "sstart", "send", "evalue", "bitscore",
               "gaps", "nident", "sstrand"]
TABLE_COLUMNS = ["pident", "length", "mismatch", "gapopen", "qstart", "qend",
                 "sstart", "send", "evalue", "bitscore", "gaps", "nident",
                 "sstrand", "qgene", "qiso", "sgene", "siso", "reverse",
                 "ssample", "qsample"]


def _tx_name(gene, iso, cov):
    return f"NODE_{gene * 10 + iso}_length_1000_cov_{cov:.6f}_g{gene}_i{iso}"


def make_case(seed, n_samples, n_families, p_present=0.92, p_iso2=0.2,
              p_paralog=0.15, p_asym=0.2, p_minus=0.1, p_drop=0.03):
    """Synthetic HSP tables for every ordered sample pair.

    Families play the role of orthologous gene groups; paralog hits, isoforms,
    F/R bitscore asymmetry and dropped hits create ties, non-ideal components
    and missing pairs.
    """
    rng = np.random.default_rng(seed)
    samples = [f"out/od1/T{i}_top.fasta" for i in range(n_samples)]
    txs = {}       # sample -> list of (gene, iso, family, cov)
    fam_gene = {}  # (sample, family) -> gene
    for si, s in enumerate(samples):
        genes = rng.choice(np.arange(1, 10 * n_families + 1), size=n_families,
                           replace=False)
        lst = []
        for f in range(n_families):
            if rng.random() > p_present:
                continue
            g = int(genes[f])
            fam_gene[(s, f)] = g
            niso = 2 if rng.random() < p_iso2 else 1
            for iso in range(1, niso + 1):
                lst.append((g, iso, f, float(rng.uniform(1, 1000))))
        txs[s] = lst
    # a symmetric "true" bitscore per (family, unordered sample pair)
    base = {}
    for f in range(n_families):
        for a, b in itertools.combinations(samples, 2):
            base[(f, a, b)] = base[(f, b, a)] = float(rng.integers(300, 340) * 3)
    hits = {}
    for q, s in itertools.permutations(samples, 2):
        rows = []
        for (g, iso, f, cov) in txs[q]:
            qrows = []
            if (s, f) in fam_gene:
                sg = fam_gene[(s, f)]
                for (g2, iso2, f2, cov2) in txs[s]:
                    if g2 != sg:
                        continue
                    if rng.random() < p_drop:
                        continue
                    bits = base[(f, q, s)]
                    if rng.random() < p_asym:
                        bits += float(rng.choice([-3.0, -1.0, 1.0, 2.0]))
                    if iso2 > 1 or iso > 1:
                        bits -= float(rng.choice([0.0, 0.0, 1.0]))
                    qrows.append((g2, iso2, cov2, bits))
            if txs[s] and rng.random() < p_paralog:
                g2, iso2, f2, cov2 = txs[s][int(rng.integers(len(txs[s])))]
                top = max([r[3] for r in qrows], default=900.0)
                bits = top if rng.random() < 0.35 else top - float(rng.integers(1, 200))
                qrows.append((g2, iso2, cov2, bits))
            qrows.sort(key=lambda r: -r[3])
            for (g2, iso2, cov2, bits) in qrows:
                length = int(rng.integers(400, 1600))
                gaps = int(rng.choice([0, 0, 0, 1, 2, 5]))
                mism = int(rng.integers(0, 30))
                nident = length - gaps - mism
                minus = rng.random() < p_minus
                qs = int(rng.integers(1, 50))
                ss = int(rng.integers(1, 50))
                rows.append({
                    "qseqid": _tx_name(g, iso, cov),
                    "sseqid": _tx_name(g2, iso2, cov2),
                    "pident": round(100.0 * nident / length, 3),
                    "length": length, "mismatch": mism,
                    "gapopen": min(gaps, int(rng.integers(0, 3))),
                    "qstart": qs, "qend": qs + length - 1,
                    "sstart": ss + length - 1 if minus else ss,
                    "send": ss if minus else ss + length - 1,
                    "evalue": 0.0, "bitscore": bits, "gaps": gaps,
                    "nident": nident, "sstrand": "minus" if minus else "plus",
                })
        hits[(q, s)] = rows
    return samples, hits


def run_reference(samples, hits, top_matches, keep_all):
    import pandas as pd
    ref = ref_harness.reference_modules()
    ref_harness.FAKE_BLAST_DB.clear()
    for (q, s), rows in hits.items():
        ref_harness.FAKE_BLAST_DB[(q, s)] = pd.DataFrame(rows, columns=HSP_COLUMNS)
    parser = ref.transcripts.TranscriptID.parser_from_re(ref.transcripts.default_gene_re)
    out = {"tables": {}, "errors": {}}
    tables = []
    q1_ok = True
    for t1, t2 in itertools.combinations(samples, 2):
        hf = ref.find_homologs.HomologFinder(parser, top_matches, 1e-99, keep_all)
        try:
            table = hf.get_match_table(t1, t2)
        except Exception as e:  # reference failure is recorded, not hidden
            out["errors"][f"{t1}|{t2}"] = f"{type(e).__name__}: {e}"
            continue
        # find_all_pairs.py:82-86
        table["ssample"] = str(t1)
        table["qsample"] = str(t2)
        rows = []
        for label, r in zip(table.index.tolist(), table.to_dict("records")):
            rows.append([int(label)] + [
                (bool(r[c]) if c == "reverse" else
                 (float(r[c]) if c in ("pident", "evalue", "bitscore") else
                  (str(r[c]) if c in ("sstrand", "ssample", "qsample") else int(r[c]))))
                for c in TABLE_COLUMNS])
        out["tables"][f"{t1}|{t2}"] = rows
        if len(table) and 0 not in table.index:
            q1_ok = False  # mapping_from_dfs would raise KeyError: 0 (Q1)
        tables.append((t1, t2, table))
    out["mapping_from_dfs_ok"] = q1_ok
    if out["errors"]:
        return out
    graph = ref.build_graph.build_graph(t for (_, _, t) in tables)
    edges = sorted(sorted([list(u), list(v)]) for u, v in graph.edges)
    out["edges"] = edges
    out["nodes"] = sorted(list(n) for n in graph.nodes)
    # Pair keys taken from the pair itself (Q1: mapping_from_dfs uses a label
    # lookup that fails when row 0 was filtered out).
    sim = ref.filtered_distance.SampleSimilarity(
        graph, [(frozenset((t2, t1)), t) for (t1, t2, t) in tables])
    out["sample_count"] = int(sim.sample_count)
    out["valid"] = sorted([str(s), int(g)] for s, g in
                          sim.valid.itertuples(index=False))
    sums = {}
    for t1, t2, t in tables:
        r = sim.restricted(t)
        sums[f"{t1}|{t2}"] = [int(r["nident"].sum()),
                              int(r["length"].sum() - r["gaps"].sum())]
    out["sums"] = sums
    try:
        df = sim.get_dissimilarity_df()
        out["matrix"] = {"labels": [str(x) for x in df.index],
                         "values": df.values.tolist()}
    except ref.filtered_distance.NoIdealComponentsError:
        out["matrix"] = None
        out["errors"]["matrix"] = "NoIdealComponentsError"
    return out


def no_ideal_case():
    """3 samples whose only component has 4 vertices: no ideal components,
    so the reference raises NoIdealComponentsError (filtered_distance.py:242-247)."""
    A, B, C = [f"out/od1/T{i}_top.fasta" for i in range(3)]

    def row(qg, sg, bits):
        return {"qseqid": _tx_name(qg, 1, 5.0), "sseqid": _tx_name(sg, 1, 5.0),
                "pident": 99.0, "length": 500, "mismatch": 5, "gapopen": 0,
                "qstart": 1, "qend": 500, "sstart": 1, "send": 500,
                "evalue": 0.0, "bitscore": bits, "gaps": 0, "nident": 495,
                "sstrand": "plus"}
    hits = {(B, A): [row(2, 1, 900.0)], (A, B): [row(1, 2, 900.0)],
            (C, B): [row(3, 2, 900.0)], (B, C): [row(2, 3, 900.0)],
            (C, A): [row(4, 1, 900.0)], (A, C): [row(1, 4, 900.0)]}
    return [A, B, C], hits


CASES = [
    # (seed, samples, families)
    (11, 3, 12),
    (12, 4, 25),
    (13, 4, 40),
    (14, 5, 30),
    (15, 3, 8),
    (16, 6, 20),
]
PARAMS = [(1, True), (1, False), (2, True)]


def _compact(hits):
    return {f"{q}|{s}": [[r[c] for c in HSP_COLUMNS] for r in rows]
            for (q, s), rows in hits.items()}


def main():
    fixtures = []
    for seed, ns, nf in CASES:
        samples, hits = make_case(seed, ns, nf)
        for top_matches, keep_all in PARAMS:
            res = run_reference(samples, hits, top_matches, keep_all)
            fixtures.append({
                "seed": seed, "top_matches": top_matches, "keep_all": keep_all,
                "samples": samples,
                "hits": _compact(hits),
                "expected": res,
            })
    # A case with one empty directed search and one with no ideal components.
    samples, hits = make_case(21, 3, 6, p_present=1.0)
    q, s = samples[2], samples[0]
    hits[(q, s)] = []
    fixtures.append({"seed": 21, "top_matches": 1, "keep_all": True,
                     "samples": samples,
                     "hits": _compact(hits),
                     "expected": run_reference(samples, hits, 1, True)})
    samples, hits = no_ideal_case()
    fixtures.append({"seed": 22, "top_matches": 1, "keep_all": True,
                     "samples": samples,
                     "hits": _compact(hits),
                     "expected": run_reference(samples, hits, 1, True)})
    path = os.path.join(HERE, "post_alignment.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/make_golden.py",
                   "reference": "actapia/rna_clique (stub-imported post-alignment modules)",
                   "columns": ["label"] + TABLE_COLUMNS,
                   "hsp_columns": HSP_COLUMNS,
                   "fixtures": fixtures}, f, separators=(",", ":"))
    print(f"wrote {path}: {len(fixtures)} fixtures, "
          f"{os.path.getsize(path) / 1e3:.0f} kB")
    for fx in fixtures:
        e = fx["expected"]
        print(fx["seed"], fx["top_matches"], fx["keep_all"], "tables",
              sum(len(v) for v in e["tables"].values()), "errors", e["errors"],
              "q1ok", e.get("mapping_from_dfs_ok"),
              "valid", len(e.get("valid", [])))


def _tables_digest(res):
    import hashlib
    return hashlib.sha256(json.dumps(res["tables"], sort_keys=True).encode()).hexdigest()


def simd_digests():
    """--simd-sort: the tables' digests per (case, setting) with numpy's own
    sort dispatch (no NPY_DISABLE_CPU_FEATURES), printed as JSON."""
    import post_cases
    out = {}
    for case in post_cases.fixture_cases():
        for top_matches, keep_all in post_cases.FIXTURE_SETTINGS:
            res = run_reference(case.samples, case.hits, top_matches, keep_all)
            out[f"{case.name} {top_matches}-{keep_all}"] = _tables_digest(res)
    return out


def main_ties():
    import subprocess
    import post_cases
    env = {k: v for k, v in os.environ.items() if k != "NPY_DISABLE_CPU_FEATURES"}
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--simd-sort"], env=env, check=True,
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    simd = json.loads(child.stdout.strip().splitlines()[-1])
    differs = []
    fixtures = []
    for case in post_cases.fixture_cases():
        assert all(case.hits.values()), "no empty searches in captured cases"
        expected = {}
        for top_matches, keep_all in post_cases.FIXTURE_SETTINGS:
            res = run_reference(case.samples, case.hits, top_matches, keep_all)
            assert not any(k != "matrix" for k in res["errors"]), (case.name, res["errors"])
            expected[f"{top_matches}-{keep_all}"] = json.loads(json.dumps(res))
            if simd[f"{case.name} {top_matches}-{keep_all}"] != _tables_digest(res):
                differs.append(f"{case.name} {top_matches}-{keep_all}")
        packed = json.loads(json.dumps(post_cases.pack_fixture(case, expected)))
        # the stored form loses nothing: it unpacks to the inputs and to what the reference returned
        back = post_cases.unpack_fixture(packed)
        assert back["expected"] == expected and back["hits"] == case.hits and back["transcripts"] == case.transcripts
        fixtures.append(packed)
    assert ["label"] + TABLE_COLUMNS == post_cases.TABLE_COLUMNS and HSP_COLUMNS == post_cases.HSP_COLUMNS
    path = os.path.join(HERE, "post_alignment_ties.json")
    head = {"generator": "tests/golden/make_golden.py --only ties (cases and stored form: tests/post_cases.py)",
            "reference": "actapia/rna_clique (stub-imported post-alignment modules)",
            "id_format": post_cases.ID_FORMAT,
            "hit_columns": post_cases.HIT_STORED,
            "table_row": ["label", "reverse", "index of the HSP in its search"],
            "settings": [list(s) for s in post_cases.FIXTURE_SETTINGS],
            "reference_quirks": {"Q2_unstable_tie_order": {
                "recorded_with": "NPY_DISABLE_CPU_FEATURES=" + PORTABLE_SORT,
                "tables_differ_with_simd_sort": differs}}}
    with open(path, "w") as f:
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"fixtures":[\n')
        f.write(",\n".join(json.dumps(fx, separators=(",", ":")) for fx in fixtures) + "\n]}\n")
    print(f"wrote {path}: {len(fixtures)} fixtures, {os.path.getsize(path) / 1e3:.0f} kB")
    print("tables that differ with this machine's SIMD sort (Q2):", differs)
    for fx in fixtures:
        for key, e in fx["expected"].items():
            print(fx["name"], key, "hsps", sum(len(v) for v in fx["hits"].values()), "table rows",
                  sum(len(v) for v in e["tables"].values()), "q1ok", e["mapping_from_dfs_ok"], "valid", len(e["valid"]))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", choices=["base", "ties"], help="write one of the two files (default: both)")
    ap.add_argument("--simd-sort", action="store_true", help="print the ties cases' table digests under numpy's "
                    "own sort dispatch (used by the ties capture itself)")
    args = ap.parse_args()
    if args.simd_sort:
        print(json.dumps(simd_digests()))
        sys.exit(0)
    only = args.only
    if only != "ties":
        main()
    if only != "base":
        main_ties()
