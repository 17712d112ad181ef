"""Time the component census at C3 size.

A graph-only engine of 32 samples x 50 000 genes: 50 000 cliques with one gene
per sample, in fifths ideal, one short (one sample's gene left out, the sample
rotating), incomplete (one edge left out) and joined (two complete cliques
with one extra edge between them: one component of 64 nodes) -- the kinds of
post_cases.cliques_case, in vectorised numpy, seeded, pair-major. About 24.3 M
edge records.

Timed with time.perf_counter around blocking calls (each ends in a stream
synchronise), after a warm-up on another engine, 5 times on fresh imports:

* the first Engine.components() + component_members() after import_edges:
  the build on the device (scan, keys, sort, table, members) plus the download;
* the second: the download alone.

For scale, the host time of the networkx statement the tests use
(connected_components, then subgraph(c).number_of_edges() and the distinct
samples per component) on the same kind of graph at 1/10 of the cliques.

    python scripts/census_bench.py [--samples 32] [--cliques 50000] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rna_clique_amd import _native as nat   # noqa: E402
from rna_clique_amd.census import ComponentTable   # noqa: E402
from rna_clique_amd.engine import Engine   # noqa: E402

KINDS = 5   # clique k is of kind k % 5: ideal, one short, incomplete, joined (two of them)


def mixed_records(n_samples, n_cliques, pair_order, seed=0):
    """Pair-major records; gene k of sample s is global gene s * n_cliques + k."""
    assert n_cliques % KINDS == 0 and n_samples >= 3
    rng = np.random.default_rng(seed)
    k = np.arange(n_cliques, dtype=np.int64)
    kind = k % KINDS
    skip = np.where(kind == 1, (k // KINDS) % n_samples, -1)                 # one short: the sample left out
    drop = np.where(kind == 2, (k // KINDS) % len(pair_order), -1)           # incomplete: the pair left out
    parts = []
    for p, (a, b) in enumerate(pair_order):
        keep = (skip != a) & (skip != b) & (drop != p)
        kk = k[keep]
        blk = np.zeros(len(kk), dtype=nat.EDGE_RECORD_DTYPE)
        blk["a"], blk["b"], blk["pair"] = a * n_cliques + kk, b * n_cliques + kk, p
        if (a, b) == (0, 1):   # the joining edges: sample 0 of clique k to sample 1 of clique k + 1
            j = k[kind == 3]
            ext = np.zeros(len(j), dtype=nat.EDGE_RECORD_DTYPE)
            ext["a"], ext["b"], ext["pair"] = j, n_cliques + j + 1, p
            blk = np.concatenate([blk, ext])
        num = rng.integers(200, 3000, size=len(blk), dtype=np.int32)
        blk["nident"] = num
        blk["den"] = num + rng.integers(0, 60, size=len(blk), dtype=np.int32)
        parts.append(blk)
    return np.concatenate(parts)


def expected_statistics(n_samples, n_cliques):
    f = n_cliques // KINDS
    # ideal, one short, incomplete, one joined component per two cliques
    return (n_samples, 4 * f, 3 * f, f)


def new_engine(n_samples, n_cliques):
    eng = Engine(device=0)
    for s in range(n_samples):
        eng.add_sample(f"S{s:02d}", np.zeros(0, np.uint8), np.zeros(n_cliques + 1, np.uint64),
                       np.arange(1, n_cliques + 1, dtype=np.int32), np.ones(n_cliques, np.int32))
    return eng


def census(eng):
    t0 = time.perf_counter()
    t = eng.components()
    m = eng.component_members()
    return time.perf_counter() - t0, t, m


def spread(ts):
    return f"median {statistics.median(ts) * 1e3:.2f} ms, min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f} (n = {len(ts)})"


def networkx_statement(recs, n_cliques):
    import networkx as nx
    t0 = time.perf_counter()
    g = nx.Graph()
    g.add_edges_from(zip(recs["a"].tolist(), recs["b"].tolist()))
    t_graph = time.perf_counter() - t0
    t0 = time.perf_counter()
    rows = []
    for c in nx.connected_components(g):
        rows.append((min(c), len(c), g.subgraph(c).number_of_edges(), len({v // n_cliques for v in c})))
    return t_graph, time.perf_counter() - t0, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--cliques", type=int, default=50000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-fraction", type=int, default=10, help="networkx on 1/N of the cliques (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, C = a.samples, a.cliques
    warm = new_engine(4, 50)
    warm.import_edges(mixed_records(4, 50, warm.pair_order()).view(np.uint8))
    census(warm)
    warm.close()
    eng = new_engine(N, C)
    recs = mixed_records(N, C, eng.pair_order())
    say(f"census_bench: {N} samples x {C} genes, {len(recs)} edge records")
    first, second = [], []
    for _ in range(a.runs):
        eng.import_edges(recs.view(np.uint8))
        t1, _, _ = census(eng)
        t2, tab, mem = census(eng)
        first.append(t1)
        second.append(t2)
    st = eng.stats()
    table = ComponentTable.from_engine(eng)
    assert table.statistics() == expected_statistics(N, C), table.statistics()
    assert int(table.one_short.sum()) == C // KINDS and int(tab["nodes"].sum()) == len(mem[0]) == st["nodes"]
    say(f"components {st['components']}, nodes {st['nodes']}, statistics {table.statistics()}, "
        f"one short {int(table.one_short.sum())}")
    say(f"first components() + component_members() after import_edges (build + download): {spread(first)}")
    say(f"second call (download: {20 * st['components'] + 4 * st['nodes']} bytes from the device): {spread(second)}")
    eng.close()
    if a.host_fraction:
        c10 = C // a.host_fraction // KINDS * KINDS
        e10 = new_engine(N, c10)
        r10 = mixed_records(N, c10, e10.pair_order())
        e10.import_edges(r10.view(np.uint8))
        _, t10, _ = census(e10)
        e10.close()
        t_graph, t_stmt, rows = networkx_statement(r10, c10)
        rows.sort()
        same = ([r[1] for r in rows] == t10["nodes"].tolist() and [r[2] for r in rows] == t10["edges"].tolist() and
                [r[3] for r in rows] == t10["samples"].tolist())
        say(f"networkx on the host at 1/{a.host_fraction} of the size ({N} samples x {c10} genes, {len(r10)} edges): "
            f"components, edge and sample counts {t_stmt * 1e3:.0f} ms (after {t_graph * 1e3:.0f} ms to build the "
            f"Graph); same table as the engine: {same}")
        if not same:
            raise SystemExit("the engine and networkx disagree")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
