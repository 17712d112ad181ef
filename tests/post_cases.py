"""Deterministic inputs for the post-alignment stage (RBH tables -> graph ->
ideal filter -> sums -> distances), shared by the CPU golden tests, the GPU
tests and tests/golden/make_golden.py. A plain module: no fixtures, no GPU.

Two kinds of input:

* HSP cases (`Case`): samples with an explicit transcript list (gene, isoform)
  and, per directed search (query sample, subject sample), the HSP rows in
  BLAST output order -- as the dicts `post_oracle.parse_hits` takes
  (`Case.hits`) and as `HSP_DTYPE` arrays for `Engine.add_hsps`
  (`Case.hsp_arrays()`). `family_case` draws tie-heavy random tables; the three
  `crafted_*` cases pin one selection rule each.
* Graph record cases (`GraphCase`): `EDGE_RECORD_DTYPE` arrays for
  `Engine.import_edges`, together with the same graph as (sample, gene) nodes,
  edges and per-record sums for `post_oracle.components` / `ideal_nodes`.
"""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

TIE_SCORES = [100.0, 250.5, 250.5, 400.0, 401.5]   # one decimal: bits10 is exact


ID_FORMAT = "T_cov_1.0_g{gene}_i{iso}"


def tx_id(gene, iso):
    """A transcript id that the reference's default regex parses."""
    return ID_FORMAT.format(gene=gene, iso=iso)


def sample_label(i):
    return f"out/od1/T{i}_top.fasta"


class Case:
    """samples: labels in input order; transcripts[label]: [(gene, iso)] in
    transcript order; hits[(query label, subject label)]: HSP dicts."""

    def __init__(self, name, samples, transcripts, hits):
        self.name = name
        self.samples = list(samples)
        self.transcripts = {s: list(t) for s, t in transcripts.items()}
        self.hits = hits

    def n_hsps(self):
        return sum(len(v) for v in self.hits.values())

    def hsp_arrays(self):
        """{(query index, subject index): HSP_DTYPE array}, transcript indices
        local to each sample's transcript list."""
        from rna_clique_amd._native import HSP_DTYPE
        from oracle.post_oracle import default_parse_id
        tix = {s: {gi: k for k, gi in enumerate(t)} for s, t in self.transcripts.items()}
        out = {}
        for (q, s), rows in self.hits.items():
            arr = np.zeros(len(rows), dtype=HSP_DTYPE)
            for i, h in enumerate(rows):
                _, qg, qi = default_parse_id(h["qseqid"])
                _, sg, si = default_parse_id(h["sseqid"])
                arr[i]["q_tx"] = tix[q][(qg, qi)]
                arr[i]["s_tx"] = tix[s][(sg, si)]
                for f in ("qstart", "qend", "sstart", "send", "length", "nident", "mismatch", "gaps", "gapopen"):
                    arr[i][f] = h[f]
                b10 = int(round(h["bitscore"] * 10))
                assert b10 / 10.0 == h["bitscore"], "bit scores carry one decimal"
                arr[i]["bits10"] = b10
                arr[i]["strand"] = 1 if h["sstrand"] == "minus" else 0
            out[(self.samples.index(q), self.samples.index(s))] = arr
        return out


def _hsp(rng, q, s, bits):
    """One HSP row between transcripts q and s ((gene, iso) each): random
    length, gaps, mismatches and strand; nident = length - gaps - mismatch."""
    length = int(rng.integers(30, 900))
    gaps = int(rng.integers(0, 4))
    mism = int(rng.integers(0, 9))
    nident = length - gaps - mism
    minus = bool(rng.random() < 0.3)
    qs, ss = int(rng.integers(1, 50)), int(rng.integers(1, 50))
    return {"qseqid": tx_id(*q), "sseqid": tx_id(*s), "pident": round(100.0 * nident / length, 3),
            "length": length, "mismatch": mism, "gapopen": min(gaps, int(rng.integers(0, 3))),
            "qstart": qs, "qend": qs + length - 1,
            "sstart": ss + length - 1 if minus else ss, "send": ss if minus else ss + length - 1,
            "evalue": 0.0, "bitscore": float(bits), "gaps": gaps, "nident": nident,
            "sstrand": "minus" if minus else "plus"}


def family_case(seed, n_samples, n_families, n_iso, max_hsps, scores=TIE_SCORES, p_paralog=0.3,
                p_empty=0.05, n_silent=3, unhit_sample=False):
    """Gene family f has one gene with n_iso isoforms in every sample (its gene
    id differs from sample to sample). Every (query transcript, subject
    transcript) of a family gets 0..max_hsps HSPs; with probability p_paralog
    a query transcript also hits a transcript of a random other gene. Scores
    come from the short list `scores`. A directed search is empty with
    probability p_empty. Every sample also has n_silent genes without HSPs;
    unhit_sample adds a last sample that no search touches."""
    rng = np.random.default_rng(seed)
    samples = [sample_label(i) for i in range(n_samples + (1 if unhit_sample else 0))]
    transcripts, fam_gene = {}, {}
    for s in samples:
        ids = rng.permutation(np.arange(1, n_families + n_silent + 1))
        fam_gene[s] = [int(g) for g in ids[:n_families]]
        tx = [(int(g), i) for g in ids for i in range(1, n_iso + 1)]
        transcripts[s] = [tx[k] for k in rng.permutation(len(tx))]
    live = samples[:n_samples]
    hits = {}
    for q, s in itertools.permutations(samples, 2):
        rows = []
        if q in live and s in live and rng.random() >= p_empty:
            gene_fam = {g: f for f, g in enumerate(fam_gene[q])}
            for (g, iso) in transcripts[q]:
                if g not in gene_fam:
                    continue
                block = []
                sg = fam_gene[s][gene_fam[g]]
                for iso2 in range(1, n_iso + 1):
                    for _ in range(int(rng.integers(0, max_hsps + 1))):
                        block.append(_hsp(rng, (g, iso), (sg, iso2), rng.choice(scores)))
                if rng.random() < p_paralog and n_families > 1:
                    og = sg
                    while og == sg:
                        og = fam_gene[s][int(rng.integers(n_families))]
                    block.append(_hsp(rng, (g, iso), (og, int(rng.integers(1, n_iso + 1))), rng.choice(scores)))
                rows.extend(block[k] for k in rng.permutation(len(block)))
        hits[(q, s)] = rows
    name = f"family-s{seed}-{n_samples}x{n_families}x{n_iso}x{max_hsps}" + ("-unhit" if unhit_sample else "")
    return Case(name, samples, transcripts, hits)


# The four parametrised shapes (samples, families, isoforms, max HSPs) and the
# seed used for each: seeds are chosen so that post_oracle finds an ideal
# component at every top_matches setting (checked by the CPU test
# test_family_shapes_force_their_paths).
FAMILY_SHAPES = {
    "ties": (3, 40, 2, 2),          # general ties, groups up to ~13 HSPs
    "large-groups": (4, 30, 3, 2),  # groups of 20+ HSPs
    "spans-blocks": (2, 300, 1, 3),  # > 256 items in one pair: the pair spans blocks
    "many-pairs": (5, 20, 2, 1),    # 200 items of 10 pairs inside one 256-thread block
}
FAMILY_SEEDS = {"ties": 1, "large-groups": 1, "spans-blocks": 0, "many-pairs": 23}


def family_shape_case(shape):
    ns, nf, ni, mh = FAMILY_SHAPES[shape]
    return family_case(FAMILY_SEEDS[shape], ns, nf, ni, mh)


class _Builder:
    """Hand-placed HSPs: add() appends one HSP to a directed search and
    registers both transcripts."""

    def __init__(self, name, n_samples, seed):
        self.name = name
        self.rng = np.random.default_rng(seed)
        self.samples = [sample_label(i) for i in range(n_samples)]
        self.tx = {s: [] for s in self.samples}
        self.hits = {p: [] for p in itertools.permutations(self.samples, 2)}

    def add(self, q, qt, s, st, bits):
        qs, ss = self.samples[q], self.samples[s]
        for lab, t in ((qs, qt), (ss, st)):
            if t not in self.tx[lab]:
                self.tx[lab].append(t)
        self.hits[(qs, ss)].append(_hsp(self.rng, qt, st, bits))

    def both(self, a, at, b, bt, bits):
        self.add(a, at, b, bt, bits)
        self.add(b, bt, a, at, bits)

    def orthologs(self, genes, bits0):
        """One-to-one reciprocal hits of gene g between all samples, one score
        per (gene, pair): ideal components for the graph phase to find."""
        n = len(self.samples)
        for k, g in enumerate(genes):
            for a, b in itertools.combinations(range(n), 2):
                self.both(a, (g, 1), b, (g, 1), bits0 + 3 * k + a + 2 * b)

    def case(self):
        return Case(self.name, self.samples, self.tx, self.hits)


def crafted_tie_across_genes():
    """One query gene's maximum is shared by rows of two subject genes, both
    reciprocated: the item has 2 edges with keep_all=True, and with
    keep_all=False the first row in the reference's order survives alone.
    Table (S0, S1): forward = query S1, subject S0."""
    b = _Builder("tie-across-genes", 3, 101)
    b.orthologs([1, 2, 3, 4], 300.0)
    # S1 g10 -> S0 g12 and g11 at 400 (g12 first in output order: the table
    # orders pairs by gene, not by output order); both hit back at 400
    b.add(1, (10, 1), 0, (12, 1), 400.0)
    b.add(1, (10, 1), 0, (11, 1), 400.0)
    b.add(0, (11, 1), 1, (10, 1), 400.0)
    b.add(0, (12, 1), 1, (10, 1), 400.0)
    # S1 g20: two isoforms' rows to g21 at 400 and one to g22; g21 answers
    # lower, g22 at 400: rows F, F, F, R over two edges
    b.add(1, (20, 2), 0, (21, 1), 400.0)
    b.add(1, (20, 1), 0, (22, 1), 400.0)
    b.add(1, (20, 1), 0, (21, 2), 400.0)
    b.add(0, (21, 1), 1, (20, 1), 390.0)
    b.add(0, (22, 1), 1, (20, 2), 400.0)
    # the tie made by one forward and one reverse row (needs top_matches >= 2)
    b.add(1, (30, 1), 0, (31, 1), 300.0)
    b.add(1, (30, 1), 0, (32, 1), 350.0)
    b.add(0, (31, 1), 1, (30, 1), 350.0)
    b.add(0, (32, 1), 1, (30, 1), 300.0)
    # the same in another pair, (S1, S2): three subject genes at the maximum
    for g in (41, 42, 43):
        b.add(2, (40, 1), 1, (g, 1), 250.5)
        b.add(1, (g, 1), 2, (40, 1), 250.5)
    b.add(2, (40, 1), 1, (44, 1), 100.0)
    b.add(1, (44, 1), 2, (40, 1), 100.0)
    return b.case()


def crafted_placing_keep_all():
    """keep_all=True on the placing path: every score of a search is distinct,
    so no item has more than 2 rows or more than 1 edge at any top_matches, and
    the pairs whose two directions score the same give items with one forward
    and one reverse row."""
    b = _Builder("placing-keep-all", 3, 102)
    tenths = itertools.count(2000, 7)   # distinct scores, in tenths of a bit

    def nxt(plus=0):
        return (next(tenths) + plus) / 10.0
    for g in range(1, 5):
        for a, c in itertools.combinations(range(3), 2):
            if g % 4 == 0:     # asymmetric: the forward row wins alone
                x = next(tenths)
                b.add(c, (g, 1), a, (g, 1), (x + 500) / 10.0)
                b.add(a, (g, 1), c, (g, 1), x / 10.0)
            else:              # one forward and one reverse row at the maximum
                b.both(a, (g, 1), c, (g, 1), nxt(600))
            # lower rows of other isoforms and a paralog, each score once
            b.add(c, (g, 2), a, (g, 1), nxt(-1000))
            b.add(a, (g, 2), c, (g, 2), nxt(-1000))
            b.add(c, (g, 1), a, (g % 4 + 1, 1), nxt(-1200))
            b.add(a, (g, 1), c, (g % 4 + 1, 2), nxt(-1200))
    return b.case()


# group score lists of crafted_threshold(): per top_n, n-th largest duplicated
# with cnt > top_n (both "more rows than n at the threshold" and "duplicates
# above it"), cnt == top_n and cnt == top_n + 1
THRESHOLD_GROUPS = {
    2: [[500.0, 400.0, 400.0, 300.0], [500.0, 500.0, 400.0, 400.0, 300.0], [400.0, 300.0], [400.0, 400.0, 300.0]],
    3: [[500.0, 450.0, 400.0, 400.0, 400.0, 300.0], [500.0, 500.0, 500.0, 400.0, 400.0, 300.0],
        [450.0, 400.0, 300.0], [450.0, 400.0, 400.0, 300.0]],
    5: [[500.0, 480.0, 460.0, 440.0, 400.0, 400.0, 400.0, 300.0],
        [500.0, 500.0, 500.0, 480.0, 480.0, 480.0, 400.0, 300.0],
        [500.0, 480.0, 460.0, 440.0, 400.0], [500.0, 480.0, 460.0, 400.0, 400.0, 400.0]],
}


def crafted_threshold():
    """Duplicates at the nlargest threshold. Each group (one query gene against
    one subject sample) has a given score list; every row hits a subject gene
    of its own, and every subject gene hits back with one row at 600.0, above
    every score of the group -- so exactly the gene pairs whose row passes the
    group's threshold reach the table (as one item with several edges, or as
    several items), and a threshold that counted or dropped duplicates
    differently changes it.
    The groups of each top_n go to the four searches between S0 and S1, S2."""
    b = _Builder("threshold-duplicates", 3, 103)
    b.orthologs([1, 2, 3], 300.0)
    gene = itertools.count(100)
    for top_n, groups in sorted(THRESHOLD_GROUPS.items()):
        for (qs, ss), scores in zip(((1, 0), (0, 1), (2, 0), (0, 2)), groups):
            q = next(gene)
            for k in (int(k) for k in b.rng.permutation(len(scores))):
                sg = next(gene)
                b.add(qs, (q, 1 + k % 2), ss, (sg, 1), scores[k])
                b.add(ss, (sg, 1), qs, (q, 1), 600.0)
    return b.case()


CRAFTED = {"tie-across-genes": crafted_tie_across_genes, "placing-keep-all": crafted_placing_keep_all,
           "threshold-duplicates": crafted_threshold}


# (top_matches, keep_all) settings and cases of tests/golden/post_alignment_ties.json
FIXTURE_SETTINGS = [(1, True), (3, True), (5, True), (3, False)]


def fixture_cases():
    """The cases whose reference output tests/golden/make_golden.py records:
    2, 3 and 4 samples at 400-480 HSPs (the last with groups of 16 HSPs), no
    empty searches (the reference fails on them), and the crafted cases."""
    return [family_case(1, 2, 120, 1, 3, p_empty=0.0), family_case(0, 3, 15, 2, 2, p_empty=0.0),
            family_case(2, 4, 4, 3, 2, p_empty=0.0)] + [f() for f in CRAFTED.values()]


# --- the compact form of tests/golden/post_alignment_ties.json -------------
# A table row of the reference is one input HSP with a label and a direction,
# so the file stores it as [label, reverse, index of the HSP in its search];
# transcripts are (gene, iso) pairs named by ID_FORMAT, samples are indices.
# make_golden.py checks at capture time that unpacking gives back exactly what
# the reference returned, every column of every row.

HSP_COLUMNS = ["qseqid", "sseqid", "pident", "length", "mismatch", "gapopen", "qstart", "qend", "sstart", "send",
               "evalue", "bitscore", "gaps", "nident", "sstrand"]
TABLE_COLUMNS = ["label", "pident", "length", "mismatch", "gapopen", "qstart", "qend", "sstart", "send", "evalue",
                 "bitscore", "gaps", "nident", "sstrand", "qgene", "qiso", "sgene", "siso", "reverse", "ssample",
                 "qsample"]


# a stored hit; the other HSP columns follow from these (an ungapped-coordinate
# HSP as _hsp() draws it): nident = length - gaps - mismatch, pident = 100 *
# nident / length to 3 places, qend = qstart + length - 1, the subject range
# [slow, slow + length - 1] read downwards on the minus strand, evalue 0
HIT_STORED = ["q_tx", "s_tx", "length", "mismatch", "gapopen", "qstart", "bitscore", "gaps", "slow", "minus"]


def _hit(qseqid, sseqid, r):
    nident, shigh = r["length"] - r["gaps"] - r["mismatch"], r["slow"] + r["length"] - 1
    return {"qseqid": qseqid, "sseqid": sseqid, "pident": round(100.0 * nident / r["length"], 3),
            "length": r["length"], "mismatch": r["mismatch"], "gapopen": r["gapopen"], "qstart": r["qstart"],
            "qend": r["qstart"] + r["length"] - 1, "sstart": shigh if r["minus"] else r["slow"],
            "send": r["slow"] if r["minus"] else shigh, "evalue": 0.0, "bitscore": r["bitscore"], "gaps": r["gaps"],
            "nident": nident, "sstrand": "minus" if r["minus"] else "plus"}


def _table_row(h, label, reverse, t1, t2):
    from oracle.post_oracle import default_parse_id
    q, s_ = default_parse_id(h["qseqid"])[1:], default_parse_id(h["sseqid"])[1:]
    if reverse:
        q, s_ = s_, q
    return [label] + [h[c] for c in HSP_COLUMNS[2:]] + [q[0], q[1], s_[0], s_[1], bool(reverse), t1, t2]


def pack_fixture(case, expected):
    """case + {setting: the reference's result} -> the stored form."""
    six = {s: i for i, s in enumerate(case.samples)}
    tix = {s: {t: k for k, t in enumerate(case.transcripts[s])} for s in case.samples}
    from oracle.post_oracle import default_parse_id

    def pair(key):
        a, b = key.split("|")
        return f"{six[a]}-{six[b]}"

    hits = {}
    for (q, s_), rows in case.hits.items():
        hits[f"{six[q]}-{six[s_]}"] = [
            [tix[q][tuple(default_parse_id(h["qseqid"])[1:])], tix[s_][tuple(default_parse_id(h["sseqid"])[1:])]] +
            [h[c] for c in HIT_STORED[2:-2]] + [min(h["sstart"], h["send"]), 1 if h["sstrand"] == "minus" else 0]
            for h in rows]
    packed = {}
    for setting, res in expected.items():
        tables = {}
        for key, rows in res["tables"].items():
            t1, t2 = key.split("|")
            out = []
            for r in rows:
                label, reverse = r[0], r[TABLE_COLUMNS.index("reverse")]
                src = case.hits[(t1, t2) if reverse else (t2, t1)]
                out.append([label, int(reverse), next(i for i, h in enumerate(src)
                                                      if _table_row(h, label, reverse, t1, t2) == r)])
            tables[pair(key)] = out
        packed[setting] = {
            "tables": tables,
            "edges": [[six[u[0]], u[1], six[v[0]], v[1]] for u, v in res["edges"]],
            "nodes": [[six[s_], g] for s_, g in res["nodes"]],
            "valid": [[six[s_], g] for s_, g in res["valid"]],
            "sums": {pair(k): v for k, v in res["sums"].items()},
            "matrix": res["matrix"], "errors": res["errors"], "sample_count": res["sample_count"],
            "mapping_from_dfs_ok": res["mapping_from_dfs_ok"]}
    return {"name": case.name, "samples": case.samples,
            "transcripts": [[list(t) for t in case.transcripts[s]] for s in case.samples],
            "hits": hits, "expected": packed}


def unpack_fixture(fx):
    """The stored form -> {"name", "samples", "transcripts" {label: [(gene,
    iso)]}, "hits" {(q label, s label): HSP dicts}, "expected" {setting: the
    reference's result as make_golden.run_reference returned it}}."""
    samples = fx["samples"]
    tx = {s: [tuple(t) for t in fx["transcripts"][i]] for i, s in enumerate(samples)}
    hits = {}
    for key, rows in fx["hits"].items():
        q, s_ = (samples[int(x)] for x in key.split("-"))
        hits[(q, s_)] = [_hit(tx_id(*tx[q][r[0]]), tx_id(*tx[s_][r[1]]), dict(zip(HIT_STORED, r))) for r in rows]

    def pair(key):
        a, b = key.split("-")
        return samples[int(a)], samples[int(b)]

    expected = {}
    for setting, e in fx["expected"].items():
        tables = {}
        for key, rows in e["tables"].items():
            t1, t2 = pair(key)
            tables[f"{t1}|{t2}"] = [_table_row(hits[(t1, t2) if rev else (t2, t1)][i], label, rev, t1, t2)
                                    for label, rev, i in rows]
        expected[setting] = {
            "tables": tables, "errors": e["errors"], "mapping_from_dfs_ok": e["mapping_from_dfs_ok"],
            "edges": [[[samples[a], ga], [samples[b], gb]] for a, ga, b, gb in e["edges"]],
            "nodes": [[samples[s_], g] for s_, g in e["nodes"]], "sample_count": e["sample_count"],
            "valid": [[samples[s_], g] for s_, g in e["valid"]],
            "sums": {"|".join(pair(k)): v for k, v in e["sums"].items()}, "matrix": e["matrix"]}
    return {"name": fx["name"], "samples": samples, "transcripts": tx, "hits": hits, "expected": expected}


def item_profile(tables):
    """Per item -- (table, query gene): one thread of the RBH kernels -- the
    rows, edges (distinct subject genes) and whether it has both a forward
    and a reverse row, from the oracle's tables. Returns {"max_rows",
    "max_edges", "over_rows" (items with > 2 rows), "over_edges" (items with
    > 1 edge), "both" (items with a forward and a reverse row)}."""
    items = {}
    for key, rows in tables.items():
        for r in rows:
            it = items.setdefault((key, r["qgene"]), {"rows": 0, "genes": set(), "rev": set()})
            it["rows"] += 1
            it["genes"].add(r["sgene"])
            it["rev"].add(bool(r["reverse"]))
    return {"max_rows": max((i["rows"] for i in items.values()), default=0),
            "max_edges": max((len(i["genes"]) for i in items.values()), default=0),
            "over_rows": sum(i["rows"] > 2 for i in items.values()),
            "over_edges": sum(len(i["genes"]) > 1 for i in items.values()),
            "both": sum(len(i["rev"]) == 2 for i in items.values())}


def threshold_groups(case, top_n):
    """Groups (search, query gene) of more than top_n HSPs whose top_n-th
    largest bit score occurs more than once."""
    from oracle.post_oracle import default_parse_id
    n = 0
    for key, rows in case.hits.items():
        groups = {}
        for h in rows:
            groups.setdefault(default_parse_id(h["qseqid"])[1], []).append(h["bitscore"])
        for g in groups.values():
            if len(g) > top_n and g.count(sorted(g, reverse=True)[top_n - 1]) > 1:
                n += 1
    return n


def largest_group(case):
    from oracle.post_oracle import default_parse_id
    m = 0
    for rows in case.hits.values():
        groups = {}
        for h in rows:
            g = default_parse_id(h["qseqid"])[1]
            groups[g] = groups.get(g, 0) + 1
        m = max(m, max(groups.values(), default=0))
    return m


# ---------------------------------------------------------------------------
# graph record cases
# ---------------------------------------------------------------------------

EDGE, SUM_ONLY, NODE_ONLY = 0, 1, 2


def pair_index(a, b):
    """A single shard's pair numbering (subject-major): (0,1), (0,2), (1,2),
    (0,3), ... The GPU test checks it against Engine.pair_order()."""
    a, b = min(a, b), max(a, b)
    return b * (b - 1) // 2 + a


class GraphCase:
    """genes[s]: number of genes of sample s (gene ids 1..genes[s]; the
    engine numbers nodes sample-major in ascending gene id). recs: (kind,
    (sample, gene), (sample, gene), nident, den) in record order.
    sample_count: the value for set_sample_count, or None."""

    def __init__(self, name, genes, recs, sample_count=None):
        self.name, self.genes, self.recs, self.sample_count = name, list(genes), list(recs), sample_count

    def with_order(self, tag, order):
        return GraphCase(f"{self.name}-{tag}", self.genes, [self.recs[i] for i in order], self.sample_count)

    def pair_major(self):
        key = [pair_index(u[0], v[0]) if k != NODE_ONLY else -1 for k, u, v, _, _ in self.recs]
        return self.with_order("pair-major", sorted(range(len(self.recs)), key=lambda i: key[i]))

    def permuted(self, seed):
        return self.with_order("permuted", np.random.default_rng(seed).permutation(len(self.recs)))

    def prefix(self, n):
        return GraphCase(f"{self.name}-first{n}", self.genes, self.recs[:n], self.sample_count)

    def records(self):
        """The EDGE_RECORD_DTYPE array: a < b for edges and sums-only records,
        a == b for node records."""
        from rna_clique_amd import _native as nat
        base = np.concatenate([[0], np.cumsum(self.genes)])
        arr = np.zeros(len(self.recs), dtype=nat.EDGE_RECORD_DTYPE)
        seen = set()
        for i, (kind, u, v, num, den) in enumerate(self.recs):
            assert 1 <= u[1] <= self.genes[u[0]] and 1 <= v[1] <= self.genes[v[0]]
            a, b = int(base[u[0]]) + u[1] - 1, int(base[v[0]]) + v[1] - 1
            if kind == NODE_ONLY:
                assert a == b
                arr[i] = (a, a, nat.RC_NODE_ONLY, 0, 0)
                continue
            assert u[0] != v[0] and 0 <= num < 2 ** 31 and 0 <= den < 2 ** 31
            p = pair_index(u[0], v[0])
            if kind == EDGE:
                assert (min(a, b), max(a, b)) not in seen, "one graph record per undirected edge"
                seen.add((min(a, b), max(a, b)))
            arr[i] = (min(a, b), max(a, b), p | (nat.RC_EDGE_SUM_ONLY if kind == SUM_ONLY else 0), num, den)
        return arr

    def graph(self):
        """(nodes, edges) as post_oracle takes them: nodes of edge and node
        records; sums-only records join nothing."""
        nodes, edges = set(), set()
        for kind, u, v, _, _ in self.recs:
            if kind == SUM_ONLY:
                continue
            nodes.add(u)
            nodes.add(v)
            if kind == EDGE:
                edges.add(tuple(sorted((u, v))))
        return nodes, edges

    def expected(self):
        """The reference's answer from post_oracle: components, ideal nodes,
        sample count, and both sums per sample pair in Python integers
        (filtered: both endpoints in ideal components, post_oracle.pair_sums)."""
        from oracle import post_oracle as po
        nodes, edges = self.graph()
        sc = self.sample_count if self.sample_count else po.sample_count(nodes)
        valid = po.ideal_nodes(nodes, edges, sc)
        comps, _ = po.components(nodes, edges)
        n = len(self.genes)
        fsum = {p: [0, 0] for p in itertools.combinations(range(n), 2)}
        usum = {p: [0, 0] for p in itertools.combinations(range(n), 2)}
        for kind, u, v, num, den in self.recs:
            if kind == NODE_ONLY:
                continue
            p = (min(u[0], v[0]), max(u[0], v[0]))
            usum[p][0] += num
            usum[p][1] += den
            if u in valid and v in valid:
                fsum[p][0] += num
                fsum[p][1] += den
        return {"nodes": len(nodes), "records": len(self.recs), "components": len(comps),
                "ideal_components": len(valid) // sc if sc else 0, "ideal_nodes": sorted(valid),
                "sample_count": sc, "sums": fsum, "usums": usum}


def _w(rng):
    num = int(rng.integers(20, 800))
    return num, num + int(rng.integers(0, 50))


def chain_case(n=20000, seed=7):
    """a1-b1-a2-b2-...-an-bn alternating samples 0 and 1: one component of 2n
    nodes, no ideal one. Records in ascending order."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(1, n + 1):
        recs.append((EDGE, (0, i), (1, i), *_w(rng)))
        if i < n:
            recs.append((EDGE, (1, i), (0, i + 1), *_w(rng)))
    return GraphCase("chain", [n, n], recs)


def star_case(n=20000, n_pairs=50, seed=8):
    """Gene 1 of sample 0 joined to genes 1..n of sample 1, plus n_pairs
    separate two-node components (the ideal ones of a two-sample graph)."""
    rng = np.random.default_rng(seed)
    recs = [(EDGE, (0, 1), (1, j), *_w(rng)) for j in range(1, n + 1)]
    recs += [(EDGE, (0, 1 + k), (1, n + k), *_w(rng)) for k in range(1, n_pairs + 1)]
    return GraphCase("star", [1 + n_pairs, n + n_pairs], recs)


def cliques_case(S, n_each=25, seed=9, extras=True):
    """n_each of: complete S-cliques (ideal), S-cliques missing one edge, two
    S-cliques joined by one extra edge (one component of 2S nodes), complete
    cliques over S - 1 samples. One gene per sample and clique. With `extras`,
    sums-only records between two different ideal cliques (both endpoints
    valid: they count in the filtered sums) and with one endpoint outside the
    ideal cliques (unfiltered sums only)."""
    rng = np.random.default_rng(seed + S)
    nxt = [0] * S
    recs, ideal, other = [], [], []

    def clique(samples, drop=None):
        genes = {}
        for s in samples:
            nxt[s] += 1
            genes[s] = nxt[s]
        for a, b in itertools.combinations(samples, 2):
            if (a, b) != drop:
                recs.append((EDGE, (a, genes[a]), (b, genes[b]), *_w(rng)))
        return genes

    for k in range(n_each):
        ideal.append(clique(range(S)))
        pairs = list(itertools.combinations(range(S), 2))
        other.append(clique(range(S), drop=pairs[int(rng.integers(len(pairs)))]))
        g1, g2 = clique(range(S)), clique(range(S))
        a, b = (int(x) for x in rng.choice(S, 2, replace=False))
        recs.append((EDGE, (a, g1[a]), (b, g2[b]), *_w(rng)))
        other += [g1, g2]
        skip = int(rng.integers(S))
        other.append(clique([s for s in range(S) if s != skip]))
    if extras:
        for k in range(n_each):
            c1, c2 = ideal[k], ideal[(k + 1) % n_each]
            a, b = (int(x) for x in rng.choice(S, 2, replace=False))
            recs.append((SUM_ONLY, (a, c1[a]), (b, c2[b]), *_w(rng)))
            c3 = other[int(rng.integers(len(other)))]
            b = [s for s in c3 if s != a][0]
            recs.append((SUM_ONLY, (a, c1[a]), (b, c3[b]), *_w(rng)))
    return GraphCase(f"cliques{S}", nxt, recs)


def node_only_case(extra_sample=False, sample_count=None):
    """Pair-major 3-cliques with node-only records at positions 0 and 64, in
    the middle of a pair's run and at the end. extra_sample: one more node
    record of a fourth sample that has no other node -- it raises the sample
    count to 4 and empties the ideal set unless set_sample_count(3) is given."""
    base = cliques_case(3, n_each=30, seed=21, extras=False).pair_major()
    recs, genes = list(base.recs), list(base.genes)
    if extra_sample:
        genes.append(2)

    def fresh(s):
        genes[s] += 1
        return (NODE_ONLY, (s, genes[s]), (s, genes[s]), 0, 0)
    run1 = [i for i, r in enumerate(recs) if pair_index(r[1][0], r[2][0]) == 1]
    mid = run1[len(run1) // 2]
    assert mid > 66
    recs.insert(0, fresh(0))
    recs.insert(64, fresh(2))
    recs.insert(mid + 2, fresh(1))
    if extra_sample:
        recs.insert(130, (NODE_ONLY, (3, 2), (3, 2), 0, 0))
    recs.append(fresh(0))
    assert recs[0][0] == NODE_ONLY and recs[64][0] == NODE_ONLY and recs[-1][0] == NODE_ONLY
    name = "node-only" + ("-extra-sample" if extra_sample else "") + (f"-count{sample_count}" if sample_count else "")
    return GraphCase(name, genes, recs, sample_count)


def large_sums_case(n=3000, seed=5):
    """One pair, n two-node ideal components whose nident and den are near
    2^31 - 1: the sums pass 2^32 (about 6.4e12). The distance must be
    float(1 - Fraction(num, den)) = correctly rounded (den - num) / den; the
    values are chosen so that 1.0 - num / den differs from it."""
    rng = np.random.default_rng(seed)
    top = 2 ** 31 - 1
    recs = []
    for i in range(1, n + 1):
        den = top - int(rng.integers(0, 1000))
        recs.append((EDGE, (0, i), (1, i), den - int(rng.integers(1, 10 ** 6)), den))
    num, den = sum(r[3] for r in recs), sum(r[4] for r in recs)
    assert num > 2 ** 32 and den > 2 ** 32
    exact = float(1 - Fraction(num, den))
    assert (den - num) / den == exact and 1.0 - num / den != exact
    return GraphCase("large-sums", [n, n], recs)


def graph_cases():
    """Every graph record case, by name."""
    out = []
    ch = chain_case()
    out += [ch.with_order("ascending", range(len(ch.recs))), ch.with_order("descending", range(len(ch.recs) - 1, -1, -1)),
            ch.permuted(31)]
    st = star_case()
    out += [st.with_order("ascending", range(len(st.recs))), st.permuted(32)]
    for S in (3, 4, 6):
        c = cliques_case(S)
        out += [c.pair_major(), c.permuted(33 + S)]
    out += [node_only_case(), node_only_case(extra_sample=True), node_only_case(extra_sample=True, sample_count=3)]
    small = cliques_case(3, n_each=30, seed=22).permuted(34)
    out += [small.prefix(n) for n in (0, 1, 63, 64, 65, 257)]
    out.append(large_sums_case())
    return {c.name: c for c in out}
