"""The post-alignment GPU stage (rbh_kernel / rbh_place_kernel, the union-find
graph kernels, pair_sums_kernel, distance_kernel) on tie-heavy and
adversarial inputs, integer- and bit-exact, no tolerances.

RBH stage: external-alignment engines fed with the cases of tests/post_cases.py
(every sample with its explicit transcript list), compared with
oracle/post_oracle.py and with the reference's own recorded output
(tests/golden/post_alignment_ties.json). Each test asserts, from the expected
tables and not from the engine, which way out of the RBH step its input
forces: an item with more than RBH_RMAX = 2 rows or RBH_EMAX = 1 edge sends
the engine through the full second pass, none sends it through
rbh_place_kernel.

Graph phase: graph-only engines given edge records (import_edges): chains and
stars for the lock-free union-find, pair-major and permuted cliques for the
wave-uniform and the per-lane path of pair_sums_kernel, sums-only and
node-only records, record counts around the wave size, sums above 2^32.
"""
import functools
import itertools

import numpy as np
import pytest

import post_cases as pc
from oracle import post_oracle as po
from oracle.parity import ROW_COMPARE, engine_rows_as_dicts

pytestmark = pytest.mark.gpu

TOPS = (1, 2, 3, 5)
STAT_KEYS = ("nodes", "edges", "components", "ideal_components", "ideal_nodes", "sample_count")


# ---------------------------------------------------------------------------
# expected results, in one form whatever their source
# ---------------------------------------------------------------------------

def _graph_expectation(samples, tables, nodes, edges, sample_count, valid, sums, matrix):
    comps, _ = po.components(set(nodes), set(edges))
    usums = {k: (sum(r["nident"] for r in rows), sum(r["length"] - r["gaps"] for r in rows))
             for k, rows in tables.items()}
    return {"tables": tables, "edges": sorted(edges), "valid": sorted(valid), "sums": sums, "usums": usums,
            "matrix": matrix,
            "stats": {"nodes": len(nodes), "edges": len(edges), "components": len(comps),
                      "ideal_components": len(valid) // sample_count if sample_count else 0,
                      "ideal_nodes": len(valid), "sample_count": sample_count}}


@functools.lru_cache(maxsize=None)
def _case(kind, name):
    if kind == "family":
        return pc.family_shape_case(name)
    if kind == "crafted":
        return pc.CRAFTED[name]()
    if kind == "empty-search":
        case = pc.family_case(0, 3, 40, 2, 2)   # seed 0: the search T1 -> T0 comes out empty
        assert sorted(len(v) == 0 for v in case.hits.values()) == [False] * 5 + [True]
        return case
    return pc.family_case(3, 3, 12, 2, 2, p_empty=0.0, unhit_sample=True)


@functools.lru_cache(maxsize=None)
def _oracle_expected(kind, name, top, keep):
    """post_oracle.run_pipeline on a generator case (computed once per
    setting, shared, never modified)."""
    case = _case(kind, name)
    res = po.run_pipeline(case.samples, case.hits, po.default_parse_id, top, keep)
    try:
        matrix = po.distance_matrix(case.samples, res["sums"])
    except po.NoIdealComponentsError:
        matrix = None
    return _graph_expectation(case.samples, res["tables"], res["nodes"], res["edges"], res["sample_count"],
                              res["valid"], res["sums"], matrix)


def _recorded_expected(fx, cols, key):
    """The reference's recorded output of one fixture setting."""
    exp = fx["expected"][key]
    tables = {tuple(k.split("|")): [dict(zip(cols, r)) for r in rows] for k, rows in exp["tables"].items()}
    nodes = {(s, g) for s, g in exp["nodes"]}
    edges = {tuple(sorted(((u[0], u[1]), (v[0], v[1])))) for u, v in exp["edges"]}
    sums = {tuple(k.split("|")): tuple(v) for k, v in exp["sums"].items()}
    matrix = None if exp["matrix"] is None else (exp["matrix"]["labels"], exp["matrix"]["values"])
    return _graph_expectation(fx["samples"], tables, nodes, edges, exp["sample_count"],
                              {(s, g) for s, g in exp["valid"]}, sums, matrix)


# ---------------------------------------------------------------------------
# the engine's side
# ---------------------------------------------------------------------------

def _run_case(case, top, keep):
    """An external-alignment engine over the case: every sample with its own
    transcript list (silent genes and unhit samples included), every directed
    search's HSPs (empty searches too), then run()."""
    from rna_clique_amd.engine import Engine
    eng = Engine(device=0, top_matches=top, keep_all=keep)
    for s in case.samples:
        tx = case.transcripts[s]
        seq = np.frombuffer(b"ACGT" * 50 * len(tx), dtype=np.uint8)
        eng.add_sample(s, seq, np.arange(len(tx) + 1, dtype=np.uint64) * 200, [g for g, _ in tx], [i for _, i in tx])
    for (q, s), arr in sorted(case.hsp_arrays().items()):
        eng.add_hsps(q, s, arr)
    eng.run()
    return eng


def _check_distance(eng, matrix):
    from rna_clique_amd._native import NativeError, RC_E_NO_IDEAL
    if matrix is None:
        with pytest.raises(NativeError) as ei:
            eng.distance()
        assert ei.value.code == RC_E_NO_IDEAL
    else:
        labels, mat = eng.distance()
        assert labels == matrix[0]
        assert np.array_equal(mat, np.array(matrix[1]))


def _compare(eng, samples, exp):
    for a, b in itertools.combinations(range(len(samples)), 2):
        got = [[r[k] for k in ROW_COMPARE] for r in engine_rows_as_dicts(eng.pair_rows(a, b))]
        want = [[r[k] for k in ROW_COMPARE] for r in exp["tables"][(samples[a], samples[b])]]
        assert got == want, f"table {a},{b}: first difference " \
            f"{next(((x, y) for x, y in zip(got, want) if x != y), (len(got), len(want)))}"
    edges = sorted(tuple(sorted(((samples[e["sample_a"]], int(e["gene_a"])), (samples[e["sample_b"]], int(e["gene_b"])))))
                   for e in eng.edges())
    assert edges == exp["edges"]
    st = eng.stats()
    assert {k: st[k] for k in STAT_KEYS} == exp["stats"]
    s_, g_ = eng.ideal_nodes()
    assert sorted((samples[a], int(b)) for a, b in zip(s_, g_)) == exp["valid"]
    for unfiltered, want in ((False, exp["sums"]), (True, exp["usums"])):
        num, den = eng.pair_sums(unfiltered=unfiltered)
        for (t1, t2), (n_, d_) in want.items():
            a, b = samples.index(t1), samples.index(t2)
            assert (int(num[a, b]), int(den[a, b])) == (n_, d_) == (int(num[b, a]), int(den[b, a])), (unfiltered, t1, t2)
    _check_distance(eng, exp["matrix"])


def _check(kind, name, top, keep):
    case, exp = _case(kind, name), _oracle_expected(kind, name, top, keep)
    eng = _run_case(case, top, keep)
    try:
        _compare(eng, case.samples, exp)
    finally:
        eng.close()
    return pc.item_profile(exp["tables"]), exp


# ---------------------------------------------------------------------------
# RBH stage against the oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("shape", list(pc.FAMILY_SHAPES))
def test_family_cases(native, shape, top, keep):
    """Tie-heavy family tables. keep_all=True: some item has more than 2 rows
    (full second pass); keep_all=False: no item has more than 2 rows or more
    than 1 edge (placing kernel). Every setting has an ideal component."""
    prof, exp = _check("family", shape, top, keep)
    assert exp["stats"]["ideal_components"] > 0 and exp["matrix"] is not None
    if keep:
        assert prof["over_rows"] > 0
    else:
        assert prof["over_rows"] == 0 and prof["over_edges"] == 0


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("top", TOPS)
def test_unhit_sample(native, top, keep):
    """A fourth sample that no search touches (all six searches with it are
    empty): it does not count toward sample_count, the other three keep their
    ideal components, its pairs have empty tables and the matrix is refused
    as the reference refuses it."""
    prof, exp = _check("unhit", "", top, keep)
    assert exp["stats"]["sample_count"] == 3 and exp["stats"]["ideal_components"] > 0
    assert exp["matrix"] is None
    assert prof["over_rows"] > 0 if keep else prof["over_rows"] == 0 and prof["over_edges"] == 0


@pytest.mark.parametrize("top,keep", [(1, True), (3, True), (3, False)])
def test_empty_directed_search(native, top, keep):
    """One of the six directed searches is empty (the reference itself fails
    there; the oracle gives that pair an empty table): the pair has no rows
    and no edges, so no component is ideal and the matrix is refused, while
    the other two tables equal the oracle's."""
    prof, exp = _check("empty-search", "", top, keep)
    assert sorted(len(t) == 0 for t in exp["tables"].values()) == [False, False, True]
    assert exp["stats"]["ideal_components"] == 0 and exp["matrix"] is None
    assert prof["over_rows"] > 0 if keep else prof["over_rows"] == 0


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("top", TOPS)
def test_tie_across_two_subject_genes(native, top, keep):
    """An item whose maximum ties across subject genes: 2 or 3 edges with
    keep_all (second pass); exactly one row per item -- the reference's
    first -- without it (placing kernel)."""
    prof, _ = _check("crafted", "tie-across-genes", top, keep)
    if keep:
        assert prof["max_edges"] >= 2 and prof["over_edges"] >= 3
    else:
        assert prof["max_rows"] == 1


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("top", TOPS)
def test_keep_all_on_the_placing_path(native, top, keep):
    """Distinct scores: no item exceeds the slots at any setting, so
    keep_all=True goes through rbh_place_kernel, with items that have one
    forward and one reverse row."""
    prof, _ = _check("crafted", "placing-keep-all", top, keep)
    assert prof["over_rows"] == 0 and prof["over_edges"] == 0
    if keep:
        assert prof["both"] >= 3


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("top", TOPS)
def test_duplicates_at_the_threshold(native, top, keep):
    """Groups with cnt > top_n whose n-th largest value is duplicated (for
    top_n 2, 3 and 5), with cnt == top_n and cnt == top_n + 1. With keep_all
    and top_matches >= 2 the rows at the threshold give items with several
    edges (second pass); otherwise no item exceeds its slots (placing)."""
    case = _case("crafted", "threshold-duplicates")
    for top_n in (2, 3, 5):
        assert pc.threshold_groups(case, top_n) >= 1
    prof, _ = _check("crafted", "threshold-duplicates", top, keep)
    if keep and top >= 2:
        assert prof["over_edges"] > 0 and prof["max_edges"] >= 3
    else:
        assert prof["over_rows"] == 0 and prof["over_edges"] == 0


# ---------------------------------------------------------------------------
# RBH stage against the reference's recorded output
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ties():
    from test_oracle_golden_ties import load_ties
    return load_ties()


def _tie_params():
    cols, hc, settings, fixtures = _ties()
    return [(i, f"{top}-{keep}") for i in range(len(fixtures)) for top, keep in settings]


@pytest.mark.parametrize("index,key", _tie_params(),
                         ids=[f"{_ties()[3][i]['name']}-n{k}" for i, k in _tie_params()])
def test_recorded_reference_ties(native, index, key):
    """Every fixture of post_alignment_ties.json at every recorded setting:
    the engine gives the reference's own tables, graph, ideal nodes, sums and
    matrix. keep_all family fixtures force the second pass."""
    cols, hc, settings, fixtures = _ties()
    fx = fixtures[index]
    top, keep = int(key.split("-")[0]), key.endswith("True")
    case = pc.Case(fx["name"], fx["samples"], fx["transcripts"], fx["hits"])
    exp = _recorded_expected(fx, cols, key)
    eng = _run_case(case, top, keep)
    try:
        _compare(eng, case.samples, exp)
    finally:
        eng.close()
    prof = pc.item_profile(exp["tables"])
    if fx["name"].startswith("family") and keep:
        assert prof["over_rows"] > 0
    if not keep or fx["name"] == "placing-keep-all":
        assert prof["over_rows"] == 0 and prof["over_edges"] == 0


# ---------------------------------------------------------------------------
# placing kernel against the full second pass
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name,top,keep", [("family", "large-groups", 3, False),
                                                 ("crafted", "placing-keep-all", 5, True)])
def test_placing_equals_second_pass(native, monkeypatch, kind, name, top, keep):
    """An input without slot overflow, run through rbh_place_kernel (default)
    and through the full second pass (RC_RBH_TWO_PASS=1): the same rows,
    labels and edges, byte for byte -- and both equal the oracle's."""
    case, exp = _case(kind, name), _oracle_expected(kind, name, top, keep)
    prof = pc.item_profile(exp["tables"])
    assert prof["over_rows"] == 0 and prof["over_edges"] == 0 and prof["max_rows"] >= 1
    out = []
    for two_pass in (False, True):
        if two_pass:
            monkeypatch.setenv("RC_RBH_TWO_PASS", "1")
        else:
            monkeypatch.delenv("RC_RBH_TWO_PASS", raising=False)
        eng = _run_case(case, top, keep)
        try:
            _compare(eng, case.samples, exp)
            n = len(case.samples)
            out.append(([eng.pair_rows(a, b).tobytes() for a, b in itertools.combinations(range(n), 2)],
                        eng.edges().tobytes()))
        finally:
            eng.close()
    assert out[0] == out[1]


# ---------------------------------------------------------------------------
# graph phase through import_edges
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _graph_cases():
    return pc.graph_cases()


@functools.lru_cache(maxsize=None)
def _graph_expected(name):
    return _graph_cases()[name].expected()


def _graph_engine(case):
    """A graph-only engine: one zero-length transcript per gene (as
    similarity._graph_engine builds it), then import_edges of the host
    records."""
    from rna_clique_amd.engine import Engine
    eng = Engine(device=0)
    for s, n in enumerate(case.genes):
        eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                       np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
    n = len(case.genes)
    assert eng.pair_order() == sorted(itertools.combinations(range(n), 2), key=lambda p: pc.pair_index(*p))
    if case.sample_count:
        eng.set_sample_count(case.sample_count)
    eng.import_edges(case.records().view(np.uint8))
    return eng


def _check_graph(name):
    case, exp = _graph_cases()[name], _graph_expected(name)
    eng = _graph_engine(case)
    try:
        st = eng.stats()
        # (in graph-only mode stats()["edges"] counts the imported records)
        assert {k: st[k] for k in STAT_KEYS} == {
            "nodes": exp["nodes"], "edges": exp["records"], "components": exp["components"],
            "ideal_components": exp["ideal_components"], "ideal_nodes": len(exp["ideal_nodes"]),
            "sample_count": exp["sample_count"]}
        s_, g_ = eng.ideal_nodes()
        assert sorted((int(a), int(b)) for a, b in zip(s_, g_)) == exp["ideal_nodes"]
        for unfiltered, want in ((False, exp["sums"]), (True, exp["usums"])):
            num, den = eng.pair_sums(unfiltered=unfiltered)
            for (a, b), (n_, d_) in want.items():
                assert (int(num[a, b]), int(den[a, b])) == (n_, d_) == (int(num[b, a]), int(den[b, a])), (unfiltered, a, b)
        labels = [f"S{s}" for s in range(len(case.genes))]
        try:
            matrix = po.distance_matrix(labels, {(labels[a], labels[b]): v for (a, b), v in exp["sums"].items()})
        except po.NoIdealComponentsError:
            matrix = None
        _check_distance(eng, matrix)
    finally:
        eng.close()
    return exp


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_union_find_chain(native, order):
    """A 40 000-node chain alternating two samples, 157 blocks hooking at
    once: one component, no ideal one, no filtered sums (RC_E_NO_IDEAL)."""
    exp = _check_graph(f"chain-{order}")
    assert (exp["components"], exp["ideal_components"], exp["nodes"]) == (1, 0, 40000)


@pytest.mark.parametrize("order", ["ascending", "permuted"])
def test_union_find_star(native, order):
    """One gene joined to 20 000 genes of the other sample (every hook
    contends for one root), beside 50 two-node ideal components."""
    exp = _check_graph(f"star-{order}")
    assert (exp["components"], exp["ideal_components"]) == (51, 50)


@pytest.mark.parametrize("S", [3, 4, 6])
def test_cliques_pair_major_and_permuted(native, S):
    """Complete S-cliques, cliques missing an edge, joined pairs of cliques
    and (S-1)-cliques, with sums-only records between ideal cliques (filtered
    and unfiltered sums) and into non-ideal ones (unfiltered only). Pair-major
    records take pair_sums_kernel's wave-uniform path, permuted ones its
    per-lane path (almost every wave mixes pairs); both give the oracle's
    result, hence the same one."""
    a = _check_graph(f"cliques{S}-pair-major")
    b = _check_graph(f"cliques{S}-permuted")
    assert a == b and a["ideal_components"] == 25 and a["components"] == 100
    arr = _graph_cases()[f"cliques{S}-permuted"].records()
    pairs = (arr["pair"] & 0x7FFFFFFF)[:len(arr) // 64 * 64].reshape(-1, 64)
    assert (pairs != pairs[:, :1]).any(1).mean() > 0.9
    arr = _graph_cases()[f"cliques{S}-pair-major"].records()
    assert (np.diff((arr["pair"] & 0x7FFFFFFF).astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("name,ideal,count", [("node-only", 30, 3), ("node-only-extra-sample", 0, 4),
                                              ("node-only-extra-sample-count3", 30, 3)])
def test_node_only_records(native, name, ideal, count):
    """Node-only records at positions 0 and 64, inside a pair's run and at the
    end: they add isolated nodes and no sums. One for a sample with no other
    node raises sample_count to 4 and empties the ideal set; set_sample_count(3)
    restores it."""
    exp = _check_graph(name)
    assert (exp["ideal_components"], exp["sample_count"]) == (ideal, count)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_record_counts(native, n):
    """Record counts around the wave (64) and block (256) sizes, mixed pairs."""
    exp = _check_graph(f"cliques3-permuted-first{n}")
    assert exp["records"] == n


def test_sums_above_2_to_32(native):
    """3000 records of nident and den near 2^31 - 1 in one pair: sums of about
    6.4e12, and a distance that must be the correctly rounded (den - num) / den
    = float(1 - Fraction(num, den)), which differs from 1.0 - num / den."""
    exp = _check_graph("large-sums")
    num, den = exp["sums"][(0, 1)]
    assert num > 2 ** 32 and den > 2 ** 32 and 1.0 - num / den != (den - num) / den
