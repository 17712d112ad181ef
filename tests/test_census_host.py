"""The component census on the host: the restatement of tests/census_oracle.py
against the reference's recorded components (tests/golden/component_stats.json)
and against networkx, census.ComponentTable on a hand-written graph whose every
derived column is written out, and the command's two output formats. No GPU.
Every comparison is exact."""
import functools
import json
import os

import numpy as np
import pytest

import census_cases as cc
import census_oracle as zo
import component_oracle as co
import post_cases as pc
from oracle import post_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "component_stats.json")
SETTINGS = [(1, True), (3, True), (3, False)]


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


def fixture_multiset(exp):
    """A recorded setting's components as census_oracle.Census.multiset()."""
    return sorted((tuple(tuple(m) for m in c["members"]), c["edges"]) for c in exp["components"])


def case_census(case, top, keep):
    """The oracle's census of an HSP case: post_oracle's own tables and graph,
    samples as indices in input order."""
    res = po.run_pipeline(case.samples, case.hits, po.default_parse_id, top, keep)
    nodes, edges = co.index_nodes(case.samples, res["nodes"], res["edges"])
    return zo.Census(nodes, edges, res["sample_count"])


FIXTURE_PARAMS = [(c, top, keep) for c in pc.fixture_cases() for top, keep in SETTINGS]


@pytest.mark.parametrize("case,top,keep", FIXTURE_PARAMS, ids=[f"{c.name}-n{t}-{k}" for c, t, k in FIXTURE_PARAMS])
def test_oracle_equals_recorded_reference(case, top, keep):
    """Members and edge count of every component as the reference's
    component_subgraphs gave them (as multisets: its order is networkx's), the
    sample count, and the reference's number of ideal components."""
    fx = golden()["cases"][case.name]
    assert fx["samples"] == case.samples
    exp = fx["expected"][f"{top}-{keep}"]
    z = case_census(case, top, keep)
    assert z.multiset() == fixture_multiset(exp)
    assert z.sample_count == exp["sample_count"]
    assert len(z.ideal_ids()) == exp["ideal_components"]
    assert z.statistics()[1] == len(exp["components"])


def test_recorded_summaries():
    """The totals the fixture was captured with."""
    c = golden()["cases"]
    e = c["threshold-duplicates"]["expected"]["3-True"]
    sizes = [len(x["members"]) for x in e["components"]]
    assert (len(sizes), e["ideal_components"], min(sizes), max(sizes)) == (15, 3, 3, 6)
    assert {len({s for s, _ in x["members"]}) for x in e["components"]} == {2, 3}
    e = c["tie-across-genes"]["expected"]["1-True"]
    assert (len(e["components"]), e["ideal_components"]) == (8, 4)
    t = case_census(next(k for k in pc.fixture_cases() if k.name == "tie-across-genes"), 1, True).table("ABC")
    assert int(t.one_short.sum()) == 1 and t.nodes[t.one_short].tolist() == [2]
    e = c["family-s2-4x4x3x2"]["expected"]["1-True"]
    big = [x for x in e["components"] if len(x["members"]) == 8]
    assert len(big) == 1 and len({s for s, _ in big[0]["members"]}) == 4


def _graph_cases():
    out = dict(pc.graph_cases())
    out.update(cc.new_cases())
    return out


@pytest.mark.parametrize("name", sorted(_graph_cases()))
def test_oracle_equals_networkx(name):
    """An independent statement with networkx: connected_components and each
    subgraph's number_of_edges, ordered by lowest node."""
    import networkx as nx
    case = _graph_cases()[name]
    nodes, edges = case.graph()
    g = nx.Graph()
    g.add_nodes_from(nodes)
    g.add_edges_from(edges)
    comps = sorted((sorted(c) for c in nx.connected_components(g)), key=lambda c: c[0])
    z = zo.from_case(case)
    assert z.members == comps
    assert z.edges == [g.subgraph(c).number_of_edges() for c in comps]
    a = z.arrays()
    assert a["samples"].tolist() == [len({s for s, _ in c}) for c in comps]
    assert a["nodes"].sum() == len(nodes) and a["edges"].sum() == len(edges)
    assert len(z) == case.expected()["components"] and z.statistics()[3] == case.expected()["ideal_components"]


def test_new_cases_are_what_they_claim():
    z = zo.from_case(cc.missing_sample_case5())
    t = z.table([f"S{i}" for i in range(5)])
    assert t.present_samples == 5 and t.sample_count == 5
    assert t.missing_sample_counts().tolist() == [3, 0, 5, 0, 2]
    assert t.statistics() == (5, 17, 4, 4)
    three_one = [c for c in z.members if [s for s, _ in c] == [1, 1, 1, 3]]
    assert len(three_one) == 1
    i = z.members.index(three_one[0])
    assert (t.samples[i], t.nodes[i], bool(t.one_short[i]), bool(t.single_copy[i])) == (2, 4, False, False)
    z6 = zo.from_case(cc.missing_sample_case())
    t6 = z6.table([f"S{i}" for i in range(6)])
    assert t6.present_samples == 6 and t6.statistics() == (6, 15, 0, 0)
    assert t6.missing_sample_counts().tolist() == [0, 0, 0, 0, 0, 4]
    w = zo.from_case(cc.wide_case()).table([f"S{i:02d}" for i in range(70)])
    assert w.nodes.tolist() == [70, 69, 69] and w.samples.tolist() == [70, 69, 69]
    assert w.statistics() == (70, 3, 1, 1)
    m = w.missing_sample_counts()
    assert m["S00"] == 1 and m["S64"] == 1 and int(m.sum()) == 2
    for n in (63, 64, 65, 255, 256, 257):
        assert zo.from_case(cc.pairs_case(n)).statistics() == (2, n, n, n)


# ---------------------------------------------------------------------------
# ComponentTable on the hand-written graph
# ---------------------------------------------------------------------------

def hand_table():
    return zo.from_case(cc.hand_case()).table(["A", "B", "C"])


def test_component_table_by_hand():
    t = hand_table()
    assert len(t) == 7 and t.sample_count == 3 and t.present_samples == 3
    assert t.root_sample.tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert t.root_gene.tolist() == [1, 2, 3, 4, 5, 4, 5]
    assert t.nodes.tolist() == [3, 2, 2, 3, 2, 1, 3] and t.nodes.dtype == np.int64
    assert t.edges.tolist() == [3, 1, 1, 2, 1, 0, 2] and t.edges.dtype == np.int64
    assert t.samples.tolist() == [3, 2, 2, 3, 2, 1, 2]
    assert t.offsets.tolist() == [0, 3, 5, 7, 10, 12, 13, 16]
    assert t.complete.tolist() == [True, True, True, False, True, True, False]
    assert t.single_copy.tolist() == [True, True, True, True, True, True, False]
    assert t.ideal.tolist() == [True, False, False, False, False, False, False]
    assert t.large.tolist() == [True, False, False, True, False, False, True]
    assert t.one_short.tolist() == [False, True, True, False, True, False, False]
    assert t.ratio.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2 / 3]
    d = t.density
    assert d[[0, 1, 2, 3, 4, 6]].tolist() == [1.0, 1.0, 1.0, 4 / 6, 1.0, 4 / 6]
    assert np.isnan(d[5]) and np.isnan(d).sum() == 1
    assert t.statistics() == (3, 7, 3, 1)
    assert t.size_histogram().tolist() == [0, 1, 3, 3]
    assert t.sample_histogram().tolist() == [0, 1, 4, 2]
    m = t.missing_sample_counts()
    assert m.index.tolist() == ["A", "B", "C"] and m.tolist() == [0, 1, 2]


def test_component_table_frames():
    t = hand_table()
    df = t.members_of([6, 1])
    assert list(df.columns) == ["component", "sample", "gene"]
    assert df.values.tolist() == [[6, "B", 5], [6, "C", 4], [6, "C", 5], [1, "A", 2], [1, "B", 2]]
    ideal = t.members_of(t.ideal)
    assert ideal.values.tolist() == [[0, "A", 1], [0, "B", 1], [0, "C", 1]]
    assert len(t.members_of()) == 16 and t.members_of()["component"].tolist() == np.repeat(range(7), t.nodes).tolist()
    fr = t.to_frame()
    assert list(fr.columns) == ["component", "root_sample", "root_gene", "nodes", "edges", "samples", "complete",
                                "single_copy", "ideal", "large", "one_short", "ratio", "density"]
    assert len(fr) == 7 and fr["root_sample"].tolist() == ["A"] * 5 + ["B"] * 2
    assert fr["nodes"].tolist() == t.nodes.tolist() and fr["ideal"].tolist() == t.ideal.tolist()


def test_sample_count_is_the_engines_not_the_graphs():
    """With sample_count = 2 (set_sample_count) the pairs are the ideal
    components; one_short still refers to the graph's own three samples."""
    z = zo.Census(*cc.hand_case().graph(), 2)
    t = z.table(["A", "B", "C"])
    assert t.statistics() == (2, 7, 6, 3)
    assert t.ideal.tolist() == [False, True, True, False, True, False, False]
    assert t.one_short.tolist() == [False, True, True, False, True, False, False]


def test_empty_table():
    t = zo.Census(set(), set(), 0).table([])
    assert len(t) == 0 and t.statistics() == (0, 0, 0, 0)
    assert t.size_histogram().tolist() == [0] and t.sample_histogram().tolist() == [0]
    assert len(t.members_of()) == 0 and len(t.to_frame()) == 0 and len(t.missing_sample_counts()) == 0


def test_component_table_checks_its_arrays():
    from rna_clique_amd.census import ComponentTable
    with pytest.raises(ValueError):
        ComponentTable([0], [1], [2], [1], [2], 2, ["A", "B"], [0], [1])   # two nodes, one member
    with pytest.raises(ValueError):
        ComponentTable([0], [1], [2, 2], [1], [2], 2, ["A", "B"], [0, 1], [1, 1])


# ---------------------------------------------------------------------------
# the command's output
# ---------------------------------------------------------------------------

def test_statistics_formats(tmp_path):
    from rna_clique_amd import component_stats as cs
    t = hand_table()
    assert cs.format_statistics(t.statistics(), "h") == ("Samples: 3\nTotal components: 7\n"
                                                         "Components >= samples: 3\nIdeal components: 1\n")
    assert cs.format_statistics(t.statistics(), "m") == "3 7 3 1\n"
    with pytest.raises(ValueError):
        cs.format_statistics(t.statistics(), "x")
    a = cs.build_parser().parse_args(["g.pkl", "--statistics"])
    assert (a.graph, a.statistics, a.samples, a.table, a.device) == ("g.pkl", "h", None, None, 0)
    a = cs.build_parser().parse_args(["g.pkl", "--statistics", "m", "--samples", "4", "--table", "o.tsv"])
    assert (a.statistics, a.samples, a.table) == ("m", 4, "o.tsv")
    assert cs.build_parser().parse_args(["g.pkl"]).statistics is None
    cs.write_table(t, tmp_path / "t.tsv")
    lines = (tmp_path / "t.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(t.to_frame().columns) and len(lines) == 8
    assert lines[1].split("\t")[:6] == ["0", "A", "1", "3", "3", "3"]
    assert lines[6].split("\t")[-1] == ""   # NaN density of the one-node component
