"""The component census on the GPU (components.hip: rc_components,
rc_component_members; census.ComponentTable) against the plain-Python
restatement of tests/census_oracle.py and the reference's recorded components.
Every comparison is exact: integers, or floats from the same expression."""
import ctypes
import functools
import itertools
import json

import numpy as np
import pytest

import census_cases as cc
import census_oracle as zo
import post_cases as pc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

def _graph_engine(case, eng=None):
    """A graph-only engine over a GraphCase (one zero-length transcript per
    gene, then import_edges of the host records)."""
    from rna_clique_amd.engine import Engine
    if eng is None:
        eng = Engine(device=0)
        for s, n in enumerate(case.genes):
            eng.add_sample(f"S{s:02d}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                           np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
        if case.sample_count:
            eng.set_sample_count(case.sample_count)
    eng.import_edges(case.records().view(np.uint8))
    return eng


def _code(fn, *a, **k):
    from rna_clique_amd._native import NativeError
    with pytest.raises(NativeError) as ei:
        fn(*a, **k)
    return ei.value.code


def _census_arrays(eng):
    """Everything the two entry points return, as one dict."""
    t = eng.components()
    t["member_sample"], t["member_gene"] = eng.component_members()
    return t


def _check_census(eng, z):
    """The table, the members and the statistics against the oracle; the
    statistics against Engine.stats(); the ideal rows against
    Engine.ideal_components(). Returns the ComponentTable."""
    from rna_clique_amd.census import ComponentTable
    got, want = eng.components(), z.arrays()
    assert list(got) == ["root_sample", "root_gene", "nodes", "edges", "samples"]
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    ms, mg = eng.component_members()
    es, eg = z.member_arrays()
    assert ms.dtype == np.int32 and np.array_equal(ms, es) and np.array_equal(mg, eg)
    t = ComponentTable.from_engine(eng)
    st = eng.stats()
    assert t.statistics() == z.statistics()
    assert t.statistics() == (st["sample_count"], st["components"], int((got["nodes"] >= st["sample_count"]).sum()),
                              st["ideal_components"])
    assert len(ms) == st["nodes"] and int(got["edges"].sum()) == sum(z.edges)
    s, g = eng.ideal_components()
    ideal = t.members_of(t.ideal)
    assert ideal["sample"].tolist() == [eng.labels[i] for i in s.ravel().tolist()]
    assert ideal["gene"].tolist() == g.ravel().tolist()
    assert np.flatnonzero(t.ideal).tolist() == z.ideal_ids()
    return t


# ---------------------------------------------------------------------------
# 1. the record cases of test_gpu_components
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _record_cases():
    out = {}
    for S in (3, 4, 6):
        c = pc.cliques_case(S)
        out[f"cliques{S}-pair-major"] = c.pair_major()
        out[f"cliques{S}-permuted"] = c.permuted(33 + S)
    out["node-only"] = pc.node_only_case()
    out["node-only-count3"] = pc.node_only_case(extra_sample=True, sample_count=3)
    out["star"] = pc.star_case(n=200)
    out["chain"] = pc.chain_case(n=200)
    small = pc.cliques_case(3, n_each=30, seed=22).permuted(34)
    for n in (0, 1, 63, 64, 65, 257):
        out[f"prefix{n}"] = small.prefix(n)
    return out


RECORD_CASES = ["cliques3-pair-major", "cliques3-permuted", "cliques4-pair-major", "cliques4-permuted",
                "cliques6-pair-major", "cliques6-permuted", "node-only", "node-only-count3", "star", "chain",
                "prefix0", "prefix1", "prefix63", "prefix64", "prefix65", "prefix257"]


@pytest.mark.parametrize("name", RECORD_CASES)
def test_record_cases(native, name):
    """Ideal cliques, cliques with one edge missing, two cliques joined,
    S - 1 cliques and sums-only extras (which join nothing), node-only records
    with and without a given sample count, a star, a chain and record counts
    around 64 and 256."""
    case = _record_cases()[name]
    z = zo.from_case(case)
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, z)
        if name.startswith("cliques"):
            S = len(case.genes)
            # per 25: one ideal, one an edge short, one of 2 S nodes, one over S - 1 samples
            assert t.statistics() == (S, 100, 75, 25)
            assert int(t.one_short.sum()) == 25 and int(t.missing_sample_counts().sum()) == 25
            assert sorted(set(t.nodes.tolist())) == [S - 1, S, 2 * S]
        if name == "node-only-count3":
            assert t.sample_count == 3 and t.present_samples == 4 and t.statistics()[3] == 30
            assert int((t.nodes == 1).sum()) == 5 and np.isnan(t.density).sum() == 5
        if name == "chain":
            assert t.statistics() == (2, 1, 1, 0) and t.nodes.tolist() == [400] and t.edges.tolist() == [399]
        if name == "prefix0":
            assert len(t) == 0 and t.statistics() == (0, 0, 0, 0) and len(t.member_sample) == 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 2. the scan and the scatter around a wave and a block
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_component_counts_around_block_sizes(native, n):
    case = cc.pairs_case(n).permuted(n)
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        assert t.statistics() == (2, n, n, n)
        assert t.root_gene.tolist() == list(range(1, n + 1)) and t.offsets.tolist() == list(range(0, 2 * n + 1, 2))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 3. one giant component
# ---------------------------------------------------------------------------

def test_giant_chain(native):
    """chain_case(20000), permuted: 40 000 members, 39 999 edges, 2 samples.
    The member slice crosses every block boundary; samples counts each of the
    two samples once."""
    case = pc.chain_case(20000).permuted(31)
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        assert (t.nodes.tolist(), t.edges.tolist(), t.samples.tolist()) == ([40000], [39999], [2])
        assert t.member_sample.tolist() == [0] * 20000 + [1] * 20000
        assert t.member_gene.tolist() == 2 * list(range(1, 20001))
    finally:
        eng.close()


def test_giant_star(native):
    case = pc.star_case(20000).permuted(32)
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        assert (int(t.nodes[0]), int(t.edges[0]), int(t.samples[0])) == (20001, 20000, 2)
        assert t.statistics() == (2, 51, 51, 50)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 4., 5. sample boundaries inside a member slice; more samples than lanes
# ---------------------------------------------------------------------------

def test_missing_samples(native):
    """S - 1 cliques lacking the first, a middle and the last sample a known
    number of times; three genes of one sample and one of another in one
    component; a node-only gene."""
    case = cc.missing_sample_case5().permuted(5)
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        m = t.missing_sample_counts()
        assert m.index.tolist() == eng.labels and m.tolist() == [3, 0, 5, 0, 2]
        assert t.statistics() == (5, 17, 4, 4)
        i = next(c for c in range(len(t)) if t.members_of([c])["sample"].tolist() == ["S01", "S01", "S01", "S03"])
        assert (int(t.samples[i]), int(t.nodes[i]), int(t.edges[i])) == (2, 4, 3)
    finally:
        eng.close()


def test_sample_known_from_a_node_only_record(native):
    """A sixth sample whose only node is a node-only record raises P to 6:
    the 5-cliques are one short of it, nothing is ideal; with
    set_sample_count(5) they are ideal and still one_short."""
    from rna_clique_amd.census import ComponentTable
    case = cc.missing_sample_case()
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        assert t.statistics() == (6, 15, 0, 0) and t.missing_sample_counts().tolist() == [0, 0, 0, 0, 0, 4]
        assert (int(t.nodes[-1]), int(t.samples[-1]), int(t.root_sample[-1])) == (1, 1, 5)
    finally:
        eng.close()
    case.sample_count = 5
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        assert t.statistics() == (5, 15, 4, 4) and t.missing_sample_counts().tolist() == [0, 0, 0, 0, 0, 4]
        assert isinstance(t, ComponentTable)
    finally:
        eng.close()


def test_more_samples_than_lanes(native):
    """70 samples: a 70-clique, a 69-clique lacking sample 64 and one lacking
    sample 0."""
    case = cc.wide_case().permuted(70)
    eng = _graph_engine(case)
    try:
        t = _check_census(eng, zo.from_case(case))
        assert t.nodes.tolist() == [70, 69, 69] and t.samples.tolist() == [70, 69, 69]
        assert t.edges.tolist() == [70 * 69 // 2, 69 * 68 // 2, 69 * 68 // 2]
        assert t.statistics() == (70, 3, 1, 1) and t.one_short.tolist() == [False, True, True]
        m = t.missing_sample_counts()
        assert np.flatnonzero(m.to_numpy()).tolist() == [0, 64] and m.tolist()[0] == 1 and m.tolist()[64] == 1
        # the second component lacks sample 64 (its root is in sample 0), the third sample 0
        assert t.root_sample.tolist() == [0, 0, 1]
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 6. record order
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("S", [3, 6])
def test_record_order_does_not_matter(native, S):
    base = pc.cliques_case(S)
    got = []
    for case in (base.pair_major(), base.permuted(1), base.permuted(2)):
        eng = _graph_engine(case)
        try:
            got.append(_census_arrays(eng))
        finally:
            eng.close()
    for other in got[1:]:
        assert list(other) == list(got[0])
        for k in got[0]:
            assert np.array_equal(other[k], got[0][k]), k


# ---------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------

def _rc_components(eng, cap, n_bufs=5):
    """rc_components through the bindings with `cap` entries in the first
    n_bufs buffers (the rest NULL). Returns (code, n_comp)."""
    from rna_clique_amd import _native as nat
    dts = [np.int32, np.int32, np.int64, np.int64, np.int32]
    bufs = [np.zeros(max(cap, 1), dtype=d) for d in dts]
    ptrs = [b.ctypes.data_as(ctypes.c_void_p) if i < n_bufs else None for i, b in enumerate(bufs)]
    n = ctypes.c_uint64()
    return nat.lib().rc_components(eng._h, *ptrs, cap, ctypes.byref(n)), n.value


def test_state_and_argument_errors(native):
    from rna_clique_amd import _native as nat
    from rna_clique_amd.engine import Engine
    case = _record_cases()["cliques3-pair-major"]
    eng = Engine(device=0)
    try:
        for s, n in enumerate(case.genes):
            eng.add_sample(f"S{s:02d}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                           np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
        # nothing has run
        assert _code(eng.components) == nat.RC_E_STATE
        assert _code(eng.component_members) == nat.RC_E_STATE
        _graph_engine(case, eng)
        k = len(zo.from_case(case))
        assert _rc_components(eng, k) == (nat.RC_OK, k)
        assert _rc_components(eng, k - 1) == (nat.RC_E_CAPACITY, k)
        assert _rc_components(eng, k, n_bufs=4) == (nat.RC_E_ARG, k)
        assert _rc_components(eng, 0, n_bufs=0) == (nat.RC_OK, k)
        L, n = nat.lib(), ctypes.c_uint64()
        nn = eng.stats()["nodes"]
        s, g = np.zeros(nn, np.int32), np.zeros(nn, np.int32)
        vp = ctypes.c_void_p
        assert L.rc_component_members(eng._h, s.ctypes.data_as(vp), g.ctypes.data_as(vp), nn - 1,
                                      ctypes.byref(n)) == nat.RC_E_CAPACITY and n.value == nn
        assert L.rc_component_members(eng._h, s.ctypes.data_as(vp), None, nn, ctypes.byref(n)) == nat.RC_E_ARG
        assert L.rc_component_members(eng._h, s.ctypes.data_as(vp), g.ctypes.data_as(vp), nn,
                                      ctypes.byref(n)) == nat.RC_OK
        assert np.array_equal(s, zo.from_case(case).member_arrays()[0])
    finally:
        eng.close()


def test_an_aligning_engine_before_finish(native):
    """Samples uploaded and aligned but not finished: RC_E_STATE."""
    from rna_clique_amd import _native as nat
    from rna_clique_amd.engine import Engine
    case = next(c for c in pc.fixture_cases() if c.name == "tie-across-genes")
    eng = Engine(device=0)
    try:
        for s in case.samples:
            tx = case.transcripts[s]
            eng.add_sample(s, np.frombuffer(b"ACGT" * 50 * len(tx), dtype=np.uint8),
                           np.arange(len(tx) + 1, dtype=np.uint64) * 200, [g for g, _ in tx], [i for _, i in tx])
        for (q, s), arr in sorted(case.hsp_arrays().items()):
            eng.add_hsps(q, s, arr)
        eng.align()
        assert _code(eng.components) == nat.RC_E_STATE
        eng.finish()
        assert len(eng.components()["nodes"]) == eng.stats()["components"] == 8
    finally:
        eng.close()


def test_a_new_graph_phase_invalidates_the_census(native):
    first = _record_cases()["cliques3-pair-major"]
    second = pc.GraphCase("second", first.genes, pc.cliques_case(3).permuted(2).recs[:150])
    z1, z2 = zo.from_case(first), zo.from_case(second)
    assert z1.multiset() != z2.multiset()
    eng = _graph_engine(first)
    try:
        _check_census(eng, z1)
        _graph_engine(second, eng)
        _check_census(eng, z2)
        eng.ideal_components()   # the other per-component tables, then the census again
        _check_census(eng, z2)
    finally:
        eng.close()


def test_trim_keeps_the_census(native):
    case = _record_cases()["cliques4-permuted"]
    eng = _graph_engine(case)
    try:
        before = _census_arrays(eng)
        eng.trim()
        after = _census_arrays(eng)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        _check_census(eng, zo.from_case(case))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 8. the reference's recorded components through the engine
# ---------------------------------------------------------------------------

def _run_case(case, top, keep):
    from rna_clique_amd.engine import Engine
    eng = Engine(device=0, top_matches=top, keep_all=keep)
    for s in case.samples:
        tx = case.transcripts[s]
        seq = np.frombuffer(b"ACGT" * 50 * len(tx), dtype=np.uint8)
        eng.add_sample(s, seq, np.arange(len(tx) + 1, dtype=np.uint64) * 200, [g for g, _ in tx], [i for _, i in tx])
    for (q, s), arr in sorted(case.hsp_arrays().items()):
        eng.add_hsps(q, s, arr)
    eng.align()
    eng.finish()
    return eng


def _engine_multiset(t):
    """ComponentTable -> sorted [(members as ((sample id, gene), ...), edges)]."""
    out = []
    for c in range(len(t)):
        lo, hi = t.offsets[c], t.offsets[c + 1]
        out.append((tuple(zip(t.member_sample[lo:hi].tolist(), t.member_gene[lo:hi].tolist())), int(t.edges[c])))
    return sorted(out)


FIXTURE_NAMES = [c.name for c in pc.fixture_cases()]


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_recorded_reference_components(native, name):
    """The fixture HSP tables through add_hsps and finish: the census equals
    the reference's component_subgraphs as multisets of (members, edges) at
    (1, keep_all), (3, keep_all) and (3, keep first), and its statistics are
    the reference's."""
    from rna_clique_amd.census import ComponentTable
    from test_census_host import SETTINGS, fixture_multiset, golden
    case = next(c for c in pc.fixture_cases() if c.name == name)
    fx = golden()["cases"][name]
    for top, keep in SETTINGS:
        exp = fx["expected"][f"{top}-{keep}"]
        eng = _run_case(case, top, keep)
        try:
            t = ComponentTable.from_engine(eng)
            assert _engine_multiset(t) == fixture_multiset(exp)
            S = exp["sample_count"]
            assert t.statistics() == (S, len(exp["components"]),
                                      sum(len(c["members"]) >= S for c in exp["components"]), exp["ideal_components"])
        finally:
            eng.close()


# ---------------------------------------------------------------------------
# 9. an aligned run, end to end
# ---------------------------------------------------------------------------

def _by_root(t):
    """Rows keyed by (root label, root gene): what two engines that order the
    samples differently agree on."""
    f = t.to_frame()
    rows = {}
    for r in f.itertuples(index=False):
        m = t.members_of([r.component])
        rows[(r.root_sample, r.root_gene)] = (r.nodes, r.edges, r.samples, r.ideal, r.large, r.one_short,
                                              sorted(zip(m["sample"], m["gene"])))
    return rows


def test_aligned_run_end_to_end(native, tmp_path):
    """5 samples x 200 genes aligned by the engine: the census against the
    oracle on the engine's own edges, through SampleSimilarity, and again from
    the run's written graph.pkl and tables."""
    from rna_clique_amd.engine import Engine
    from rna_clique_amd.similarity import SampleSimilarity
    from rna_clique_amd.simulate import simulate
    from rna_clique_amd.tables import write_engine_outputs
    samples, _ = simulate(5, 200, seed=11, p_iso2=0.2, indel_rate=0.002)
    eng = Engine(device=0)
    try:
        for s in samples:
            eng.add_sample(s.name, s.seq, s.tx_offsets, s.gene, s.iso)
        eng.run()
        edges = {tuple(sorted(((int(e["sample_a"]), int(e["gene_a"])), (int(e["sample_b"]), int(e["gene_b"])))))
                 for e in eng.edges()}
        nodes = {v for e in edges for v in e}
        z = zo.Census(nodes, edges, len({s for s, _ in nodes}))
        t = _check_census(eng, z)
        assert len(t) > 20 and t.statistics()[3] > 20
        sim = SampleSimilarity.from_engine(eng)
        ts = sim.components()
        assert ts.statistics() == t.statistics() and ts.labels == list(eng.labels)
        for k in ("root_sample", "root_gene", "nodes", "edges", "samples", "member_sample", "member_gene"):
            assert np.array_equal(getattr(ts, k), getattr(t, k)), k
        ideal = sim.ideal_components()
        assert ts.members_of(ts.ideal)[["sample", "gene"]].values.tolist() == ideal[["sample", "gene"]].values.tolist()
        # the written outputs, read back: a graph-only engine of its own, samples in label order
        pairs = list(itertools.combinations(range(5), 2))
        fns = [tmp_path / f"t{a}_{b}.h5" for a, b in pairs]
        write_engine_outputs(eng, pairs, fns, tmp_path / "graph.pkl")
        back = SampleSimilarity.from_filenames(tmp_path / "graph.pkl", fns)
        try:
            tb = back.components()
            assert tb.statistics() == t.statistics()
            assert sorted(_by_root(tb).values(), key=repr) == sorted(_by_root(t).values(), key=repr)
            if list(back.labels) == list(eng.labels):
                assert _by_root(tb) == _by_root(t)
            assert tb.missing_sample_counts().sort_index().tolist() == t.missing_sample_counts().sort_index().tolist()
            assert np.array_equal(tb.size_histogram(), t.size_histogram())
            assert np.array_equal(tb.sample_histogram(), t.sample_histogram())
        finally:
            back.engine.close()
        # graph.pkl alone, as the command reads it
        from rna_clique_amd import component_stats as cs
        assert cs.main([str(tmp_path / "graph.pkl"), "--table", str(tmp_path / "c.tsv")]) == 0
        assert len((tmp_path / "c.tsv").read_text().splitlines()) == len(t) + 1
    finally:
        eng.close()


def test_command_statistics(native, tmp_path, capsys):
    """python -m rna_clique_amd.component_stats on a written graph: both
    formats, and --samples."""
    import networkx as nx
    from rna_clique_amd import component_stats as cs
    from rna_clique_amd.filtering_step import dump_graph
    case = cc.hand_case()
    nodes, edges = case.graph()
    g = nx.Graph()
    g.add_nodes_from((f"s{s}", gene) for s, gene in nodes)
    g.add_edges_from(((f"s{u[0]}", u[1]), (f"s{v[0]}", v[1])) for u, v in edges)
    dump_graph(g, tmp_path / "graph.pkl")
    assert cs.main([str(tmp_path / "graph.pkl"), "--statistics"]) == 0
    assert capsys.readouterr().out == ("Samples: 3\nTotal components: 7\nComponents >= samples: 3\n"
                                       "Ideal components: 1\n")
    assert cs.main([str(tmp_path / "graph.pkl"), "--statistics", "m", "--samples", "2"]) == 0
    assert capsys.readouterr().out == "2 7 6 3\n"
