"""Per-component tables and resampling on the GPU (components.hip:
rc_ideal_components, rc_component_sums, rc_resample) against the plain-Python
restatement of tests/component_oracle.py. Every integer is compared exactly;
distances equal the float64 (den - num) / den of the expected integers and,
where den < 2^53, float(1 - Fraction(num, den)). No tolerance anywhere."""
import functools
import itertools

import numpy as np
import pytest

import component_oracle as co
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
            eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
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


def _sums_matrix(eng, vec):
    """A (P,) vector of pair values -> the N x N matrix of Engine.pair_sums()."""
    n = len(eng.labels)
    out = np.zeros((n, n), dtype=np.int64)
    for p, (a, b) in enumerate(eng.pair_order()):
        out[a, b] = out[b, a] = vec[p]
    return out


def _check_tables(eng, t):
    """Ids and members, both sum tables, and the invariant: summed over the
    components the table is pair_sums()."""
    n = len(eng.labels)
    assert eng.pair_order() == sorted(itertools.combinations(range(n), 2), key=lambda p: co.pair_index(*p))
    s, g = eng.ideal_components()
    es, eg = t.member_arrays()
    assert s.shape == es.shape and np.array_equal(s, es) and np.array_equal(g, eg)
    assert eng.stats()["ideal_components"] == t.n_components == eng.n_components()
    num, den = eng.component_sums()
    en, ed = t.sums_int64()
    assert num.shape == (t.n_components, t.n_pairs) and num.dtype == np.int64
    assert np.array_equal(num, en) and np.array_equal(den, ed)
    pn, pd_ = eng.pair_sums()
    assert np.array_equal(_sums_matrix(eng, num.sum(axis=0)), pn)
    assert np.array_equal(_sums_matrix(eng, den.sum(axis=0)), pd_)


def _check_resample(eng, t, W, order=None, exact=True):
    """One resample call against the helper: sums, distances, NaN placement
    and the return code."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    W = np.asarray(W)
    en, ed = t.resample(W)
    n = len(eng.labels)
    idx = sorted(range(n), key=lambda i: eng.labels[i]) if order is None else list(order)
    want = co.distances_from_sums(en, ed, idx)
    labels, mats, (num, den) = eng.resample(W, order, sums=True, allow_nan=True)
    assert labels == [eng.labels[i] for i in idx]
    assert np.array_equal(num, en.astype(np.int64)) and np.array_equal(den, ed.astype(np.int64))
    assert mats.shape == want.shape and np.array_equal(mats, want, equal_nan=True)
    if exact:
        assert max((int(x) for x in ed.ravel()), default=0) < 2 ** 53
        assert np.array_equal(mats, co.distances_from_sums(en, ed, idx, exact=True), equal_nan=True)
    if np.isnan(want).any():
        assert _code(eng.resample, W, order) == RC_E_NO_IDEAL
    else:
        assert np.array_equal(eng.resample(W, order)[1], want)
    return mats


def _check_ones(eng, t):
    """All-ones weights: pair_sums() and Engine.distance() bit for bit (or
    RC_E_NO_IDEAL from both, NaN exactly at the pairs without rows)."""
    from rna_clique_amd._native import NativeError, RC_E_NO_IDEAL
    W = np.ones((1, t.n_components), dtype=np.uint16)
    labels, mats, (num, den) = eng.resample(W, sums=True, allow_nan=True)
    pn, pd_ = eng.pair_sums()
    assert np.array_equal(_sums_matrix(eng, num[0]), pn) and np.array_equal(_sums_matrix(eng, den[0]), pd_)
    idx = [eng.labels.index(x) for x in labels]
    assert np.array_equal(np.isnan(mats[0]), (pd_[np.ix_(idx, idx)] == 0) & ~np.eye(len(idx), dtype=bool))
    try:
        l2, d = eng.distance()
    except NativeError as e:
        assert e.code == RC_E_NO_IDEAL and np.isnan(mats).any()
        assert _code(eng.resample, W) == RC_E_NO_IDEAL
        return
    assert l2 == labels and np.array_equal(d, mats[0])


def _weights(rng, R, C):
    """Random uint16 weights whose values include 0 and 65535 (when there is
    room), a third of them zero like bootstrap counts."""
    W = rng.integers(0, 65536, size=(R, C)).astype(np.uint16)
    W[rng.random((R, C)) < 0.35] = 0
    flat = W.reshape(-1)
    if flat.size >= 2:
        flat[rng.integers(flat.size)] = 65535
        flat[(int(np.argmax(flat)) + 1) % flat.size] = 0
    return W


# ---------------------------------------------------------------------------
# graph-only engines on record cases
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
    """Ids, members, both sum tables and sum over components == pair_sums on
    pair-major and permuted cliques (with sums-only records between two ideal
    components: the attribution rule), node-only records, S < N, a star, a
    chain without ideal components and record counts around 64 and 256."""
    from rna_clique_amd._native import RC_E_ARG
    case = _record_cases()[name]
    t = co.from_case(case)
    eng = _graph_engine(case)
    try:
        _check_tables(eng, t)
        _check_ones(eng, t)
        C = t.n_components
        if name.startswith("cliques"):
            assert C == 25 and t.crossing == 25
        if name == "star":
            assert C == 50 and t.sample_count == 2
        if name == "node-only-count3":
            # S = 3 < N = 4: the fourth sample's pairs have all-zero columns, NaN exactly there
            assert C == 30 and eng.ideal_components()[0].shape == (30, 3)
            num, den = eng.component_sums()
            cols = [p for p, (a, b) in enumerate(eng.pair_order()) if b == 3]
            assert len(cols) == 3 and not den[:, cols].any() and den[:, [p for p in range(6) if p not in cols]].all()
            _, mats = eng.resample(np.ones((2, C), dtype=np.uint16), [0, 1, 2, 3], allow_nan=True)
            nan = np.zeros((4, 4), dtype=bool)
            nan[3, :3] = nan[:3, 3] = True
            assert np.array_equal(np.isnan(mats[0]), nan) and np.array_equal(np.isnan(mats[1]), nan)
            # without the fourth sample the matrix is whole
            assert not np.isnan(eng.resample(np.ones((1, C), dtype=np.uint16), [2, 0, 1])[1]).any()
        if C == 0:
            s, g = eng.ideal_components()
            assert s.shape[0] == 0 and g.shape[0] == 0
            num, den = eng.component_sums()
            assert num.shape == (0, t.n_pairs) and den.shape == (0, t.n_pairs)
            for bad in (1, 2, 64):
                assert _code(eng.resample, np.ones((1, bad), dtype=np.uint16)) == RC_E_ARG
        else:
            _check_resample(eng, t, _weights(np.random.default_rng(len(name)), 9, C))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# resample shapes
# ---------------------------------------------------------------------------

SHAPES = [(S, C) for S in (2, 3, 6, 12) for C in (1, 63, 64, 65, 257, 1000)]


@pytest.mark.parametrize("S,C", SHAPES, ids=[f"S{S}-C{C}" for S, C in SHAPES])
def test_resample_shapes(native, S, C):
    """One pair-major clique family with C ideal components over S samples
    (P = 1, 3, 15, 66 pairs: less than, and more than, one 64-lane pair tile;
    C around the 128-component weight tile and the 4-row unroll), replicates
    R = 1, 7, 8, 9, 65 around the 8 replicates of a wave and the 32 of a
    block: random weights with 0 and 65535, all ones, the identity, all-zero
    rows, and a permuted subset of the samples as order."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    case = pc.cliques_case(S, n_each=C, extras=S > 2).pair_major()
    t = co.from_case(case)
    assert t.n_components == C and t.n_pairs == S * (S - 1) // 2
    eng = _graph_engine(case)
    rng = np.random.default_rng(1000 * S + C)
    try:
        _check_tables(eng, t)
        _check_ones(eng, t)
        sub = [int(x) for x in rng.permutation(S)[:max(2, S - 1)]]
        for R in (1, 7, 8, 9, 65):
            W = _weights(rng, R, C)
            _check_resample(eng, t, W)
            _check_resample(eng, t, W, order=sub)
        # the identity returns each component's own row
        _, _, (num, den) = eng.resample(np.eye(C, dtype=np.uint16), sums=True)
        en, ed = t.sums_int64()
        assert np.array_equal(num, en) and np.array_equal(den, ed)
        # all-zero rows: NaN everywhere off the diagonal, the other rows untouched
        W = _weights(rng, 9, C)
        W[W == 0] = 1
        W[[0, 8]] = 0
        mats = _check_resample(eng, t, W)
        off = ~np.eye(S, dtype=bool)
        assert np.isnan(mats[0][off]).all() and np.isnan(mats[8][off]).all() and not np.isnan(mats[1:8]).any()
        assert _code(eng.resample, W) == RC_E_NO_IDEAL
    finally:
        eng.close()


def test_64_bit_accumulation(native):
    """large_sums_case(n=3000): cells near 2^31, pair sums near 6.4e12; with
    weights of 65535 the totals are near 4e17 (past 2^53), exact."""
    case = pc.large_sums_case(n=3000)
    t = co.from_case(case)
    eng = _graph_engine(case)
    try:
        assert t.n_components == 3000 and int(t.den.max()) > 2 ** 30
        _check_tables(eng, t)
        _check_ones(eng, t)
        W = _weights(np.random.default_rng(4), 3, 3000)
        W[0] = 65535
        en, ed = t.resample(W)
        assert int(ed[0, 0]) > 4 * 10 ** 17 and int(ed[0, 0]) < 2 ** 63
        _check_resample(eng, t, W, exact=False)
        _check_resample(eng, t, np.ones((1, 3000), dtype=np.uint16))   # den < 2^53: also the exact Fraction
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------

def test_stacked_sum_only_records_hit_the_cell_limit(native):
    """Three sums-only records near 2^31 on one (component, pair) cell:
    rc_component_sums is exact, rc_resample refuses with RC_E_LIMIT."""
    from rna_clique_amd._native import RC_E_LIMIT
    top = 2 ** 31 - 1
    recs = [(pc.EDGE, (0, 1), (1, 1), 90, 100), (pc.EDGE, (0, 2), (1, 2), 80, 100)]
    recs += [(pc.SUM_ONLY, (0, 1), (1, 1), top - 7 - k, top - k) for k in range(3)]
    case = pc.GraphCase("stacked", [2, 2], recs)
    t = co.from_case(case)
    assert t.n_components == 2 and int(t.den[0, 0]) == 3 * top - 3 + 100 >= 2 ** 32
    eng = _graph_engine(case)
    try:
        _check_tables(eng, t)
        assert _code(eng.resample, np.ones((1, 2), dtype=np.uint16)) == RC_E_LIMIT
    finally:
        eng.close()


def test_weight_times_denominator_limit(native):
    """large_sums_case(n=70000): the pair's denominator is about 1.5e14, and
    65535 x 1.5e14 >= 2^63: RC_E_LIMIT; weights of 1 pass."""
    from rna_clique_amd._native import RC_E_LIMIT
    case = pc.large_sums_case(n=70000)
    eng = _graph_engine(case)
    try:
        _, den = eng.pair_sums()
        assert 65535 * int(den[0, 1]) >= 2 ** 63 > 61000 * int(den[0, 1])
        W = np.ones((2, 70000), dtype=np.uint16)
        labels, mats = eng.resample(W)
        assert np.array_equal(mats[0], eng.distance()[1]) and np.array_equal(mats[1], mats[0])
        W[1, 69999] = 65535
        assert _code(eng.resample, W) == RC_E_LIMIT
    finally:
        eng.close()


def test_argument_and_state_errors(native):
    from rna_clique_amd._native import RC_E_ARG, RC_E_STATE
    from rna_clique_amd.engine import Engine
    case = _record_cases()["cliques3-pair-major"]
    eng = Engine(device=0)
    try:
        for s, n in enumerate(case.genes):
            eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                           np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
        # nothing has run: every call is out of order
        assert _code(eng.ideal_components) == RC_E_STATE
        assert _code(eng.component_sums) == RC_E_STATE
        assert _code(eng.resample, np.ones((1, 25), dtype=np.uint16)) == RC_E_STATE
        _graph_engine(case, eng)
        assert eng.n_components() == 25
        for bad in (24, 26):
            assert _code(eng.resample, np.ones((1, bad), dtype=np.uint16)) == RC_E_ARG
        assert _code(eng.resample, np.ones((0, 25), dtype=np.uint16)) == RC_E_ARG
        for order in ([0, 0, 1], [0, 3], [-1, 1], [0, 1, 2, 1]):
            assert _code(eng.resample, np.ones((1, 25), dtype=np.uint16), order) == RC_E_ARG
        with pytest.raises(ValueError):
            eng.resample(np.full((1, 25), 65536))
        with pytest.raises(ValueError):
            eng.resample(np.full((1, 25), -1))
        with pytest.raises(TypeError):
            eng.resample(np.ones((1, 25)))
        with pytest.raises(ValueError):
            eng.resample(np.ones(25, dtype=np.uint16))
    finally:
        eng.close()


def test_a_new_graph_phase_invalidates_the_tables(native):
    """Two import_edges calls with different record sets on one engine: the
    answers after the second follow the second set."""
    first = _record_cases()["cliques3-pair-major"]
    second = pc.GraphCase("second", first.genes, pc.cliques_case(3).permuted(2).recs[:150])
    t1, t2 = co.from_case(first), co.from_case(second)
    assert 0 < t2.n_components < t1.n_components
    eng = _graph_engine(first)
    try:
        _check_tables(eng, t1)
        _check_resample(eng, t1, _weights(np.random.default_rng(1), 8, t1.n_components))
        _graph_engine(second, eng)
        _check_tables(eng, t2)
        _check_ones(eng, t2)
        _check_resample(eng, t2, _weights(np.random.default_rng(2), 8, t2.n_components))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# an aligned run, end to end
# ---------------------------------------------------------------------------

def _run_tables(eng, labels):
    """The helper's tables from an aligned engine's own rows and edges, with
    samples indexed as in `labels`."""
    n = len(eng.labels)
    ix = [labels.index(x) for x in eng.labels]
    recs = []
    for a, b in itertools.combinations(range(n), 2):
        rows = eng.pair_rows(a, b)
        for sg, qg, ni, ln, gp in zip(rows["sgene"].tolist(), rows["qgene"].tolist(), rows["hsp"]["nident"].tolist(),
                                      rows["hsp"]["length"].tolist(), rows["hsp"]["gaps"].tolist()):
            recs.append(((ix[a], sg), (ix[b], qg), ni, ln - gp))
    edges = {tuple(sorted(((ix[e["sample_a"]], int(e["gene_a"])), (ix[e["sample_b"]], int(e["gene_b"])))))
             for e in eng.edges()}
    nodes = {v for e in edges for v in e}
    return co.ComponentTables(recs, nodes, edges, len({s for s, _ in nodes}), n)


def _support(full, reps, labels):
    import treecheck
    splits = sorted(treecheck.nj_splits(full, labels), key=sorted)
    rep_splits = [treecheck.nj_splits(m, labels) for m in reps]
    return [sum(s in rs for rs in rep_splits) / len(reps) for s in splits]


def _check_similarity(sim, t):
    """SampleSimilarity's component interface against the helper whose
    samples are indexed as sim.labels."""
    from rna_clique_amd.similarity import bootstrap_weights
    order = [sim.labels.index(s) for s in sim.samples]
    full = sim.get_dissimilarity_matrix()
    C = t.n_components
    ones = sim.resampled_dissimilarity_matrices(np.ones((1, C), dtype=np.uint16))
    assert ones.shape == (1,) + full.shape and np.array_equal(ones[0], full)
    W = bootstrap_weights(C, 64, seed=1)
    boot = sim.bootstrap_dissimilarity_matrices(64, seed=1)
    en, ed = t.resample(W)
    assert np.array_equal(boot, co.distances_from_sums(en, ed, order))
    assert np.array_equal(boot, co.distances_from_sums(en, ed, order, exact=True))
    sup = _support(full, boot, sim.samples)
    assert sup and all(0.0 <= x <= 1.0 for x in sup)
    assert sup == _support(full, sim.bootstrap_dissimilarity_matrices(64, seed=1), sim.samples)
    return boot


def test_aligned_run_end_to_end(native, tmp_path):
    """5 samples x 200 genes aligned by the engine: components, sums, the
    DataFrame and the mask, the all-ones replicate, 64 bootstrap replicates
    and split support through neighbour joining -- from the engine and again
    from the run's written graph.pkl and tables."""
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
        t = _run_tables(eng, list(eng.labels))
        assert t.n_components > 20
        _check_tables(eng, t)
        _check_ones(eng, t)
        sim = SampleSimilarity.from_engine(eng)
        df = sim.ideal_components()
        es, eg = t.member_arrays()
        assert list(df.columns) == ["component", "sample", "gene"]
        assert df["component"].tolist() == np.repeat(np.arange(t.n_components), 5).tolist()
        assert df["sample"].tolist() == [eng.labels[i] for i in es.ravel().tolist()]
        assert df["gene"].tolist() == eg.ravel().tolist()
        assert sorted(zip(df["sample"], df["gene"])) == sorted(zip(sim.valid["sample"], sim.valid["gene"]))
        mask = sim.contributing_components()
        en, ed = t.sums_int64()
        assert mask.dtype == bool and np.array_equal(mask, (ed - en).sum(axis=1) > 0) and mask.any()
        num, den = sim.component_sums()
        assert np.array_equal(num, en) and np.array_equal(den, ed)
        boot = _check_similarity(sim, t)
        # the written outputs, read back: a graph-only engine of its own
        pairs = list(itertools.combinations(range(5), 2))
        fns = [tmp_path / f"t{a}_{b}.h5" for a, b in pairs]
        write_engine_outputs(eng, pairs, fns, tmp_path / "graph.pkl")
        back = SampleSimilarity.from_filenames(tmp_path / "graph.pkl", fns)
        try:
            assert back.samples == sim.samples
            tb = _run_tables(eng, list(back.labels))
            _check_tables(back.engine, tb)
            assert np.array_equal(_check_similarity(back, tb), boot)
            assert np.array_equal(back.contributing_components().sum(), mask.sum())
        finally:
            back.engine.close()
    finally:
        eng.close()
