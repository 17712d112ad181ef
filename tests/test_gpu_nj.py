"""Neighbour-joining trees and split support on the GPU (nj.hip: rc_nj,
rc_resample_trees) against tests/nj_oracle.py. Joins, splits and valid are
compared exactly and branch lengths as bits: the operation order is the
specification, so there is no tolerance anywhere."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import nj_cases as nc
import nj_oracle as no
import post_cases as pc
import treecheck

pytestmark = pytest.mark.gpu

LDS_SIZES = (3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 127, 128)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

def _engine():
    from rna_clique_amd.engine import Engine
    return Engine(device=0)


def _code(fn, *a, **k):
    from rna_clique_amd._native import NativeError
    with pytest.raises(NativeError) as ei:
        fn(*a, **k)
    return ei.value.code


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """Seven matrices of n samples and the oracle's trees of them (computed
    once, shared by the tests): noisy additive, exact additive with integer
    branch lengths (ties in q), all-equal (every q ties), random symmetric
    non-metric (negative lengths), the first with garbage below and on the
    diagonal, and two more noisy additive ones. tie_free: indices whose tree
    the independent treecheck.nj_splits must give too."""
    Ds = np.stack([nc.noisy_additive(n, seed=n)[0], nc.additive(n, seed=n + 1, integer=True)[0], nc.all_equal(n),
                   nc.random_symmetric(n, seed=n + 2), nc.with_garbage(nc.noisy_additive(n, seed=n)[0], seed=n + 3),
                   nc.noisy_additive(n, seed=n + 4)[0], nc.noisy_additive(n, seed=n + 5)[0]])
    Ds.setflags(write=False)
    want = no.nj_batch(Ds)
    for a in want:
        a.setflags(write=False)
    return Ds, want, (0, 3, 5, 6)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(res, want, rows=None):
    """res (NJResult) equals the oracle's (joins, lengths, splits, valid)."""
    joins, lengths, splits, valid = (w if rows is None else w[rows] for w in want)
    assert res.joins.shape == joins.shape and np.array_equal(res.joins, joins)
    assert res.splits.shape == splits.shape and np.array_equal(res.splits, splits)
    assert np.array_equal(res.valid, valid)
    ok = valid.astype(bool)
    assert np.array_equal(_bits(res.lengths[ok]), _bits(lengths[ok]))
    assert np.isnan(res.lengths[~ok]).all()
    assert res.n_valid == int(ok.sum())


def _check_sizes(eng, sizes):
    for n in sizes:
        Ds, want, tie_free = _inputs(n)
        res = eng.nj(Ds)
        _same(res, want)
        assert (res.lengths[3] < 0).any() or n < 16   # the non-metric matrix
        _same(eng.nj(Ds[2]), want, rows=slice(2, 3))   # one replicate, as a 2-D matrix
        labels = list(range(n))
        for r in tie_free:
            assert no.split_sets(res.splits[r], labels) == treecheck.nj_splits(Ds[r], labels)


# ---------------------------------------------------------------------------
# rc_nj on host matrices
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", LDS_SIZES)
def test_lds_path(native, n):
    """One iteration (4), none (3), the wave boundary (63..65: one wave, then
    two) and the mask-word boundary (64, 65), up to the largest LDS size."""
    eng = _engine()
    try:
        _check_sizes(eng, [n])
        assert eng.timings()["nj_ms"] > 0
    finally:
        eng.close()


def test_workspace_path_by_default_above_128(native):
    eng = _engine()
    try:
        _check_sizes(eng, [129])
    finally:
        eng.close()


def test_workspace_path_by_knob(native, monkeypatch):
    """RC_NJ_LDS=0 on a fresh engine: every tree through the global workspace."""
    monkeypatch.setenv("RC_NJ_LDS", "0")
    eng = _engine()
    try:
        _check_sizes(eng, [4, 5, 64, 65])
    finally:
        eng.close()


def test_knob_is_a_threshold(native, monkeypatch):
    """RC_NJ_LDS=5: 5 samples in LDS, 8 in the workspace, on one engine."""
    monkeypatch.setenv("RC_NJ_LDS", "5")
    eng = _engine()
    try:
        _check_sizes(eng, [5, 8])
    finally:
        eng.close()


def test_more_replicates_than_workgroups_fit(native):
    """300 replicates of 8 samples: more workgroups than run at once."""
    rng = np.random.default_rng(300)
    base = nc.additive(8, seed=8)[0]
    Ds = np.stack([nc.jitter(base, seed=int(s)) for s in rng.integers(1 << 30, size=300)])
    want = no.nj_batch(Ds)
    assert len({tuple(no.split_ints(s)) for s in want[2]}) > 1   # the noise changes the topology
    eng = _engine()
    try:
        _same(eng.nj(Ds), want)
    finally:
        eng.close()


def _nan_third(n):
    Ds = np.array(_inputs(n)[0][[0, 3, 5, 6, 1]])
    Ds[2, 1, n - 1] = np.nan
    return Ds, no.nj_batch(Ds)


@pytest.mark.parametrize("n,knob", [(5, None), (65, None), (65, "0")])
def test_nan_replicate_is_flagged_and_the_rest_unaffected(native, monkeypatch, n, knob):
    from rna_clique_amd._native import RC_E_NO_IDEAL
    if knob is not None:
        monkeypatch.setenv("RC_NJ_LDS", knob)
    Ds, want = _nan_third(n)
    assert want[3].tolist() == [1, 1, 0, 1, 1]
    clean = _inputs(n)[1]
    for r, src in ((0, 0), (1, 3), (3, 6), (4, 1)):
        assert np.array_equal(want[0][r], clean[0][src]) and np.array_equal(_bits(want[1][r]), _bits(clean[1][src]))
    eng = _engine()
    try:
        assert _code(eng.nj, Ds) == RC_E_NO_IDEAL
        res = eng.nj(Ds, allow_nan=True)
        _same(res, want)
        assert (res.joins[2] == -1).all() and not res.splits[2].any() and res.n_valid == 4
        # an infinity above the diagonal too; NaN below it is not read
        Ds[2, 1, n - 1] = -np.inf
        Ds[0, n - 1, 1] = np.nan
        _same(eng.nj(Ds, allow_nan=True), want)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# support
# ---------------------------------------------------------------------------

def _absent_split(n, have):
    """A non-trivial split (without position 0) that no tree in `have` has."""
    for a, b in itertools.combinations(range(1, n), 2):
        m = 1 << a | 1 << b
        if m not in have:
            return m
    raise AssertionError("every cherry is present")


def _words(mask, n):
    return [(mask >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(no.words(n))]


@pytest.mark.parametrize("n,knob", [(8, None), (65, None), (130, None), (65, "0")])
def test_support_counts(native, monkeypatch, n, knob):
    """Reference splits from one replicate plus one that no replicate has;
    40 jittered replicates of one tree, the third with a NaN."""
    if knob is not None:
        monkeypatch.setenv("RC_NJ_LDS", knob)
    base = nc.additive(n, seed=n)[0]
    Ds = np.stack([nc.jitter(base, seed=1000 + r) for r in range(40)])
    Ds[2, 0, 1] = np.nan
    want = no.nj_batch(Ds)
    have = {m for r in range(40) for m in no.split_ints(want[2][r])}
    ref = np.concatenate([want[2][5], np.array([_words(_absent_split(n, have), n)], dtype=np.uint64)])
    counts, nv = no.support_counts(ref, want[2], want[3])
    assert nv == 39 and counts[-1] == 0 and counts[:-1].min() >= 1 and counts.max() <= 39
    assert 2 < len(set(counts.tolist()))   # the replicates disagree somewhere
    eng = _engine()
    try:
        res = eng.nj(Ds, ref, allow_nan=True)
        _same(res, want)
        assert res.support.dtype == np.uint32 and np.array_equal(res.support, counts) and res.n_valid == 39
        # no reference splits: n_valid alone
        res = eng.nj(Ds, np.zeros((0, no.words(n)), dtype=np.uint64), allow_nan=True)
        assert res.support.shape == (0,) and res.n_valid == 39
    finally:
        eng.close()


def test_every_null_output_combination(native):
    from rna_clique_amd._native import RC_E_NO_IDEAL
    n = 5
    Ds, want = _nan_third(n)
    ref = np.ascontiguousarray(want[2][0])
    counts, nv = no.support_counts(ref, want[2], want[3])
    vp = ctypes.c_void_p
    eng = _engine()
    try:
        for mask in range(64):
            joins = np.full((5, n - 2, 3), 7, dtype=np.int32)
            lengths = np.full((5, n - 2, 3), 7.0)
            splits = np.full((5, n - 3, 1), 7, dtype=np.uint64)
            valid = np.full(5, 7, dtype=np.uint8)
            support = np.full(len(ref), 7, dtype=np.uint32)
            nvalid = ctypes.c_uint32(7)
            arrs = [joins, lengths, splits, valid, support]
            ptr = [a.ctypes.data_as(vp) if mask >> i & 1 else None for i, a in enumerate(arrs)]
            code = native.rc_nj(eng._h, Ds.ctypes.data_as(vp), 5, n, ptr[0], ptr[1], ptr[2], ptr[3],
                                ref.ctypes.data_as(vp), len(ref), ptr[4], ctypes.byref(nvalid) if mask & 32 else None)
            assert code == RC_E_NO_IDEAL
            for i, (a, w) in enumerate(zip(arrs, [want[0], want[1], want[2], want[3], counts])):
                if mask >> i & 1:
                    assert np.array_equal(a, w, equal_nan=True)
                else:
                    assert (a == 7).all()
            assert nvalid.value == (nv if mask & 32 else 7)
    finally:
        eng.close()


def test_argument_errors(native):
    """Argument checks only: nothing here reaches a kernel."""
    from rna_clique_amd._native import RC_E_ARG, RC_E_LIMIT
    eng = _engine()
    try:
        D = np.array(_inputs(5)[0][:1])
        one = np.zeros((1, 1), dtype=np.uint64)
        assert _code(eng.nj, np.zeros((1, 2, 2))) == RC_E_ARG
        assert _code(eng.nj, np.zeros((0, 5, 5))) == RC_E_ARG
        for bad in (0b00111, 0b00001, 0b100010, 1 << 63):   # position 0, or bits at or above n = 5
            one[0, 0] = bad
            assert _code(eng.nj, D, one) == RC_E_ARG
        one[0, 0] = 0b10110
        assert eng.nj(D, one).support.tolist() in ([0], [1])
        vp = ctypes.c_void_p
        sup = np.zeros(1, dtype=np.uint32)
        assert native.rc_nj(eng._h, D.ctypes.data_as(vp), 1, 5, None, None, None, None, None, 0,
                            sup.ctypes.data_as(vp), None) == RC_E_ARG   # support without ref_splits
        assert native.rc_nj(eng._h, D.ctypes.data_as(vp), 1, 5, None, None, None, None, None, 1,
                            None, None) == RC_E_ARG
        assert native.rc_nj(eng._h, None, 1, 5, None, None, None, None, None, 0, None, None) == RC_E_ARG
        # the sample limit is checked before the matrix is touched
        assert native.rc_nj(eng._h, D.ctypes.data_as(vp), 1, 1025, None, None, None, None, None, 0, None,
                            None) == RC_E_LIMIT
        # a 65-sample split may use bit 0 of its second word, not bit 1
        D65 = np.array(_inputs(65)[0][:1])
        two = np.zeros((1, 2), dtype=np.uint64)
        two[0] = (0b110, 0b10)
        assert _code(eng.nj, D65, two) == RC_E_ARG
        two[0] = (0b110, 0b01)
        assert eng.nj(D65, two).support.shape == (1,)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# the engine path: rc_resample_trees on graph-only engines
# ---------------------------------------------------------------------------

def _graph_engine(case):
    """A graph-only engine over a GraphCase, as test_gpu_components builds it."""
    eng = _engine()
    for s, n in enumerate(case.genes):
        eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                       np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
    if case.sample_count:
        eng.set_sample_count(case.sample_count)
    eng.import_edges(case.records().view(np.uint8))
    return eng


def _check_trees(eng, W, order=None):
    """resample_trees(W) == the oracle on resample(W)'s matrices, with the
    support of the first replicate's splits."""
    labels, mats = eng.resample(W, order, allow_nan=True)
    want = no.nj_batch(mats)
    ref = np.ascontiguousarray(want[2][0])
    counts, nv = no.support_counts(ref, want[2], want[3])
    l2, res = eng.resample_trees(W, order, ref, allow_nan=True)
    assert l2 == labels
    _same(res, want)
    assert np.array_equal(res.support, counts) and res.n_valid == nv
    return res


@pytest.mark.parametrize("S", (4, 6, 8))
def test_resample_trees_on_graph_engines(native, S):
    """Clique cases of tests/post_cases.py over 4 and 6 samples and a synthetic
    one over 8 (40 ideal components): all ones, a delete-one jackknife and 50
    bootstrap rows, with and without order; an empty pair."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    from rna_clique_amd.similarity import SampleSimilarity, bootstrap_weights
    case = (pc.cliques_case(S) if S < 8 else pc.cliques_case(S, n_each=40, seed=3)).permuted(S)
    eng = _graph_engine(case)
    try:
        C = eng.n_components()
        assert C == (25 if S < 8 else 40)
        order = [int(x) for x in np.random.default_rng(S).permutation(S)[:max(3, S - 1)]]
        boot = bootstrap_weights(C, 50, seed=S)
        for W in (np.ones((1, C), dtype=np.uint16), 1 - np.eye(C, dtype=np.uint16), boot):
            _check_trees(eng, W)
            _check_trees(eng, W, order)
        assert eng.timings()["nj_ms"] > 0
        # a row that leaves every pair without rows
        W = np.array(boot[:5])
        W[2] = 0
        assert _code(eng.resample_trees, W) == RC_E_NO_IDEAL
        res = _check_trees(eng, W)
        assert res.valid.tolist() == [1, 1, 0, 1, 1] and (res.joins[2] == -1).all() and res.n_valid == 4
        # SampleSimilarity on the same engine
        sim = SampleSimilarity.from_engine(eng)
        tree = sim.neighbor_joining_tree()
        wj, wl, ws, wv = no.nj(sim.get_dissimilarity_matrix())
        assert wv == 1 and tree.labels == sim.samples and tree.support is None
        assert np.array_equal(tree.joins, wj) and np.array_equal(_bits(tree.lengths), _bits(wl))
        assert np.array_equal(tree.splits, ws)
        assert set(tree.splits_as_sets()) == treecheck.nj_splits(sim.get_dissimilarity_matrix(), sim.samples)
        reps = sim.resampled_trees(boot)
        assert len(reps) == 50
        sup = sim.bootstrap_support(50, seed=S)
        assert np.array_equal(sup.splits, ws) and np.array_equal(sup.joins, wj)
        masks = tree.split_masks()
        count = [sum(m in set(t.split_masks()) for t in reps) for m in masks]
        assert sup.support.tolist() == [c / 50 for c in count]
        assert sup.newick().endswith(";") and sup.newick() != tree.newick()
    finally:
        eng.close()


def test_three_samples_and_fewer(native):
    """Exactly 3 samples: the star tree with empty support; 2: ValueError."""
    from rna_clique_amd.similarity import SampleSimilarity
    eng = _graph_engine(pc.cliques_case(3).pair_major())
    try:
        sim = SampleSimilarity.from_engine(eng)
        sup = sim.bootstrap_support(10, seed=1)
        wj, wl, ws, _ = no.nj(sim.get_dissimilarity_matrix())
        assert sup.joins.tolist() == [[0, 1, 2]] == wj.tolist() and np.array_equal(_bits(sup.lengths), _bits(wl))
        assert sup.splits.shape == (0, 1) and sup.support.shape == (0,) and sup.splits_as_sets() == []
        assert sup.newick().count(",") == 2
    finally:
        eng.close()
    eng = _graph_engine(pc.star_case(n=50))
    try:
        sim = SampleSimilarity.from_engine(eng)
        for fn in (sim.neighbor_joining_tree, lambda: sim.bootstrap_support(5), lambda: sim.resampled_trees([[1]])):
            with pytest.raises(ValueError):
                fn()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# science level: the reference's verify_distances check
# ---------------------------------------------------------------------------

def test_gpu_tree_of_a_simulated_run_is_the_simulated_tree(native):
    """8 samples x 1000 genes (the reference's install-test shape), aligned by
    the engine: the GPU tree has Robinson-Foulds distance 0 to the simulated
    tree (tests/verify_install/verify_distances.py:39-55)."""
    from rna_clique_amd.similarity import SampleSimilarity
    from rna_clique_amd.simulate import simulate
    samples, (parent, _, leaves) = simulate(taxa=8, genes=1000, seed=487)
    eng = _engine()
    try:
        for s in samples:
            eng.add_sample(s.name, s.seq, s.tx_offsets, s.gene, s.iso)
        eng.run()
        tree = SampleSimilarity.from_engine(eng).neighbor_joining_tree()
        truth = treecheck.tree_splits(parent, leaves, {leaf: samples[i].name for i, leaf in enumerate(leaves)})
        assert len(truth) == 5
        assert treecheck.robinson_foulds(set(tree.splits_as_sets()), truth) == 0
    finally:
        eng.close()
