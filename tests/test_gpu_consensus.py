"""The census of replicate trees' splits and their Robinson-Foulds distances
on the GPU (splits.hip: rc_split_census, rc_tree_rf) against
tests/consensus_oracle.py run on nj_oracle's trees of the same matrices.
Splits, counts, ids, n_valid and both distance arrays are compared exactly;
consensus trees as split sets plus support and length bits."""
import ctypes
import functools

import numpy as np
import pytest

import consensus_oracle as co
import nj_cases as nc
import nj_oracle as no
import post_cases as pc

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle(Ds):
    """nj_oracle's trees of Ds and the oracle's census and distances of them
    (read-only: the tests share them)."""
    Ds = np.ascontiguousarray(Ds, dtype=np.float64)
    trees = no.nj_batch(Ds)
    masks, counts, ids, nv = co.census(trees[2], trees[3])
    n = Ds.shape[1]
    out = {"Ds": Ds, "trees": trees, "masks": masks, "splits": co.census_words(masks, n), "counts": counts,
           "ids": ids, "n_valid": nv, "pairwise": co.rf_pairwise(trees[2], trees[3])}
    for a in (Ds, out["splits"], counts, ids, out["pairwise"]) + trees:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _jittered(n, R):
    D = nc.additive(n, seed=n)[0]
    return _oracle(np.stack([nc.jitter(D, seed=100 * n + r, rel=0.3) for r in range(R)]))


def _absent_split(n, have):
    """A cherry without position 0 that no tree has."""
    for a in range(1, n):
        for b in range(a + 1, n):
            if (1 << a | 1 << b) not in have:
                return 1 << a | 1 << b
    raise AssertionError("every cherry is present")


def _same_census(census, want):
    assert census.splits.dtype == np.uint64 and census.counts.dtype == np.uint32 and census.ids.dtype == np.int32
    assert census.n_valid == want["n_valid"]
    assert census.splits.shape == want["splits"].shape and np.array_equal(census.splits, want["splits"])
    assert np.array_equal(census.counts, want["counts"])
    assert census.ids.shape == want["ids"].shape and np.array_equal(census.ids, want["ids"])


def _same_rf(eng, want, ref):
    """tree_rf against the oracle: to `ref` (n_ref, W) and pairwise, in one
    call and in one call each."""
    trees = want["trees"]
    to_ref = co.rf_to_ref(ref, trees[2], trees[3])
    got = eng.tree_rf(ref, pairwise=True)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], to_ref) and np.array_equal(got[1], want["pairwise"])
    only_ref, none = eng.tree_rf(ref)
    assert none is None and np.array_equal(only_ref, to_ref)
    none, only_pw = eng.tree_rf(pairwise=True)
    assert none is None and np.array_equal(only_pw, want["pairwise"])
    return to_ref


def _check(eng, want, allow_nan=False):
    """nj on want's matrices, then the census and the distances."""
    n = want["Ds"].shape[1]
    res = eng.nj(want["Ds"], allow_nan=allow_nan)
    assert np.array_equal(res.splits, want["trees"][2]) and np.array_equal(res.valid, want["trees"][3])
    census = eng.split_census()
    _same_census(census, want)
    first = int(np.flatnonzero(want["trees"][3])[0]) if want["n_valid"] else 0
    ref = np.array(want["trees"][2][first])
    if n > 4:
        ref = np.concatenate([ref, np.array([co.words(_absent_split(n, set(want["masks"])), n)], dtype=np.uint64)])
    _same_rf(eng, want, ref)
    return res, census


# ---------------------------------------------------------------------------
# jittered replicates of one tree
# ---------------------------------------------------------------------------

# (n, R): distinct splits, majority splits, splits of a single replicate, as the CPU oracle gives them
JITTERED = {(5, 7): (4, 2, 1), (8, 64): (9, 5, 0), (33, 64): (66, 28, 7), (65, 64): (208, 52, 65),
            (129, 24): (339, 104, 93)}


@pytest.mark.parametrize("n,R", list(JITTERED) + [(63, 16), (64, 16), (128, 16)])
def test_jittered_replicates(native, n, R):
    """One to three mask words (129: the global-workspace NJ path too), the
    word-boundary sizes; for n >= 33 more distinct splits than a tree holds, a
    multifurcating majority tree that greedy extends, and singletons."""
    from rna_clique_amd.tree import consensus_tree
    want = _jittered(n, R)
    masks, counts, nv = want["masks"], want["counts"], want["n_valid"]
    major = co.consensus_splits(masks, counts, nv, n, "majority")
    greedy = co.consensus_splits(masks, counts, nv, n, "greedy")
    if (n, R) in JITTERED:
        assert (len(masks), len(major), int((counts == 1).sum())) == JITTERED[n, R]
    if n >= 33:
        assert len(masks) > n - 3 and len(major) < n - 3 and len(greedy) > len(major) and (counts == 1).any()
    eng = _engine()
    try:
        res, census = _check(eng, want)
        assert eng.timings()["split_ms"] > 0
        labels = [f"s{b}" for b in range(n)]
        for method, chosen in (("majority", major), ("greedy", greedy)):
            tree = consensus_tree(census, labels, res.lengths, res.joins, method)
            assert tree.split_masks() == [masks[k] for k in chosen]
            assert tree.support.tolist() == [int(counts[k]) / nv for k in chosen]
            mean, leaf = co.mean_lengths(want["ids"], want["trees"][0], want["trees"][1], want["trees"][3], chosen, n)
            assert np.array_equal(_bits(tree.lengths), _bits(mean))
            assert np.array_equal(_bits(tree.leaf_lengths), _bits(leaf))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# many classes, one class per join, the smallest trees
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random65():
    return _oracle(np.stack([nc.random_symmetric(65, seed) for seed in range(48)]))


def test_almost_all_distinct_splits(native):
    """48 unrelated matrices of 65 samples: nearly every instance is a class
    of its own, which loads the table."""
    want = _random65()
    assert len(want["masks"]) > 0.8 * 48 * 62
    eng = _engine()
    try:
        _check(eng, want)
    finally:
        eng.close()


@pytest.mark.parametrize("n", (4, 64, 65))
def test_copies_of_one_tree(native, n):
    want = _oracle(np.stack([nc.all_equal(n)] * 16))
    assert len(want["masks"]) == n - 3 and want["counts"].tolist() == [16] * (n - 3)
    eng = _engine()
    try:
        _, census = _check(eng, want)
        assert census.ids.tolist() == [list(range(n - 3))] * 16
        assert not eng.tree_rf(want["trees"][2][0], pairwise=True)[1].any()
    finally:
        eng.close()


def test_three_and_four_samples(native):
    eng = _engine()
    try:
        want = _oracle(np.stack([nc.random_symmetric(3, seed) for seed in range(5)]))
        eng.nj(want["Ds"])
        census = eng.split_census()
        _same_census(census, want)
        assert census.splits.shape == (0, 1) and census.ids.shape == (5, 0) and census.n_valid == 5
        to_ref, pw = eng.tree_rf(np.zeros((0, 1), dtype=np.uint64), pairwise=True)
        assert to_ref.tolist() == [0] * 5 and pw.shape == (5, 5) and not pw.any()
        want = _oracle(np.stack([nc.random_symmetric(4, seed) for seed in range(40)]))
        assert 2 <= len(want["masks"]) <= 3
        _, census = _check(eng, want)
        assert len(census.counts) == len(want["masks"]) and int(census.counts.sum()) == 40
    finally:
        eng.close()


@pytest.mark.parametrize("n", (5, 65, 130))
def test_one_replicate(native, n):
    want = _oracle(nc.noisy_additive(n, seed=n)[0][None])
    eng = _engine()
    try:
        _, census = _check(eng, want)
        assert census.ids.tolist() == [list(range(n - 3))] and census.counts.tolist() == [1] * (n - 3)
        to_ref, pw = eng.tree_rf(want["trees"][2][0], pairwise=True)
        assert to_ref.tolist() == [0] and pw.tolist() == [[0]]
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# invalid replicates
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", (8, 65))
def test_invalid_replicates(native, n):
    """NaN matrices first, in the middle and last of 9: their ids are -1,
    their distances 0xFFFFFFFF in rows and columns, and the numbering starts
    at the first valid instance."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    Ds = np.array(_jittered(n, 64)["Ds"][:9])
    for r in (0, 4, 8):
        Ds[r, 0, 1] = np.nan
    want = _oracle(Ds)
    assert want["n_valid"] == 6 and want["trees"][3].tolist() == [0, 1, 1, 1, 0, 1, 1, 1, 0]
    assert want["ids"][1].tolist() == list(range(n - 3)) and (want["ids"][[0, 4, 8]] == -1).all()
    eng = _engine()
    try:
        assert _code(eng.nj, Ds) == RC_E_NO_IDEAL
        _, census = _check(eng, want, allow_nan=True)
        assert census.n_valid == 6 and (census.ids[[0, 4, 8]] == -1).all()
        to_ref, pw = eng.tree_rf(want["trees"][2][1], pairwise=True)
        bad = np.zeros(9, dtype=bool)
        bad[[0, 4, 8]] = True
        assert (to_ref[bad] == INVALID).all() and (to_ref[~bad] != INVALID).all() and to_ref[1] == 0
        assert (pw[bad] == INVALID).all() and (pw[:, bad] == INVALID).all()
        assert (pw[np.ix_(~bad, ~bad)] != INVALID).all() and not pw[~bad, ~bad].any()
        # every replicate invalid: an empty census
        eng.nj(np.full((3, n, n), np.nan), allow_nan=True)
        census = eng.split_census()
        assert census.splits.shape == (0, no.words(n)) and census.n_valid == 0 and (census.ids == -1).all()
        to_ref, pw = eng.tree_rf(want["trees"][2][1], pairwise=True)
        assert (to_ref == INVALID).all() and (pw == INVALID).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# determinism, state, error codes
# ---------------------------------------------------------------------------

def test_two_calls_give_identical_bytes_and_trees_stay(native):
    want = _jittered(33, 64)
    eng = _engine()
    try:
        before = eng.nj(want["Ds"], want["trees"][2][0])
        a = eng.split_census()
        rf_a = eng.tree_rf(want["trees"][2][0], pairwise=True)
        # the same trees built again: a new table, filled in another order
        after = eng.nj(want["Ds"], want["trees"][2][0])
        b = eng.split_census()
        rf_b = eng.tree_rf(want["trees"][2][0], pairwise=True)
        c = eng.split_census()
        for x, y in zip(a[:3] + rf_a, b[:3] + rf_b):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(b[:3], c[:3]):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(before[:5], after[:5]):
            assert x.tobytes() == y.tobytes()
        assert before.n_valid == after.n_valid == a.n_valid == 64
    finally:
        eng.close()


def test_census_follows_the_last_trees(native):
    first, second = _jittered(33, 64), _jittered(8, 64)
    eng = _engine()
    try:
        eng.nj(first["Ds"])
        _same_census(eng.split_census(), first)
        eng.nj(second["Ds"])
        _same_census(eng.split_census(), second)
        assert np.array_equal(eng.tree_rf(pairwise=True)[1], second["pairwise"])
        # a call that fails its argument checks leaves trees and census alone
        assert _code(eng.nj, np.zeros((1, 2, 2))) != 0
        _same_census(eng.split_census(), second)
    finally:
        eng.close()


def test_state_and_argument_errors(native):
    from rna_clique_amd._native import RC_E_ARG, RC_E_CAPACITY, RC_E_LIMIT, RC_E_STATE, RC_OK
    vp = ctypes.c_void_p
    want = _jittered(8, 64)
    K = len(want["masks"])
    eng = _engine()
    try:
        k, nv = ctypes.c_uint64(7), ctypes.c_uint32(7)
        assert native.rc_split_census(eng._h, None, None, None, 0, ctypes.byref(k), ctypes.byref(nv)) == RC_E_STATE
        assert native.rc_tree_rf(eng._h, None, 0, None, None) == RC_E_STATE
        assert _code(eng.split_census) == RC_E_STATE and _code(eng.tree_rf, pairwise=True) == RC_E_STATE
        eng.nj(want["Ds"])
        splits = np.zeros((K, 1), dtype=np.uint64)
        counts = np.zeros(K, dtype=np.uint32)
        sp, cp = splits.ctypes.data_as(vp), counts.ctypes.data_as(vp)
        assert native.rc_split_census(eng._h, None, None, None, 0, None, None) == RC_E_ARG
        assert native.rc_split_census(eng._h, None, None, None, 0, ctypes.byref(k), None) == RC_OK and k.value == K
        assert native.rc_split_census(eng._h, sp, None, None, K, ctypes.byref(k), None) == RC_E_ARG
        assert native.rc_split_census(eng._h, None, cp, None, K, ctypes.byref(k), None) == RC_E_ARG
        k.value = 0
        assert native.rc_split_census(eng._h, sp, cp, None, K - 1, ctypes.byref(k), ctypes.byref(nv)) == RC_E_CAPACITY
        assert k.value == K and nv.value == 64 and not splits.any()
        assert native.rc_split_census(eng._h, sp, cp, None, K, ctypes.byref(k), None) == RC_OK
        assert np.array_equal(splits, want["splits"]) and np.array_equal(counts, want["counts"])
        # ids alone
        ids = np.zeros((64, 5), dtype=np.int32)
        assert native.rc_split_census(eng._h, None, None, ids.ctypes.data_as(vp), 0, ctypes.byref(k), None) == RC_OK
        assert np.array_equal(ids, want["ids"])
        # rc_tree_rf
        to_ref = np.zeros(64, dtype=np.uint32)
        tp = to_ref.ctypes.data_as(vp)
        one = np.zeros((1, 1), dtype=np.uint64)
        assert native.rc_tree_rf(eng._h, None, 0, tp, None) == RC_E_ARG        # to_ref without ref_splits
        assert native.rc_tree_rf(eng._h, None, 1, None, None) == RC_E_ARG
        assert native.rc_tree_rf(eng._h, one.ctypes.data_as(vp), -1, None, None) == RC_E_ARG
        for bad in (0b00111, 0b00001, 1 << 8, 1 << 63):   # position 0, or bits at or above n = 8
            one[0, 0] = bad
            assert native.rc_tree_rf(eng._h, one.ctypes.data_as(vp), 1, tp, None) == RC_E_ARG
        one[0, 0] = 0b10000110
        assert native.rc_tree_rf(eng._h, one.ctypes.data_as(vp), 1, tp, None) == RC_OK
        assert np.array_equal(to_ref, co.rf_to_ref(one, want["trees"][2], want["trees"][3]))
        assert native.rc_tree_rf(eng._h, None, 0, None, None) == RC_OK
        # 8193 replicates: a census, distances to a reference, no pairwise matrix
        many = np.stack([nc.random_symmetric(4, seed) for seed in range(3)] * 2731)
        assert len(many) == 8193
        res = eng.nj(many)
        assert _code(eng.tree_rf, pairwise=True) == RC_E_LIMIT
        census = eng.split_census()
        assert int(census.counts.sum()) == 8193 and census.ids.shape == (8193, 1)
        to_ref, _ = eng.tree_rf(res.splits[0])
        assert to_ref.tolist() == (2 * (res.splits[:, 0, 0] != res.splits[0, 0, 0])).tolist()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# through an engine run
# ---------------------------------------------------------------------------

def _graph_engine(case):
    """A graph-only engine over a GraphCase, as test_gpu_nj builds it."""
    eng = _engine()
    for s, n in enumerate(case.genes):
        eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                       np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
    if case.sample_count:
        eng.set_sample_count(case.sample_count)
    eng.import_edges(case.records().view(np.uint8))
    return eng


def test_bootstrap_census_consensus_and_distances(native):
    """8 samples, 40 ideal components, 200 bootstrap replicates."""
    from rna_clique_amd.similarity import SampleSimilarity, bootstrap_weights
    from rna_clique_amd.tree import NJTree, conflicts
    S, R, seed = 8, 200, 11
    eng = _graph_engine(pc.cliques_case(S, n_each=40, seed=3).permuted(S))
    try:
        sim = SampleSimilarity.from_engine(eng)
        sup = sim.bootstrap_support(R, seed)
        # the replicates, downloaded: what the oracle works on
        reps = sim.resampled_trees(bootstrap_weights(eng.n_components(), R, seed))
        joins = np.stack([t.joins for t in reps])
        lengths = np.stack([t.lengths for t in reps])
        splits = np.stack([t.splits for t in reps])
        valid = np.ones(R, dtype=np.uint8)
        masks, counts, ids, nv = co.census(splits, valid)
        assert nv == R and len(masks) > S - 3   # the replicates disagree

        census = sim.bootstrap_split_census(R, seed)
        want = {"splits": co.census_words(masks, S), "counts": counts, "ids": ids, "n_valid": nv}
        _same_census(census, want)
        _same_census(sim.resampled_split_census(bootstrap_weights(eng.n_components(), R, seed)), want)
        assert eng.timings()["split_ms"] > 0
        # the counts of the reference tree's splits are bootstrap_support's
        number = {m: k for k, m in enumerate(masks)}
        mine = [int(census.counts[number[m]]) if m in number else 0 for m in sup.split_masks()]
        assert mine == np.rint(sup.support * nv).astype(int).tolist()
        assert [c / float(nv) for c in mine] == sup.support.tolist()

        for method in ("strict", "majority", "greedy"):
            chosen = co.consensus_splits(masks, counts, nv, S, method)
            tree = sim.bootstrap_consensus(R, seed, method)
            assert tree.labels == sim.samples and tree.split_masks() == [masks[k] for k in chosen]
            assert tree.support.tolist() == [int(counts[k]) / nv for k in chosen]
            mean, leaf = co.mean_lengths(ids, joins, lengths, valid, chosen, S)
            assert np.array_equal(_bits(tree.lengths), _bits(mean))
            assert np.array_equal(_bits(tree.leaf_lengths), _bits(leaf))
            assert tree.newick().endswith(";")

        to_ref, pw = sim.bootstrap_rf(R, seed, pairwise=True)
        assert np.array_equal(to_ref, co.rf_to_ref(sup.splits, splits, valid))
        assert np.array_equal(pw, co.rf_pairwise(splits, valid))
        assert sim.bootstrap_rf(R, seed)[1] is None

        ref = NJTree(sup.labels, sup.joins, sup.lengths, sup.splits)
        got = conflicts(census, ref)
        wantc = co.conflicts(masks, counts, nv, S, ref.split_masks())
        assert np.array_equal(got[0], wantc[0]) and np.array_equal(got[1], wantc[1])
    finally:
        eng.close()


def test_too_few_samples_and_no_components(native):
    from rna_clique_amd.similarity import SampleSimilarity
    eng = _graph_engine(pc.star_case(n=50))
    try:
        sim = SampleSimilarity.from_engine(eng)
        for fn in (lambda: sim.bootstrap_split_census(5), lambda: sim.bootstrap_consensus(5),
                   lambda: sim.bootstrap_rf(5)):
            with pytest.raises(ValueError):
                fn()
    finally:
        eng.close()
