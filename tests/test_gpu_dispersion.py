"""PERMDISP on the GPU (dispersion.hip: rc_group_dispersion,
rc_resample_group_dispersion) against tests/dispersion_oracle.py. Everything is
compared exactly: F, SS_T, SS_W, the permutations' F and the distances to the
centroids as bits, counts and validity as integers."""
import ctypes

import numpy as np
import pytest

import dispersion_oracle as do
import group_cases as gc
import group_oracle as go
import post_cases as pcases

pytestmark = pytest.mark.gpu

SIZES = (3, 4, 5, 8, 63, 64, 65, 127, 128)   # one row per lane up to 64, two from 65; the last lane; the LDS limit
CHUNK = 124                                  # permutations per workgroup (dispersion.hip: DISP_PERM_CHUNK)
NAMES = ("statistic", "n_ge", "total", "within", "perm_statistics", "valid", "distances")


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


def _tuple(res):
    return tuple(getattr(res, name) for name in NAMES)


def _eq(x, y):
    return np.array_equal(_bits(x), _bits(y)) if np.asarray(y).dtype.kind == "f" else np.array_equal(x, y)


def _assert_same(got, want, what=""):
    """A DispersionResult (with perm_stats) against the oracle's batch()."""
    for name, x, y in zip(NAMES, _tuple(got), want):
        assert _eq(x, y), (what, name, x, y)


def _res_same(a, b):
    return all((x is None and y is None) or _eq(x, y) for x, y in zip(_tuple(a), _tuple(b)))


def _rows(want, rows):
    return [x[rows] for x in want]


# ---------------------------------------------------------------------------
# rc_group_dispersion on host matrices
# ---------------------------------------------------------------------------

def test_chunk_size_is_the_kernel_s(native):
    """One more permutation than a workgroup walks changes the grid limit's
    verdict: n_rep x ceil(n_perm / CHUNK) must stay below 2^31. The argument
    check comes before any device work, so nothing this large is allocated."""
    from rna_clique_amd import groups
    from rna_clique_amd._native import RC_E_LIMIT
    assert groups.GPU_DISP_PERM_CHUNK == CHUNK and groups.MAX_GPU_SAMPLES == 128
    vp = ctypes.c_void_p
    labels = np.array([0, 0, 1], dtype=np.int32)
    eng = _engine()
    try:
        def call(n_rep, n_perm):
            perms = np.tile(labels, (n_perm, 1))
            return native.rc_group_dispersion(eng._h, None, n_rep, 3, labels.ctypes.data_as(vp), 2,
                                              perms.ctypes.data_as(vp), n_perm, *[None] * 7)
        big = (1 << 31) // 2
        assert call(big, 2 * CHUNK + 1) == RC_E_LIMIT      # three chunks each
        assert call(big, 2 * CHUNK) == RC_E_LIMIT          # two chunks each: exactly 2^31
        assert call(big - 1, 2 * CHUNK) == -1              # below the limit: on to the NULL matrix (RC_E_ARG)
        assert call(2 * big - 1, CHUNK) == -1 and call(2 * big - 1, CHUNK + 1) == RC_E_LIMIT
    finally:
        eng.close()


@pytest.mark.parametrize("n", SIZES)
def test_every_size_grouping_and_permutation_count(native, n):
    """Six valid matrices and an invalid one in a batch; for every grouping
    CHUNK + 1 permutations (a second workgroup with a single row), their first
    0, 1, CHUNK - 1 and CHUNK, and for the first grouping 2 CHUNK + 1. Row 0 of
    the permutations is the identity: every count is at least 1."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    Ds = gc.matrices(n)
    Ds7 = np.concatenate([Ds, gc.with_nan(Ds, 0)[:1]])
    eng = _engine()
    try:
        for gi, (gname, labels) in enumerate(gc.groupings(n).items()):
            full = gc.perm_rows(labels, 2 * CHUNK + 1 if gi == 0 else CHUNK + 1, seed=n)
            want = do.batch(Ds7, labels, full)
            got = eng.group_dispersion(Ds7, labels, full, perm_stats=True, allow_nan=True)
            assert eng.timings()["disp_ms"] > 0
            _assert_same(got, want, (n, gname, len(full)))
            assert got.valid.tolist() == [1] * 6 + [0] and got.n_ge[6] == 0 and np.isnan(got.distances[6]).all()
            ok = ~np.isnan(got.statistic[:6])
            assert (got.n_ge[:6][ok] >= 1).all()
            assert _code(eng.group_dispersion, Ds7, labels, full) == RC_E_NO_IDEAL
            # the valid matrices alone: the same bits, no error
            alone = eng.group_dispersion(Ds, labels, full, perm_stats=True)
            _assert_same(alone, _rows(want, slice(0, 6)), (n, gname, "valid only"))
            for P in (0, 1, CHUNK - 1, CHUNK):
                got = eng.group_dispersion(Ds, labels, full[:P], perm_stats=True)
                w = _rows(want, slice(0, 6))
                w[4] = w[4][:, :P]
                w[1] = (w[4] >= w[0][:, None]).sum(axis=1).astype(np.uint32)
                _assert_same(got, w, (n, gname, P))
                assert got.permutations == P and (got.p_value == (1.0 + got.n_ge) / (1 + P)).all()
            # the groups renumbered: the same partition, the same bits and counts
            m = gc.renumberings(labels, seed=n)[0]
            _assert_same(eng.group_dispersion(Ds7, m[labels], m[full], perm_stats=True, allow_nan=True), want,
                         (n, gname, "renumbered"))
    finally:
        eng.close()


def test_a_negative_squared_distance(native):
    """The matrix of test_dispersion_host with an imaginary distance to the centroid."""
    D = go.mirrored(gc.matrices(6)[3])
    D[0, 1] = D[1, 0] = D[0, 2] = D[2, 0] = 1.0
    D[1, 2] = D[2, 1] = 10.0
    labels = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    assert do.centroid_distances(D, labels)[1][0] < 0
    perms = gc.perm_rows(labels, 30, seed=1)
    eng = _engine()
    try:
        _assert_same(eng.group_dispersion(D, labels, perms, perm_stats=True), do.batch(D[None], labels, perms))
    finally:
        eng.close()


def test_rows_of_the_observed_partition_have_the_observed_bits(native):
    eng = _engine()
    try:
        for n in (6, 8, 64, 66, 128):
            Ds = gc.matrices(n)
            for labels in (gc.groupings(n)["balanced"], gc.groupings(n)["pairs"]):
                rows = gc.same_partition_rows(labels, seed=n)
                res = eng.group_dispersion(Ds, labels, rows, perm_stats=True)
                assert np.array_equal(_bits(res.perm_statistics), _bits(np.repeat(res.statistic[:, None], 4, axis=1)))
                ok = ~np.isnan(res.statistic)
                assert (res.n_ge[ok] == 4).all() and (res.n_ge[~ok] == 0).all()
    finally:
        eng.close()


def test_six_samples_in_two_groups_of_three(native):
    """Only 10 distinct partitions: the count is the number of rows whose
    partition, evaluated once by the oracle, reaches the observed F."""
    labels = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    perms = gc.perm_rows(labels, 300, seed=6)
    Ds = gc.matrices(6)
    eng = _engine()
    try:
        res = eng.group_dispersion(Ds, labels, perms)
    finally:
        eng.close()
    want = [do.six_sample_expected(D, labels, perms) for D in Ds]
    assert res.n_ge.tolist() == want
    assert np.array_equal(res.p_value, (1.0 + np.array(want)) / 301)


def test_degenerate_matrices(native):
    n, P = 9, 50
    eng = _engine()
    try:
        for labels in gc.groupings(n).values():
            perms = gc.perm_rows(labels, P)
            Ds = np.stack([np.zeros((n, n)), gc.nj_cases.all_equal(n)])
            _assert_same(eng.group_dispersion(Ds, labels, perms, perm_stats=True), do.batch(Ds, labels, perms))
        res = eng.group_dispersion(np.zeros((n, n)), labels, perms).first()
        assert np.isnan(res.statistic) and res.n_ge == 0 and res.valid == 1 and res.total == 0.0
        assert (res.distances == 0).all()
    finally:
        eng.close()


def test_more_matrices_than_workgroups_fit(native):
    """3000 matrices of 8 samples x 130 permutations, two workgroups each, far
    more than the device holds at once: a matrix gives the same bits wherever
    it stands in the batch, in a batch in another order, and alone."""
    n, R = 8, 3000
    base = gc.matrices(n)
    rng = np.random.default_rng(8)
    Ds = np.stack([gc.nj_cases.jitter(go.mirrored(base[0]), int(s)) for s in rng.integers(1 << 30, size=R)])
    Ds[R - 1] = Ds[0]
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, 130, seed=1)
    eng = _engine()
    try:
        a = eng.group_dispersion(Ds, labels, perms, perm_stats=True)
        assert a.valid.all() and len(set(a.n_ge.tolist())) > 1
        assert _bits(a.statistic)[0] == _bits(a.statistic)[R - 1] and a.n_ge[0] == a.n_ge[R - 1]
        order = rng.permutation(R)
        b = eng.group_dispersion(Ds[order], labels, perms, perm_stats=True)
        for x, y in zip(_tuple(a), _tuple(b)):
            assert _eq(np.asarray(x)[order], y)
        rows = [0, 1499, R - 1]
        want = do.batch(Ds[rows], labels, perms)
        for r, k in enumerate(rows):
            alone = eng.group_dispersion(Ds[k], labels, perms, perm_stats=True)
            _assert_same(alone, _rows(want, slice(r, r + 1)))
            assert all(_eq(np.asarray(x)[k:k + 1], y) for x, y in zip(_tuple(a), _tuple(alone)))
    finally:
        eng.close()


def test_argument_errors(native):
    """Argument checks only: nothing here reaches a kernel."""
    from rna_clique_amd._native import RC_E_ARG, RC_E_LIMIT
    n = 6
    D = np.ascontiguousarray(gc.matrices(n)[:1])
    vp = ctypes.c_void_p
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)   # noqa: E731
    good, perm = i32([0, 0, 1, 1, 2, 2]), i32([[2, 0, 1, 0, 2, 1]])
    eng = _engine()
    try:
        def call(dp, r, m, lab, a, pl, p):
            ptr = lambda x: None if x is None else x.ctypes.data_as(vp)   # noqa: E731
            return native.rc_group_dispersion(eng._h, dp, r, m, ptr(lab), a, ptr(pl), p, *[None] * 7)
        dp = D.ctypes.data_as(vp)
        assert call(dp, 1, n, good, 3, perm, 1) == 0                       # every output NULL
        assert call(dp, 1, n, good, 3, None, 0) == 0                       # no permutations
        assert call(None, 1, n, good, 3, perm, 1) == RC_E_ARG              # NULL D
        assert call(dp, 1, n, None, 3, perm, 1) == RC_E_ARG                # NULL labels
        assert call(dp, 1, n, good, 3, None, 1) == RC_E_ARG                # NULL perm_labels with n_perm > 0
        assert call(dp, 0, n, good, 3, perm, 1) == RC_E_ARG                # n_rep < 1
        assert call(dp, 1, n, good, 3, perm, -1) == RC_E_ARG               # n_perm < 0
        assert call(dp, 1, n, i32([0] * 6), 1, None, 0) == RC_E_ARG        # one group
        assert call(dp, 1, n, i32(range(6)), 6, None, 0) == RC_E_ARG       # singletons only
        assert call(dp, 1, n, i32([0, 0, 2, 2, 3, 3]), 4, None, 0) == RC_E_ARG   # group 1 is empty
        assert call(dp, 1, n, i32([0, 0, 1, 1, 3, 3]), 3, None, 0) == RC_E_ARG   # label out of range
        assert call(dp, 1, n, i32([0, 0, 1, 1, -1, 2]), 3, None, 0) == RC_E_ARG
        assert call(dp, 1, n, good, 3, i32([[0, 0, 0, 1, 2, 2]]), 1) == RC_E_ARG   # not a rearrangement
        assert call(dp, 1, n, good, 3, i32([[0, 0, 1, 1, 2, 3]]), 1) == RC_E_ARG
        assert native.rc_group_dispersion(None, dp, 1, n, good.ctypes.data_as(vp), 3, None, 0, *[None] * 7) == RC_E_ARG
        # the sample limit is checked before anything is touched
        assert call(dp, 1, 129, good, 3, perm, 1) == RC_E_LIMIT
        assert call(None, 0, 129, None, 0, None, -1) == RC_E_LIMIT
        big = np.arange(129) % 2
        assert _code(eng.group_dispersion, np.zeros((1, 129, 129)), big, None) == RC_E_LIMIT
        assert _code(eng.group_dispersion, D, np.arange(n)) == RC_E_ARG
        assert _code(eng.group_dispersion, D, good, [[0, 0, 0, 1, 2, 2]]) == RC_E_ARG
        with pytest.raises(ValueError):
            eng.group_dispersion(D, good[:5])
        with pytest.raises(ValueError):
            eng.group_dispersion(D, good, perm[:, :5])
    finally:
        eng.close()


def test_every_null_output_combination(native):
    """A 2-D matrix is one replicate; any of the seven outputs may be NULL."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    n, P = 5, 7
    Ds = gc.with_nan(gc.matrices(n)[:5])
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, P)
    vp = ctypes.c_void_p
    eng = _engine()
    try:
        one = eng.group_dispersion(Ds[0], labels, perms, perm_stats=True)
        assert len(one) == 1
        _assert_same(one, do.batch(Ds[:1], labels, perms))
        want = eng.group_dispersion(Ds, labels, perms, perm_stats=True, allow_nan=True)
        _assert_same(want, do.batch(Ds, labels, perms))
        # in the ABI's order: stat, n_ge, total, within, perm_stat, dist, valid
        wants = [want.statistic, want.n_ge, want.total, want.within, want.perm_statistics, want.distances, want.valid]
        assert want.valid.tolist() == [1, 1, 0, 1, 1]
        for mask in range(128):
            arrs = [np.full(5, 7.0), np.full(5, 7, dtype=np.uint32), np.full(5, 7.0), np.full(5, 7.0),
                    np.full((5, P), 7.0), np.full((5, n), 7.0), np.full(5, 7, dtype=np.uint8)]
            ptr = [a.ctypes.data_as(vp) if mask >> i & 1 else None for i, a in enumerate(arrs)]
            assert native.rc_group_dispersion(eng._h, Ds.ctypes.data_as(vp), 5, n, labels.ctypes.data_as(vp),
                                              int(labels.max()) + 1, perms.ctypes.data_as(vp), P, *ptr) == RC_E_NO_IDEAL
            for i, (a, w) in enumerate(zip(arrs, wants)):
                if mask >> i & 1:
                    assert np.array_equal(a, w, equal_nan=True)
                else:
                    assert (a == 7).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# the engine path: rc_resample_group_dispersion on graph-only engines
# ---------------------------------------------------------------------------

def _graph_engine(case):
    """A graph-only engine over a GraphCase, as test_gpu_groups builds it."""
    eng = _engine()
    for s, n in enumerate(case.genes):
        eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                       np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
    if case.sample_count:
        eng.set_sample_count(case.sample_count)
    eng.import_edges(case.records().view(np.uint8))
    return eng


def _check_resample(eng, W, labels, perms, order=None):
    """resample_group_dispersion(W) == group_dispersion(resample(W)) as bits, and both equal the oracle."""
    names, mats = eng.resample(W, order, allow_nan=True)
    want = eng.group_dispersion(mats, labels, perms, perm_stats=True, allow_nan=True)
    n2, res = eng.resample_group_dispersion(W, labels, perms, order, perm_stats=True, allow_nan=True)
    assert n2 == names and _res_same(res, want)
    _assert_same(res, do.batch(mats, labels, perms))
    return res


@pytest.mark.parametrize("S", (4, 6, 8))
def test_resample_group_dispersion_on_graph_engines(native, S):
    """The engines of test_resample_group_test_on_graph_engines: all ones, a
    delete-one jackknife and 50 bootstrap rows, with and without a subset
    order; an empty row; SampleSimilarity."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    from rna_clique_amd.similarity import NoIdealComponentsError, SampleSimilarity, bootstrap_weights
    from rna_clique_amd import groups
    case = (pcases.cliques_case(S) if S < 8 else pcases.cliques_case(S, n_each=40, seed=3)).permuted(S)
    eng = _graph_engine(case)
    try:
        C = eng.n_components()
        labels = gc.groupings(S)["balanced"]
        perms = gc.perm_rows(labels, 130, seed=S)
        sub = [int(x) for x in np.random.default_rng(S).permutation(S)[:max(3, S - 1)]]
        sub_labels = gc.groupings(len(sub))["balanced"]
        sub_perms = gc.perm_rows(sub_labels, 20, seed=S)
        boot = bootstrap_weights(C, 50, seed=S)
        for W in (np.ones((1, C), dtype=np.uint16), 1 - np.eye(C, dtype=np.uint16), boot):
            res = _check_resample(eng, W, labels, perms)
            assert res.valid.all()
            _check_resample(eng, W, sub_labels, sub_perms, sub)
        t = eng.timings()
        assert t["disp_ms"] > 0 and t["resample_ms"] > 0
        # a row that leaves every pair without rows
        W = np.array(boot[:5])
        W[2] = 0
        assert _code(eng.resample_group_dispersion, W, labels, perms) == RC_E_NO_IDEAL
        res = _check_resample(eng, W, labels, perms)
        assert res.valid.tolist() == [1, 1, 0, 1, 1] and np.isnan(res.statistic[2]) and res.n_ge[2] == 0
        # SampleSimilarity on the same engine
        sim = SampleSimilarity.from_engine(eng)
        D = sim.get_dissimilarity_matrix()
        grouping = {s: "ab"[i % 2] if i < S - 1 else "c" for i, s in enumerate(sim.samples)}
        if S == 4:
            grouping = {s: "ab"[i % 2] for i, s in enumerate(sim.samples)}
        lab, names = groups.encode_grouping(sim.samples, grouping)
        pl = groups.permuted_labels(lab, 99, seed=5)
        got = sim.permdisp(grouping, permutations=99, seed=5)
        stat, n_ge, total, within, _, valid, z = do.permdisp(D, lab, pl)
        assert _bits(got.statistic) == _bits(stat) and got.n_ge == n_ge and got.valid == valid == 1
        assert _bits(got.total) == _bits(total) and _bits(got.within) == _bits(within)
        assert np.array_equal(_bits(got.distances), _bits(z)) and got.group_means.shape == (len(names),)
        assert got.p_value == (1 + n_ge) / 100 and got.permutations == 99
        assert (got.sample_size, got.n_groups) == (S, len(names))
        ref, reps = sim.bootstrap_permdisp(grouping, 50, seed=S, permutations=99)
        assert _bits(ref.statistic) == _bits(do.permdisp(D, lab, groups.permuted_labels(lab, 99, seed=S))[0])
        mats = sim.resampled_dissimilarity_matrices(boot)
        _assert_same(sim.resampled_permdisp(boot, grouping, 99, seed=S, perm_stats=True),
                     do.batch(mats, lab, groups.permuted_labels(lab, 99, seed=S)))
        assert np.array_equal(_bits(reps.statistic), _bits(do.batch(mats, lab, pl[:0])[0]))
        assert len(reps) == 50 and reps.valid.all()
        pairs = sim.pairwise_permdisp(grouping, permutations=30, seed=2)
        testable = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]
                    if sum(g in (a, b) for g in grouping.values()) >= 3]
        assert list(pairs) == testable and len(pairs) >= 1
        for (a, b), res in pairs.items():
            keep = [i for i, s in enumerate(sim.samples) if grouping[s] in (a, b)]
            l2, _ = groups.encode_grouping([sim.samples[i] for i in keep], [grouping[sim.samples[i]] for i in keep])
            want = do.permdisp(D[np.ix_(keep, keep)], l2, groups.permuted_labels(l2, 30, seed=2))
            assert _bits(res.statistic) == _bits(want[0]) and res.n_ge == want[1] and res.sample_size == len(keep)
        with pytest.raises(NoIdealComponentsError):
            sim.resampled_permdisp(W, grouping)
    finally:
        eng.close()
