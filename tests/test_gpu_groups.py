"""PERMANOVA and ANOSIM on the GPU (groups.hip: rc_group_test,
rc_resample_group_test) against tests/group_oracle.py. Everything is compared
exactly: statistics, totals, within-sums and the permutations' statistics as
bits, counts and validity as integers."""
import ctypes

import numpy as np
import pytest

import group_cases as gc
import group_oracle as go
import post_cases as pcases

pytestmark = pytest.mark.gpu

METHODS = ("permanova", "anosim")
CHUNK = gc.PERM_CHUNK   # 120 permutations per workgroup: 250 rows make three workgroups per matrix, the last partly full


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
    return (res.statistic, res.n_ge, res.total, res.within, res.perm_statistics, res.valid)


def _assert_same(got, want, what=""):
    """A GroupTestResult (with perm_stats) against the oracle's batch()."""
    names = ("statistic", "n_ge", "total", "within", "perm_statistics", "valid")
    for name, x, y in zip(names, _tuple(got), want):
        if np.asarray(y).dtype.kind == "f":
            assert np.array_equal(_bits(x), _bits(y)), (what, name, x, y)
        else:
            assert np.array_equal(x, y), (what, name, x, y)


def _res_same(a, b):
    return all((x is None and y is None) or
               (np.array_equal(_bits(x), _bits(y)) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y))
               for x, y in zip(_tuple(a), _tuple(b)))


# ---------------------------------------------------------------------------
# rc_group_test on host matrices
# ---------------------------------------------------------------------------

def test_chunk_size_is_the_kernel_s():
    from rna_clique_amd import groups
    assert groups.GPU_PERM_CHUNK == CHUNK and groups.MAX_GPU_SAMPLES == 128


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", gc.SIZES)
def test_every_size_grouping_and_permutation_count(native, n, method):
    """One row per lane up to 64 samples, two from 65, the LDS limit at 128;
    six valid matrices and an invalid one in a batch; 0, 1 and 199 permutations
    for every grouping, 250 (more than two workgroups' worth) for the first.
    Row 0 of the permutations is the identity: every count is at least 1."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    Ds = gc.matrices(n)
    Ds7 = np.concatenate([Ds, gc.with_nan(Ds, 0)[:1]])
    eng = _engine()
    try:
        for gi, (gname, labels) in enumerate(gc.groupings(n).items()):
            full = gc.perm_rows(labels, 250 if gi == 0 else 199, seed=n)
            assert len(full) < 2 * CHUNK or gi == 0
            want = go.batch(Ds7, labels, full, method)
            got = eng.group_test(Ds7, labels, full, method, perm_stats=True, allow_nan=True)
            assert eng.timings()["group_ms"] > 0
            _assert_same(got, want, (n, gname, len(full)))
            assert got.valid.tolist() == [1] * 6 + [0] and got.n_ge[6] == 0
            ok = ~np.isnan(got.statistic[:6])
            assert (got.n_ge[:6][ok] >= 1).all()
            assert _code(eng.group_test, Ds7, labels, full, method) == RC_E_NO_IDEAL
            # the valid matrices alone: the same bits, no error
            alone = eng.group_test(Ds, labels, full, method, perm_stats=True)
            _assert_same(alone, [x[:6] for x in want], (n, gname, "valid only"))
            for P in (0, 1):
                got = eng.group_test(Ds, labels, full[:P], method, perm_stats=True)
                _assert_same(got, go.batch(Ds, labels, full[:P], method), (n, gname, P))
                assert got.permutations == P and (got.p_value == (1.0 + got.n_ge) / (1 + P)).all()
            # the groups renumbered: the same partition, the same bits and counts
            m = gc.renumberings(labels, seed=n)[0]
            _assert_same(eng.group_test(Ds7, m[labels], m[full], method, perm_stats=True, allow_nan=True), want,
                         (n, gname, "renumbered"))
    finally:
        eng.close()


@pytest.mark.parametrize("method", METHODS)
def test_rows_of_the_observed_partition_have_the_observed_bits(native, method):
    """Equal groups that exchange their numbers are rearrangements a
    permutation test draws: each has the observed statistic's bits and counts."""
    eng = _engine()
    try:
        for n in (6, 8, 64, 66, 128):
            Ds = gc.matrices(n)
            for labels in (gc.groupings(n)["balanced"], gc.groupings(n)["pairs"]):
                rows = gc.same_partition_rows(labels, seed=n)
                res = eng.group_test(Ds, labels, rows, method, perm_stats=True)
                assert np.array_equal(_bits(res.perm_statistics), _bits(np.repeat(res.statistic[:, None], 4, axis=1)))
                ok = ~np.isnan(res.statistic)
                assert (res.n_ge[ok] == 4).all() and (res.n_ge[~ok] == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("method", METHODS)
def test_six_samples_in_two_groups_of_three(native, method):
    """Only 10 distinct partitions: the count is the number of rows whose
    partition, evaluated once by the oracle, reaches the observed statistic."""
    labels = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    perms = gc.perm_rows(labels, 300, seed=6)
    Ds = gc.matrices(6)
    eng = _engine()
    try:
        res = eng.group_test(Ds, labels, perms, method)
    finally:
        eng.close()
    want = [gc.six_sample_expected(D, labels, perms, method) for D in Ds]
    assert res.n_ge.tolist() == want
    assert np.array_equal(res.p_value, (1.0 + np.array(want)) / 301)


def test_degenerate_matrices(native):
    n, P = 9, 50
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, P)
    eng = _engine()
    try:
        res = eng.group_test(gc.nj_cases.all_equal(n), labels, perms, "anosim").first()
        assert res.statistic == 0.0 and res.n_ge == P and res.p_value == 1.0
        res = eng.group_test(np.zeros((n, n)), labels, perms, "permanova").first()
        assert np.isnan(res.statistic) and res.n_ge == 0 and res.valid == 1 and res.total == 0.0
    finally:
        eng.close()


def test_more_matrices_than_workgroups_fit(native):
    """600 matrices of 12 samples x 130 permutations: the same matrix at
    positions 0 and 599 gives the same bits, and so does a second call."""
    n = 12
    base = gc.matrices(n)
    rng = np.random.default_rng(12)
    Ds = np.stack([gc.nj_cases.jitter(go.mirrored(base[0]), int(s)) for s in rng.integers(1 << 30, size=600)])
    Ds[599] = Ds[0]
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, 130, seed=1)
    eng = _engine()
    try:
        for method in METHODS:
            a = eng.group_test(Ds, labels, perms, method, perm_stats=True)
            b = eng.group_test(Ds, labels, perms, method, perm_stats=True)
            assert _res_same(a, b) and a.valid.all()
            assert _bits(a.statistic)[0] == _bits(a.statistic)[599] and a.n_ge[0] == a.n_ge[599]
            assert len(set(a.n_ge.tolist())) > 1
            rows = [0, 299, 599]
            _assert_same(type(a).from_counts(method, n, 3, 130, a.statistic[rows], a.n_ge[rows], a.total[rows],
                                             a.within[rows], a.valid[rows], a.perm_statistics[rows]),
                         go.batch(Ds[rows], labels, perms, method))
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
        def call(dp, r, m, lab, a, pl, p, method=0):
            ptr = lambda x: None if x is None else x.ctypes.data_as(vp)   # noqa: E731
            return native.rc_group_test(eng._h, dp, r, m, ptr(lab), a, ptr(pl), p, method, None, None, None, None,
                                        None, None)
        dp = D.ctypes.data_as(vp)
        assert call(dp, 1, n, good, 3, perm, 1) == 0                       # every output NULL
        assert call(dp, 1, n, good, 3, None, 0) == 0                       # no permutations
        assert call(None, 1, n, good, 3, perm, 1) == RC_E_ARG              # NULL D
        assert call(dp, 1, n, None, 3, perm, 1) == RC_E_ARG                # NULL labels
        assert call(dp, 1, n, good, 3, None, 1) == RC_E_ARG                # NULL perm_labels with n_perm > 0
        assert call(dp, 0, n, good, 3, perm, 1) == RC_E_ARG                # n_rep < 1
        assert call(dp, 1, n, good, 3, perm, -1) == RC_E_ARG               # n_perm < 0
        assert call(dp, 1, n, good, 3, perm, 1, 2) == RC_E_ARG             # unknown method
        assert call(dp, 1, n, i32([0] * 6), 1, None, 0) == RC_E_ARG        # one group
        assert call(dp, 1, n, i32(range(6)), 6, None, 0) == RC_E_ARG       # singletons only
        assert call(dp, 1, n, i32([0, 0, 2, 2, 3, 3]), 4, None, 0) == RC_E_ARG   # group 1 is empty
        assert call(dp, 1, n, i32([0, 0, 1, 1, 3, 3]), 3, None, 0) == RC_E_ARG   # label out of range
        assert call(dp, 1, n, i32([0, 0, 1, 1, -1, 2]), 3, None, 0) == RC_E_ARG
        assert call(dp, 1, n, good, 3, i32([[0, 0, 0, 1, 2, 2]]), 1) == RC_E_ARG   # not a rearrangement
        assert call(dp, 1, n, good, 3, i32([[0, 0, 1, 1, 2, 3]]), 1) == RC_E_ARG
        # the sample limit is checked before anything is touched
        assert call(dp, 1, 129, good, 3, perm, 1) == RC_E_LIMIT
        assert call(None, 0, 129, None, 0, None, -1) == RC_E_LIMIT
        big = np.arange(129) % 2
        assert _code(eng.group_test, np.zeros((1, 129, 129)), big, None) == RC_E_LIMIT
        assert _code(eng.group_test, D, np.arange(n)) == RC_E_ARG
        assert _code(eng.group_test, D, good, [[0, 0, 0, 1, 2, 2]]) == RC_E_ARG
        with pytest.raises(ValueError):
            eng.group_test(D, good[:5])
        with pytest.raises(ValueError):
            eng.group_test(D, good, perm[:, :5])
        with pytest.raises(ValueError):
            eng.group_test(D, good, perm, "mantel")
    finally:
        eng.close()


@pytest.mark.parametrize("method", METHODS)
def test_every_null_output_combination(native, method):
    """A 2-D matrix is one replicate; any of the six outputs may be NULL."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    n, P = 5, 7
    Ds = gc.with_nan(gc.matrices(n)[:5])
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, P)
    vp = ctypes.c_void_p
    code = 0 if method == "permanova" else 1
    eng = _engine()
    try:
        one = eng.group_test(Ds[0], labels, perms, method, perm_stats=True)
        assert len(one) == 1
        _assert_same(one, go.batch(Ds[:1], labels, perms, method))
        want = eng.group_test(Ds, labels, perms, method, perm_stats=True, allow_nan=True)
        _assert_same(want, go.batch(Ds, labels, perms, method))
        wants = [want.statistic, want.n_ge, want.total, want.within, want.perm_statistics, want.valid]
        assert want.valid.tolist() == [1, 1, 0, 1, 1]
        for mask in range(64):
            arrs = [np.full(5, 7.0), np.full(5, 7, dtype=np.uint32), np.full(5, 7.0), np.full(5, 7.0),
                    np.full((5, P), 7.0), np.full(5, 7, dtype=np.uint8)]
            ptr = [a.ctypes.data_as(vp) if mask >> i & 1 else None for i, a in enumerate(arrs)]
            assert native.rc_group_test(eng._h, Ds.ctypes.data_as(vp), 5, n, labels.ctypes.data_as(vp),
                                        int(labels.max()) + 1, perms.ctypes.data_as(vp), P, code, *ptr) == RC_E_NO_IDEAL
            for i, (a, w) in enumerate(zip(arrs, wants)):
                if mask >> i & 1:
                    assert np.array_equal(a, w, equal_nan=True)
                else:
                    assert (a == 7).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# the engine path: rc_resample_group_test on graph-only engines
# ---------------------------------------------------------------------------

def _graph_engine(case):
    """A graph-only engine over a GraphCase, as test_gpu_pcoa builds it."""
    eng = _engine()
    for s, n in enumerate(case.genes):
        eng.add_sample(f"S{s}", np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                       np.arange(1, n + 1, dtype=np.int32), np.ones(n, np.int32))
    if case.sample_count:
        eng.set_sample_count(case.sample_count)
    eng.import_edges(case.records().view(np.uint8))
    return eng


def _check_resample(eng, W, labels, perms, method, order=None):
    """resample_group_test(W) == group_test(resample(W)) as bits, and both equal the oracle."""
    names, mats = eng.resample(W, order, allow_nan=True)
    want = eng.group_test(mats, labels, perms, method, perm_stats=True, allow_nan=True)
    n2, res = eng.resample_group_test(W, labels, perms, order, method, perm_stats=True, allow_nan=True)
    assert n2 == names and _res_same(res, want)
    _assert_same(res, go.batch(mats, labels, perms, method))
    return res


@pytest.mark.parametrize("S", (4, 6, 8))
def test_resample_group_test_on_graph_engines(native, S):
    """Clique cases of tests/post_cases.py over 4 and 6 samples and a synthetic
    one over 8 (40 ideal components): all ones, a delete-one jackknife and 50
    bootstrap rows, with and without a subset order; an empty row;
    SampleSimilarity."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    from rna_clique_amd.similarity import NoIdealComponentsError, SampleSimilarity, bootstrap_weights
    from rna_clique_amd import groups
    case = (pcases.cliques_case(S) if S < 8 else pcases.cliques_case(S, n_each=40, seed=3)).permuted(S)
    eng = _graph_engine(case)
    try:
        C = eng.n_components()
        assert C == (25 if S < 8 else 40)
        labels = gc.groupings(S)["balanced"]
        perms = gc.perm_rows(labels, 130, seed=S)
        sub = [int(x) for x in np.random.default_rng(S).permutation(S)[:max(3, S - 1)]]
        sub_labels = gc.groupings(len(sub))["balanced"]
        sub_perms = gc.perm_rows(sub_labels, 20, seed=S)
        boot = bootstrap_weights(C, 50, seed=S)
        for method in METHODS:
            for W in (np.ones((1, C), dtype=np.uint16), 1 - np.eye(C, dtype=np.uint16), boot):
                res = _check_resample(eng, W, labels, perms, method)
                assert res.valid.all()
                _check_resample(eng, W, sub_labels, sub_perms, method, sub)
            t = eng.timings()
            assert t["group_ms"] > 0 and t["resample_ms"] > 0
            # a row that leaves every pair without rows
            W = np.array(boot[:5])
            W[2] = 0
            assert _code(eng.resample_group_test, W, labels, perms, None, method) == RC_E_NO_IDEAL
            res = _check_resample(eng, W, labels, perms, method)
            assert res.valid.tolist() == [1, 1, 0, 1, 1] and np.isnan(res.statistic[2]) and res.n_ge[2] == 0
        # SampleSimilarity on the same engine
        sim = SampleSimilarity.from_engine(eng)
        D = sim.get_dissimilarity_matrix()
        grouping = {s: "ab"[i % 2] if i < S - 1 else "c" for i, s in enumerate(sim.samples)}
        if S == 4:
            grouping = {s: "ab"[i % 2] for i, s in enumerate(sim.samples)}
        lab, names = groups.encode_grouping(sim.samples, grouping)
        pl = groups.permuted_labels(lab, 99, seed=5)
        for method, fn in (("permanova", sim.permanova), ("anosim", sim.anosim)):
            got = fn(grouping, permutations=99, seed=5)
            stat, n_ge, total, within, _, valid = go.TESTS[method](D, lab, pl)
            assert _bits(got.statistic) == _bits(stat) and got.n_ge == n_ge and got.valid == valid == 1
            assert _bits(got.total) == _bits(total) and _bits(got.within) == _bits(within)
            assert got.p_value == (1 + n_ge) / 100 and got.permutations == 99
            assert (got.sample_size, got.n_groups) == (S, len(names))
            assert (got.r2 is None) == (method == "anosim")
            ref, reps = sim.bootstrap_group_test(grouping, 50, seed=S, method=method, permutations=99)
            assert _bits(ref.statistic) == _bits(go.TESTS[method](D, lab, groups.permuted_labels(lab, 99, seed=S))[0])
            mats = sim.resampled_dissimilarity_matrices(boot)
            _assert_same(sim.resampled_group_test(boot, grouping, method, 99, seed=S, perm_stats=True),
                         go.batch(mats, lab, groups.permuted_labels(lab, 99, seed=S), method))
            assert np.array_equal(_bits(reps.statistic), _bits(go.batch(mats, lab, pl[:0], method)[0]))
            assert len(reps) == 50 and reps.valid.all() and ((0 < reps.p_value) & (reps.p_value <= 1)).all()
            pairs = sim.pairwise_group_tests(grouping, method, permutations=30, seed=2)
            testable = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]
                        if sum(g in (a, b) for g in grouping.values()) >= 3]
            assert list(pairs) == testable and len(pairs) >= 1
            for (a, b), res in pairs.items():
                keep = [i for i, s in enumerate(sim.samples) if grouping[s] in (a, b)]
                l2, _ = groups.encode_grouping([sim.samples[i] for i in keep],
                                               [grouping[sim.samples[i]] for i in keep])
                want = go.TESTS[method](D[np.ix_(keep, keep)], l2, groups.permuted_labels(l2, 30, seed=2))
                assert _bits(res.statistic) == _bits(want[0]) and res.n_ge == want[1] and res.sample_size == len(keep)
            with pytest.raises(NoIdealComponentsError):
                sim.resampled_group_test(W, grouping, method)
    finally:
        eng.close()
