"""The Mantel test on the GPU (mantel.hip: rc_mantel, rc_resample_mantel)
against tests/mantel_oracle.py. Everything is compared exactly: r and the
permutations' r as bits, the three counts and validity as integers."""
import ctypes

import numpy as np
import pytest

import group_cases as gc
import group_oracle as go
import mantel_oracle as mo
import nj_cases
import post_cases as pcases

pytestmark = pytest.mark.gpu

SIZES = (3, 4, 5, 8, 63, 64, 65, 127, 128)   # one row per lane up to 64, two from 65; the last lane; the LDS limit
CHUNK = 124                                  # permutations per workgroup (mantel.hip: MANTEL_PERM_CHUNK)
NAMES = ("statistic", "n_ge", "n_le", "n_abs_ge", "perm_statistics", "valid")


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
    """A MantelResult (with perm_stats) against the oracle's batch()."""
    for name, x, y in zip(NAMES, _tuple(got), want):
        assert _eq(x, y), (what, name, x, y)


def _res_same(a, b):
    return all((x is None and y is None) or _eq(x, y) for x, y in zip(_tuple(a), _tuple(b)))


def _other(n, method):
    """Y: a noisy additive matrix of another tree (pearson), one with tied integer distances (spearman)."""
    if method == "spearman":
        return go.mirrored(nj_cases.additive(n, 700 + n, integer=True)[0])
    return go.mirrored(nj_cases.noisy_additive(n, 500 + n)[0])


def _cut(want, P, method):
    """The oracle's batch() for the first P permutations, from the one for all of them."""
    stat, _, _, _, ps, valid = want
    ps = ps[:, :P]
    with np.errstate(invalid="ignore"):
        counts = [(ps >= stat[:, None]).sum(axis=1), (ps <= stat[:, None]).sum(axis=1),
                  (np.abs(ps) >= np.abs(stat)[:, None]).sum(axis=1)]
    return stat, *(c.astype(np.uint32) for c in counts), ps, valid


# ---------------------------------------------------------------------------
# rc_mantel on host matrices
# ---------------------------------------------------------------------------

def test_chunk_size_is_the_kernel_s(native):
    """As test_gpu_dispersion's: the grid limit n_rep x ceil(n_perm / CHUNK) <
    2^31 turns on one permutation more than a workgroup walks; the check comes
    before any device work."""
    from rna_clique_amd import mantel
    from rna_clique_amd._native import RC_E_ARG, RC_E_LIMIT
    assert mantel.GPU_PERM_CHUNK == CHUNK and mantel.MAX_GPU_SAMPLES == 128
    vp = ctypes.c_void_p
    Y = np.ascontiguousarray(_other(3, "pearson"))
    eng = _engine()
    try:
        def call(n_rep, n_perm):
            perms = np.tile(np.arange(3, dtype=np.int32), (n_perm, 1))
            return native.rc_mantel(eng._h, None, n_rep, 3, Y.ctypes.data_as(vp), perms.ctypes.data_as(vp), n_perm, 0,
                                    *[None] * 6)
        big = 1 << 30
        assert call(big, 2 * CHUNK + 1) == RC_E_LIMIT and call(big, 2 * CHUNK) == RC_E_LIMIT
        assert call(big - 1, 2 * CHUNK) == RC_E_ARG        # below the limit: on to the NULL matrix
        assert call(2 * big - 1, CHUNK) == RC_E_ARG and call(2 * big - 1, CHUNK + 1) == RC_E_LIMIT
    finally:
        eng.close()


@pytest.mark.parametrize("method", mo.METHODS)
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_permutation_count(native, n, method):
    """Six valid matrices (one of them constant) and an invalid one in a batch
    against one Y; 2 CHUNK + 1 permutations (a third workgroup with a single
    row) and their first 0, 1, CHUNK - 1, CHUNK and CHUNK + 1. Row 0 of the
    permutations is the identity: it has the observed bits and every count of
    a matrix with a correlation is at least 1."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    Xs = gc.matrices(n)
    Xs7 = np.concatenate([Xs, gc.with_nan(Xs, 0)[:1]])
    Y = _other(n, method)
    full = mo.perm_rows(n, 2 * CHUNK + 1, seed=n)
    want = mo.batch(Xs7, Y, full, method)
    eng = _engine()
    try:
        got = eng.mantel(Xs7, Y, full, method, perm_stats=True, allow_nan=True)
        assert eng.timings()["mantel_ms"] > 0
        _assert_same(got, want, (n, len(full)))
        assert got.valid.tolist() == [1] * 6 + [0] and got.n_ge[6] == got.n_le[6] == got.n_abs_ge[6] == 0
        assert np.isnan(got.statistic[[2, 6]]).all() and got.n_ge[2] == got.n_le[2] == got.n_abs_ge[2] == 0   # "equal"
        ok = [0, 1, 3, 4, 5]
        assert np.array_equal(_bits(got.perm_statistics[ok, 0]), _bits(got.statistic[ok]))
        assert (got.n_ge[ok] >= 1).all() and (got.n_le[ok] >= 1).all() and (got.n_abs_ge[ok] >= 1).all()
        assert _code(eng.mantel, Xs7, Y, full, method) == RC_E_NO_IDEAL
        # the valid matrices alone: the same bits, no error
        alone = eng.mantel(Xs, Y, full, method, perm_stats=True)
        _assert_same(alone, [x[:6] for x in want], (n, "valid only"))
        if method == "pearson":
            for P in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1):
                _assert_same(eng.mantel(Xs7, Y, full[:P], method, perm_stats=True, allow_nan=True),
                             _cut(want, P, method), (n, P))
        else:   # the counts compare integers: from the oracle itself
            for P in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1):
                _assert_same(eng.mantel(Xs, Y, full[:P], method, perm_stats=True),
                             mo.batch(Xs, Y, full[:P], method), (n, P))
        # a constant Y; a matrix against itself
        flat = eng.mantel(Xs, nj_cases.all_equal(n, 0.5), full[:5], method, perm_stats=True)
        assert np.isnan(flat.statistic).all() and np.isnan(flat.perm_statistics).all() and flat.valid.all()
        assert not flat.n_ge.any() and not flat.n_le.any() and not flat.n_abs_ge.any()
        assert eng.mantel(Xs[0], Xs[0], None, method).statistic[0] == 1.0
    finally:
        eng.close()


@pytest.mark.parametrize("method", mo.METHODS)
def test_more_matrices_than_workgroups_fit(native, method):
    """3000 matrices of 8 samples x 130 permutations, two workgroups each, far
    more than the device holds at once: a matrix gives the same bits wherever
    it stands in the batch, in a batch in another order, and alone."""
    n, R = 8, 3000
    base = gc.matrices(n)
    rng = np.random.default_rng(8)
    Xs = np.stack([nj_cases.jitter(go.mirrored(base[0]), int(s)) for s in rng.integers(1 << 30, size=R)])
    Xs[R - 1] = Xs[0]
    Y = _other(n, method)
    perms = mo.perm_rows(n, 130, seed=1)
    eng = _engine()
    try:
        a = eng.mantel(Xs, Y, perms, method, perm_stats=True)
        assert a.valid.all() and len(set(a.n_ge.tolist())) > 1
        assert _bits(a.statistic)[0] == _bits(a.statistic)[R - 1] and a.n_abs_ge[0] == a.n_abs_ge[R - 1]
        order = rng.permutation(R)
        b = eng.mantel(Xs[order], Y, perms, method, perm_stats=True)
        for x, y in zip(_tuple(a), _tuple(b)):
            assert _eq(np.asarray(x)[order], y)
        rows = [0, 1499, R - 1]
        want = mo.batch(Xs[rows], Y, perms, method)
        for r, k in enumerate(rows):
            alone = eng.mantel(Xs[k], Y, perms, method, perm_stats=True)
            _assert_same(alone, [x[r:r + 1] for x in want])
            assert all(_eq(np.asarray(x)[k:k + 1], y) for x, y in zip(_tuple(a), _tuple(alone)))
    finally:
        eng.close()


def test_argument_errors(native):
    """Argument checks only: nothing here reaches a kernel."""
    from rna_clique_amd._native import RC_E_ARG, RC_E_LIMIT
    n = 6
    X = np.ascontiguousarray(gc.matrices(n)[:1])
    Y = np.ascontiguousarray(_other(n, "pearson"))
    vp = ctypes.c_void_p
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)   # noqa: E731
    perm = i32([[2, 0, 1, 5, 4, 3]])
    eng = _engine()
    try:
        def call(xp, r, m, y, pl, p, method=0):
            ptr = lambda x: None if x is None else x.ctypes.data_as(vp)   # noqa: E731
            return native.rc_mantel(eng._h, xp, r, m, ptr(y), ptr(pl), p, method, *[None] * 6)
        xp = X.ctypes.data_as(vp)
        assert call(xp, 1, n, Y, perm, 1) == 0 and call(xp, 1, n, Y, perm, 1, 1) == 0   # every output NULL
        assert call(xp, 1, n, Y, None, 0) == 0                       # no permutations
        assert call(None, 1, n, Y, perm, 1) == RC_E_ARG              # NULL X
        assert call(xp, 1, n, None, perm, 1) == RC_E_ARG             # NULL Y
        assert call(xp, 1, n, Y, None, 1) == RC_E_ARG                # NULL perms with n_perm > 0
        assert call(xp, 0, n, Y, perm, 1) == RC_E_ARG                # n_rep < 1
        assert call(xp, 1, n, Y, perm, -1) == RC_E_ARG               # n_perm < 0
        assert call(xp, 1, n, Y, perm, 1, 2) == RC_E_ARG and call(xp, 1, n, Y, perm, 1, -1) == RC_E_ARG   # unknown method
        assert call(xp, 1, 2, Y, None, 0) == RC_E_ARG                # n < 3
        for poison in (np.nan, np.inf, -np.inf):
            bad = np.array(Y)
            bad[1, 4] = poison
            assert call(xp, 1, n, bad, perm, 1) == RC_E_ARG          # a non-finite entry above Y's diagonal
            bad = np.array(Y)
            bad[4, 1] = bad[2, 2] = poison
            assert call(xp, 1, n, bad, perm, 1) == 0                 # below or on it: not read
        assert call(xp, 1, n, Y, i32([[0, 1, 2, 3, 4, 4]]), 1) == RC_E_ARG   # not a rearrangement of 0..n-1
        assert call(xp, 1, n, Y, i32([[0, 1, 2, 3, 4, 6]]), 1) == RC_E_ARG
        assert call(xp, 1, n, Y, i32([[0, 1, 2, 3, 4, -1]]), 1) == RC_E_ARG
        assert native.rc_mantel(None, xp, 1, n, Y.ctypes.data_as(vp), None, 0, 0, *[None] * 6) == RC_E_ARG
        # the sample limit is checked before anything is touched
        assert call(xp, 1, 129, Y, perm, 1) == RC_E_LIMIT
        assert call(None, 0, 129, None, None, -1) == RC_E_LIMIT
        assert _code(eng.mantel, np.zeros((1, 129, 129)), np.zeros((129, 129)), None) == RC_E_LIMIT
        assert _code(eng.mantel, X, Y, [[0, 1, 2, 3, 4, 4]]) == RC_E_ARG
        with pytest.raises(ValueError):
            eng.mantel(X, Y[:5, :5])
        with pytest.raises(ValueError):
            eng.mantel(X, Y, perm[:, :5])
        with pytest.raises(ValueError):
            eng.mantel(X, Y, perm, "kendall")
    finally:
        eng.close()


@pytest.mark.parametrize("method", mo.METHODS)
def test_every_null_output_combination(native, method):
    """A 2-D matrix is one replicate; any of the six outputs may be NULL."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    n, P = 5, 7
    Xs = gc.with_nan(gc.matrices(n)[[0, 1, 3, 4, 5]])
    Y = np.ascontiguousarray(_other(n, method))
    perms = mo.perm_rows(n, P)
    vp = ctypes.c_void_p
    code = 0 if method == "pearson" else 1
    eng = _engine()
    try:
        one = eng.mantel(Xs[0], Y, perms, method, perm_stats=True)
        assert len(one) == 1
        _assert_same(one, mo.batch(Xs[:1], Y, perms, method))
        want = eng.mantel(Xs, Y, perms, method, perm_stats=True, allow_nan=True)
        _assert_same(want, mo.batch(Xs, Y, perms, method))
        wants = list(_tuple(want))
        assert want.valid.tolist() == [1, 1, 0, 1, 1]
        for mask in range(64):
            arrs = [np.full(5, 7.0), np.full(5, 7, dtype=np.uint32), np.full(5, 7, dtype=np.uint32),
                    np.full(5, 7, dtype=np.uint32), np.full((5, P), 7.0), np.full(5, 7, dtype=np.uint8)]
            ptr = [a.ctypes.data_as(vp) if mask >> i & 1 else None for i, a in enumerate(arrs)]
            assert native.rc_mantel(eng._h, Xs.ctypes.data_as(vp), 5, n, Y.ctypes.data_as(vp), perms.ctypes.data_as(vp),
                                    P, code, *ptr) == RC_E_NO_IDEAL
            for i, (a, w) in enumerate(zip(arrs, wants)):
                if mask >> i & 1:
                    assert np.array_equal(a, w, equal_nan=True)
                else:
                    assert (a == 7).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# the engine path: rc_resample_mantel on graph-only engines
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


def _check_resample(eng, W, Y, perms, method, order=None):
    """resample_mantel(W) == mantel(resample(W)) as bits, and both equal the oracle."""
    names, mats = eng.resample(W, order, allow_nan=True)
    want = eng.mantel(mats, Y, perms, method, perm_stats=True, allow_nan=True)
    n2, res = eng.resample_mantel(W, Y, perms, order, method, perm_stats=True, allow_nan=True)
    assert n2 == names and _res_same(res, want)
    _assert_same(res, mo.batch(mats, Y, perms, method))
    return res


@pytest.mark.parametrize("S", (4, 6, 8))
def test_resample_mantel_on_graph_engines(native, S):
    """The engines of test_resample_group_test_on_graph_engines: all ones, a
    delete-one jackknife and 50 bootstrap rows, with and without a subset
    order; an empty row; SampleSimilarity with the other matrix's labels in
    another order, missing and surplus."""
    import pandas as pd
    from rna_clique_amd._native import RC_E_NO_IDEAL
    from rna_clique_amd.similarity import NoIdealComponentsError, SampleSimilarity, bootstrap_weights
    from rna_clique_amd import mantel
    case = (pcases.cliques_case(S) if S < 8 else pcases.cliques_case(S, n_each=40, seed=3)).permuted(S)
    eng = _graph_engine(case)
    try:
        C = eng.n_components()
        perms = mo.perm_rows(S, 130, seed=S)
        sub = [int(x) for x in np.random.default_rng(S).permutation(S)[:max(3, S - 1)]]
        sub_perms = mo.perm_rows(len(sub), 20, seed=S)
        boot = bootstrap_weights(C, 50, seed=S)
        for method in mo.METHODS:
            Y, Ysub = _other(S, method), _other(len(sub), method)
            for W in (np.ones((1, C), dtype=np.uint16), 1 - np.eye(C, dtype=np.uint16), boot):
                res = _check_resample(eng, W, Y, perms, method)
                assert res.valid.all()
                _check_resample(eng, W, Ysub, sub_perms, method, sub)
            t = eng.timings()
            assert t["mantel_ms"] > 0 and t["resample_ms"] > 0
            # a row that leaves every pair without rows
            W = np.array(boot[:5])
            W[2] = 0
            assert _code(eng.resample_mantel, W, Y, perms, None, method) == RC_E_NO_IDEAL
            res = _check_resample(eng, W, Y, perms, method)
            assert res.valid.tolist() == [1, 1, 0, 1, 1] and np.isnan(res.statistic[2]) and res.n_abs_ge[2] == 0
        # SampleSimilarity on the same engine
        sim = SampleSimilarity.from_engine(eng)
        D = sim.get_dissimilarity_matrix()
        own = sim.get_dissimilarity_df()
        constant = len(np.unique(D[np.triu_indices(S, 1)])) == 1
        for method in mo.METHODS:
            got = sim.mantel(own, method, permutations=99, seed=5)
            pm = mantel.permutations(S, 99, seed=5)
            w = mo.batch(D[None], D, pm, method)
            assert _bits(got.statistic) == _bits(w[0][0]) and got.valid == 1
            assert (got.n_ge, got.n_le, got.n_abs_ge) == (w[1][0], w[2][0], w[3][0])
            assert constant or (got.statistic == 1.0 and got.n_ge >= 0 and got.p_value("greater") == (1 + got.n_ge) / 100)
            assert (got.n, got.permutations, got.method) == (S, 99, method)
            # another matrix, its labels shuffled: aligned by label
            Y = _other(S, method)
            o = np.random.default_rng(S).permutation(S)
            df = pd.DataFrame(Y, index=sim.samples, columns=sim.samples)
            want = mo.batch(D[None], Y, pm, method)
            for other in (df, df.iloc[o, o], ([sim.samples[i] for i in o], Y[np.ix_(o, o)])):
                got = sim.mantel(other, method, permutations=99, seed=5)
                assert _bits(got.statistic) == _bits(want[0][0]) and got.n_abs_ge == want[3][0]
                assert got.p_value() == (1 + want[3][0]) / 100
            # a sample missing there, a surplus one: an error, or the common ones
            keep = sorted(o[:S - 1].tolist())
            fewer = df.iloc[keep, keep]
            more = pd.DataFrame(_other(S + 1, method), index=sim.samples + ["other"], columns=sim.samples + ["other"])
            for other in (fewer, more):
                with pytest.raises(ValueError):
                    sim.mantel(other, method)
            got = sim.mantel(fewer, method, permutations=30, seed=2, strict=False)
            w2 = mo.batch(D[np.ix_(keep, keep)][None], Y[np.ix_(keep, keep)], mantel.permutations(S - 1, 30, seed=2),
                          method)
            assert _bits(got.statistic) == _bits(w2[0][0]) and got.n_ge == w2[1][0] and got.n == S - 1
            got = sim.mantel(more, method, permutations=30, seed=2, strict=False)
            assert got.n == S
            # bootstrap replicates
            ref, reps = sim.bootstrap_mantel(df, 50, seed=S, method=method, permutations=99)
            mats = sim.resampled_dissimilarity_matrices(boot)
            pm = mantel.permutations(S, 99, seed=S)
            assert _bits(ref.statistic) == _bits(mo.batch(D[None], Y, pm, method)[0][0])
            _assert_same(sim.resampled_mantel(boot, df, method, 99, seed=S, perm_stats=True), mo.batch(mats, Y, pm, method))
            assert np.array_equal(_bits(reps.statistic), _bits(mo.batch(mats, Y, pm[:0], method)[0])) and len(reps) == 50
            with pytest.raises(NoIdealComponentsError):
                sim.resampled_mantel(W, df, method)
    finally:
        eng.close()
