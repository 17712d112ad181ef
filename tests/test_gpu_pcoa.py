"""Principal coordinates on the GPU (pcoa.hip: rc_pcoa, rc_resample_pcoa)
against numpy.linalg.eigh, within the bound tests/pcoa_oracle.py carries
(TOL_UNITS units of u = n 2^-52 ||B||_F, fixed by the oracle's own error on the
host: test_pcoa_host.py). The kernel is not compared with the oracle as bits:
its dot products add in another order. What must be bits -- the same matrix in
another batch position or call, fewer axes, the engine path against rc_pcoa on
the same matrices -- is compared as bits."""
import ctypes

import numpy as np
import pytest

import pcoa_cases as pc
import pcoa_oracle as po
import post_cases as pcases
import treecheck

pytestmark = pytest.mark.gpu

TOL = po.TOL_UNITS


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


def _same_bits(a, b):
    """Two PCoAEigen (or one and a row selection of the other) agree in every bit."""
    return (np.array_equal(_bits(a.values), _bits(b.values)) and np.array_equal(_bits(a.vectors), _bits(b.vectors))
            and np.array_equal(a.sweeps, b.sweeps) and np.array_equal(a.valid, b.valid))


def _rows(res, rows):
    from rna_clique_amd.pcoa import PCoAEigen
    return PCoAEigen(res.values[rows], res.vectors[rows], res.sweeps[rows], res.valid[rows])


def _pdist(X):
    return np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))


# ---------------------------------------------------------------------------
# rc_pcoa on host matrices
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", pc.SIZES)
def test_every_case_within_the_bound(native, n):
    """No pair or one pair (2, 3), odd n with its dummy column, one wave of
    pairs then two (8; 9, 10), one row per lane then two (16, 17) ... up to
    the full 1024-thread block (127, 128); all cases in one batch."""
    from rna_clique_amd.pcoa import eigh_eigen
    Ds = pc.batch(n)
    eng = _engine()
    try:
        res = eng.pcoa(Ds)
        assert eng.timings()["pcoa_ms"] > 0
        few = eng.pcoa(Ds, min(3, n))
    finally:
        eng.close()
    assert res.values.shape == (len(Ds), n) and res.vectors.shape == (len(Ds), n, n)
    assert res.valid.tolist() == [1] * len(Ds)
    assert (0 < res.sweeps).all() and (res.sweeps < po.DEFAULT_SWEEPS).all()
    assert (np.diff(res.values, axis=1) <= 0).all()
    # k < n: exactly the first k columns
    assert np.array_equal(_bits(few.values), _bits(res.values)) and np.array_equal(few.sweeps, res.sweeps)
    assert np.array_equal(_bits(few.vectors), _bits(res.vectors[:, :, :min(3, n)]))
    for i, name in enumerate(pc.NAMES):
        vals, vecs = res.values[i], res.vectors[i]
        e = po.errors(Ds[i], vals, vecs)
        print(f"n={n} {name}: sweeps {res.sweeps[i]} E_gram {e[0]:.2f} E_val {e[1]:.2f} E_res {e[2]:.2f} "
              f"E_orth {e[3]:.2f}")
        if not Ds[i].any():   # `zero`, and `duplicate` at n = 2: exact zeros, zero vectors
            assert e[:3] == (0.0, 0.0, 0.0) and not vecs.any() and res.sweeps[i] == 1
            continue
        assert (np.abs(np.linalg.norm(vecs, axis=0) - 1) < 1e-12).all()   # no zero vector
        assert max(e) <= TOL, (name, e)
        # the sign rule: the entry of largest magnitude is positive (the rule reads the column
        # before it is scaled to unit length, so magnitudes that differ there may tie here)
        mag = np.abs(vecs)
        lead = mag >= mag.max(axis=0) * (1 - 2.0 ** -50)
        assert ((vecs > 0) & lead).any(axis=0).all()
    # spectrum: the eigenvalues it was built with, and eigh's coordinates
    i = pc.NAMES.index("spectrum")
    D, lams = Ds[i], pc.spectrum_lams(n)
    u = po.unit(po.centre(D))
    nl = len(lams)
    assert np.abs(res.values[i, :nl] - lams).max() <= TOL * u
    assert np.abs(res.values[i, nl:]).max() <= TOL * u
    w, W = eigh_eigen(D, nl)
    tol = np.sqrt(lams[0]) * 4 * TOL * u / pc.GAP   # Davis-Kahan: eigenvalue gaps of at least GAP
    X = res.vectors[i, :, :nl] * np.sqrt(res.values[i, :nl])
    assert np.abs(X - W * np.sqrt(w[:nl])).max() <= tol
    assert np.abs(_pdist(X) - D).max() <= tol


def test_more_replicates_than_workgroups_fit(native):
    """300 replicates of 8 samples: the same matrix at positions 0 and 299
    gives the same bits, and so does a second call."""
    rng = np.random.default_rng(300)
    Ds = np.stack([pc.noneuclid(8, seed=int(s)) for s in rng.integers(1 << 30, size=300)])
    Ds[299] = Ds[0]
    eng = _engine()
    try:
        a = eng.pcoa(Ds)
        b = eng.pcoa(Ds)
    finally:
        eng.close()
    assert a.valid.all() and len(set(a.sweeps.tolist())) > 1
    assert _same_bits(_rows(a, [0]), _rows(a, [299]))
    assert not np.array_equal(a.values[0], a.values[1])
    assert _same_bits(a, b)
    for r in (0, 150, 299):
        assert max(po.errors(Ds[r], a.values[r], a.vectors[r])) <= TOL


@pytest.mark.parametrize("n", (5, 65))
def test_nonfinite_replicate_is_flagged_and_the_rest_unaffected(native, n):
    from rna_clique_amd._native import RC_E_NO_IDEAL
    Ds = np.array(pc.batch(n)[[0, 1, 3, 5, 6]])
    eng = _engine()
    try:
        clean = eng.pcoa(Ds, 3)
        for poison in (np.nan, -np.inf):
            Ds[2, 1, n - 1] = poison
            assert _code(eng.pcoa, Ds, 3) == RC_E_NO_IDEAL
            res = eng.pcoa(Ds, 3, allow_nan=True)
            assert res.valid.tolist() == [1, 1, 0, 1, 1] and res.sweeps[2] == 0
            assert np.isnan(res.values[2]).all() and np.isnan(res.vectors[2]).all()
            assert _same_bits(_rows(res, [0, 1, 3, 4]), _rows(clean, [0, 1, 3, 4]))
        # garbage below and on the diagonal is not read
        Ds[2, 1, n - 1] = pc.batch(n)[3][1, n - 1]
        Ds[:, np.tril_indices(n)[0], np.tril_indices(n)[1]] = np.nan
        assert _same_bits(eng.pcoa(Ds, 3), clean)
        # a finite entry whose square overflows: sigma is not finite
        Ds[4, 0, 1] = 1e200
        res = eng.pcoa(Ds, 3, allow_nan=True)
        assert res.valid.tolist() == [1, 1, 1, 1, 0] and _same_bits(_rows(res, [0, 1, 2, 3]), _rows(clean, [0, 1, 2, 3]))
    finally:
        eng.close()


def test_one_sweep_is_not_enough(native):
    """max_sweeps=1 on noneuclid at 8 samples: RC_E_LIMIT with the state after
    that sweep; a one-dimensional 2-D input is one replicate."""
    from rna_clique_amd._native import RC_E_LIMIT
    n = 8
    D = np.ascontiguousarray(pc.batch(n)[1])
    vp = ctypes.c_void_p
    values, vectors = np.full(n, 7.0), np.full((n, n), 7.0)
    sweeps, valid = np.full(1, 7, dtype=np.int32), np.full(1, 7, dtype=np.uint8)
    eng = _engine()
    try:
        assert _code(eng.pcoa, D, max_sweeps=1) == RC_E_LIMIT
        code = native.rc_pcoa(eng._h, D.ctypes.data_as(vp), 1, n, n, 1, values.ctypes.data_as(vp),
                              vectors.ctypes.data_as(vp), sweeps.ctypes.data_as(vp), valid.ctypes.data_as(vp))
        full = eng.pcoa(D)
        exact = eng.pcoa(D, max_sweeps=int(full.sweeps[0]))   # the last, clean sweep fits: no error
    finally:
        eng.close()
    assert code == RC_E_LIMIT and sweeps.tolist() == [1] and valid.tolist() == [1]
    assert np.isfinite(values).all() and np.isfinite(vectors).all()
    assert full.values.shape == (1, n) and 2 < full.sweeps[0] < po.DEFAULT_SWEEPS
    assert _same_bits(full, exact)
    assert not np.array_equal(values, full.values[0])


def test_argument_errors(native):
    """Argument checks only: nothing here reaches a kernel."""
    from rna_clique_amd._native import RC_E_ARG, RC_E_LIMIT
    D = np.ascontiguousarray(pc.batch(5)[:1])
    vp = ctypes.c_void_p
    eng = _engine()
    try:
        def call(dp, r, n, k, ms):
            return native.rc_pcoa(eng._h, dp, r, n, k, ms, None, None, None, None)
        dp = D.ctypes.data_as(vp)
        assert call(dp, 1, 1, 1, 0) == RC_E_ARG      # n < 2
        assert call(dp, 0, 5, 5, 0) == RC_E_ARG      # n_rep < 1
        assert call(dp, 1, 5, 0, 0) == RC_E_ARG      # k < 1
        assert call(dp, 1, 5, 6, 0) == RC_E_ARG      # k > n
        assert call(dp, 1, 5, 5, -1) == RC_E_ARG     # max_sweeps < 0
        assert call(None, 1, 5, 5, 0) == RC_E_ARG    # NULL D
        # the sample limit is checked before anything is touched
        assert call(dp, 1, 129, 3, 0) == RC_E_LIMIT
        assert call(None, 0, 129, 0, -1) == RC_E_LIMIT
        assert _code(eng.pcoa, np.zeros((1, 129, 129))) == RC_E_LIMIT
        assert _code(eng.pcoa, np.zeros((1, 1, 1))) == RC_E_ARG
        assert _code(eng.pcoa, np.zeros((0, 5, 5))) == RC_E_ARG
        assert _code(eng.pcoa, D, 6) == RC_E_ARG
        with pytest.raises(ValueError):
            eng.pcoa(np.zeros((1, 4, 5)))
        assert call(dp, 1, 5, 5, 0) == 0             # every output NULL
    finally:
        eng.close()


def test_every_null_output_combination(native):
    from rna_clique_amd._native import RC_E_NO_IDEAL
    n, k = 5, 2
    Ds = np.array(pc.batch(n)[[0, 1, 3, 5, 6]])
    Ds[2, 0, 3] = np.nan
    vp = ctypes.c_void_p
    eng = _engine()
    try:
        want = eng.pcoa(Ds, k, allow_nan=True)
        wants = [want.values, want.vectors, want.sweeps, want.valid]
        assert want.valid.tolist() == [1, 1, 0, 1, 1]
        for mask in range(16):
            arrs = [np.full((5, n), 7.0), np.full((5, n, k), 7.0), np.full(5, 7, dtype=np.int32),
                    np.full(5, 7, dtype=np.uint8)]
            ptr = [a.ctypes.data_as(vp) if mask >> i & 1 else None for i, a in enumerate(arrs)]
            assert native.rc_pcoa(eng._h, Ds.ctypes.data_as(vp), 5, n, k, 0, *ptr) == RC_E_NO_IDEAL
            for i, (a, w) in enumerate(zip(arrs, wants)):
                if mask >> i & 1:
                    assert np.array_equal(a, w, equal_nan=True)
                else:
                    assert (a == 7).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# the engine path: rc_resample_pcoa on graph-only engines
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


def _check_resample(eng, W, order=None, k=None):
    """resample_pcoa(W) == pcoa(resample(W)) as bits: the same kernel on the same input."""
    labels, mats = eng.resample(W, order, allow_nan=True)
    want = eng.pcoa(mats, k, allow_nan=True)
    l2, res = eng.resample_pcoa(W, order, k, allow_nan=True)
    assert l2 == labels and _same_bits(res, want)
    return res


@pytest.mark.parametrize("S", (4, 6, 8))
def test_resample_pcoa_on_graph_engines(native, S):
    """Clique cases of tests/post_cases.py over 4 and 6 samples and a synthetic
    one over 8 (40 ideal components): all ones, a delete-one jackknife and 50
    bootstrap rows, with and without order; an empty row; SampleSimilarity."""
    from rna_clique_amd._native import RC_E_NO_IDEAL
    from rna_clique_amd.pcoa import pcoa_eigh
    from rna_clique_amd.similarity import NoIdealComponentsError, SampleSimilarity, bootstrap_weights
    case = (pcases.cliques_case(S) if S < 8 else pcases.cliques_case(S, n_each=40, seed=3)).permuted(S)
    eng = _graph_engine(case)
    try:
        C = eng.n_components()
        assert C == (25 if S < 8 else 40)
        order = [int(x) for x in np.random.default_rng(S).permutation(S)[:max(3, S - 1)]]
        boot = bootstrap_weights(C, 50, seed=S)
        for W in (np.ones((1, C), dtype=np.uint16), 1 - np.eye(C, dtype=np.uint16), boot):
            res = _check_resample(eng, W)
            assert res.valid.all()
            _check_resample(eng, W, order, 2)
        t = eng.timings()
        assert t["pcoa_ms"] > 0 and t["resample_ms"] > 0
        # a row that leaves every pair without rows
        W = np.array(boot[:5])
        W[2] = 0
        assert _code(eng.resample_pcoa, W) == RC_E_NO_IDEAL
        res = _check_resample(eng, W)
        assert res.valid.tolist() == [1, 1, 0, 1, 1] and np.isnan(res.values[2]).all()
        assert _same_bits(_rows(res, [0, 1, 3, 4]), _rows(eng.resample_pcoa(boot[:5])[1], [0, 1, 3, 4]))
        # SampleSimilarity on the same engine
        sim = SampleSimilarity.from_engine(eng)
        D = sim.get_dissimilarity_matrix()
        got, want = sim.pcoa(), pcoa_eigh(D, sim.samples, warn=False)
        u = po.unit(po.centre(D))
        assert list(got.samples.index) == sim.samples and got.samples.shape == (S, S)
        assert np.abs(got.eigvals.to_numpy() - want.eigvals.to_numpy()).max() <= TOL * u
        perr = np.abs(got.proportion_explained.to_numpy() - want.proportion_explained.to_numpy()).max()
        print(f"S={S}: u {u:.3e}, eigvals off by {np.abs(got.eigvals.to_numpy() - want.eigvals.to_numpy()).max() / u:.2f} u, "
              f"proportions by {perr / u:.2f} u (sum of eigenvalues {want.eigvals.to_numpy().sum():.3e})")
        # a proportion is an eigenvalue over the eigenvalues' sum, so the eigenvalues' bound is
        # divided by that sum too (TOL * u itself is below the spacing of doubles near 0.5)
        assert perr <= TOL * u / want.eigvals.to_numpy().sum()
        assert sim.pcoa(2).samples.shape == (S, 2)
        ref, reps = sim.bootstrap_pcoa(50, seed=S)
        assert reps.shape == (50, S, 3) and ref.samples.shape == (S, 3) and np.isfinite(reps).all()
        assert np.array_equal(reps, sim.resampled_pcoa(boot))
        # aligned replicates are no farther from the reference than unaligned ones
        from rna_clique_amd.pcoa import clamp
        raw = eng.resample_pcoa(boot, sim._order(), 3)[1]
        coords = clamp(raw.values, raw.vectors)[1]
        R = ref.coordinates
        assert (np.linalg.norm(reps - R, axis=(1, 2)) <= np.linalg.norm(coords - R, axis=(1, 2)) * (1 + 1e-12)).all()
        with pytest.raises(NoIdealComponentsError):
            sim.resampled_pcoa(W)
    finally:
        eng.close()


def test_two_samples(native):
    """A two-sample graph (50 ideal components): one axis, whose coordinates
    lie the pair's distance apart; the default of 3 dimensions means both."""
    from rna_clique_amd.similarity import SampleSimilarity
    eng = _graph_engine(pcases.star_case(n=50))
    try:
        sim = SampleSimilarity.from_engine(eng)
        assert len(sim.samples) == 2
        d = sim.get_dissimilarity_matrix()[0, 1]
        res = sim.pcoa()
        assert res.samples.shape == (2, 2) and not res.coordinates[:, 1].any()
        assert abs(abs(res.coordinates[0, 0] - res.coordinates[1, 0]) - d) <= 4 * 2.0 ** -52 * d
        ref, reps = sim.bootstrap_pcoa(5)
        assert ref.samples.shape == (2, 2) and reps.shape == (5, 2, 2)
        with pytest.raises(ValueError):
            sim.pcoa(3)
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# science level
# ---------------------------------------------------------------------------

def test_first_axis_of_a_simulated_run_separates_the_deepest_split(native):
    """8 samples x 1000 genes aligned by the engine (the run of test_gpu_nj's
    last test). One of the root's two lineages went extinct in this seed's
    birth-death tree, and the surviving tree is a caterpillar: its deepest
    divergence is the first sample against the other seven -- a trivial split,
    which treecheck.tree_splits does not list -- and its deepest listed split
    puts the first two samples against the other six. The first axis
    separates both, on the GPU and by pcoa_eigh on the same matrix: the first
    sample alone has a positive coordinate, and the second sample lies above
    every one of the other six."""
    from rna_clique_amd.pcoa import pcoa_eigh
    from rna_clique_amd.similarity import SampleSimilarity
    from rna_clique_amd.simulate import simulate
    samples, (parent, _, leaves) = simulate(taxa=8, genes=1000, seed=487)
    names = {leaf: samples[i].name for i, leaf in enumerate(leaves)}
    truth = treecheck.tree_splits(parent, leaves, names)
    far = max(truth, key=len)   # the side without the first leaf of the deepest listed split
    assert len(far) == 6 and all(s <= far for s in truth)
    eng = _engine()
    try:
        for s in samples:
            eng.add_sample(s.name, s.seq, s.tx_offsets, s.gene, s.iso)
        eng.run()
        sim = SampleSimilarity.from_engine(eng)
        D = sim.get_dissimilarity_matrix()
        got = sim.pcoa(3)
    finally:
        eng.close()
    want = pcoa_eigh(D, sim.samples, 3, warn=False)
    near = [s for s in sim.samples if s not in far]
    assert len(near) == 2
    for res in (want, got):
        pc1 = res.samples["PC1"]
        print(pc1.to_string())
        first = pc1.idxmax()
        assert first in near and pc1[first] > 0 and (pc1.drop(first) < 0).all()
        assert pc1[near].min() > pc1[sorted(far)].max()
        assert res.proportion_explained.iloc[0] > 0.5
    u = po.unit(po.centre(D))
    assert np.abs(got.eigvals.to_numpy()[:3] - want.eigvals.to_numpy()[:3]).max() <= TOL * u
