"""Principal coordinates on the host: tests/pcoa_oracle.py (the numpy statement
of pcoa.hip) measured against numpy.linalg.eigh on every case of
tests/pcoa_cases.py -- a CPU measurement of the specification against the
reference, which fixes the bound the GPU tests use --, and rna_clique_amd/pcoa.py
(PCoAResult's clamp rule, pcoa_eigh, procrustes_align, argument checks)."""
import functools
import math
import warnings

import numpy as np
import pytest

import pcoa_cases as pc
import pcoa_oracle as po


@functools.lru_cache(maxsize=None)
def _oracle(n):
    out = po.pcoa_batch(pc.batch(n))
    for a in out:
        a.setflags(write=False)
    return out


def _errors(n):
    """{case: (E_gram, E_val, E_res, E_orth)} of the oracle at n samples; a
    zero matrix (`zero`, and `duplicate` at n = 2) must give exact zeros and
    zero vectors, and has no E_orth."""
    Ds = pc.batch(n)
    values, vectors, sweeps, valid, rotating = _oracle(n)
    assert valid.all() and not rotating.any()
    out = {}
    for i, name in enumerate(pc.NAMES):
        e = po.errors(Ds[i], values[i], vectors[i])
        if not Ds[i].any():
            assert e[:3] == (0.0, 0.0, 0.0) and not vectors[i].any() and sweeps[i] == 1
            continue
        assert (np.abs(np.linalg.norm(vectors[i], axis=0) - 1) < 1e-12).all()   # no zero vector
        out[name] = e
    return out


@pytest.mark.parametrize("n", pc.SIZES)
def test_oracle_against_eigh(n):
    errs = _errors(n)
    print(f"n={n}: " + "; ".join(f"{k} " + " ".join(f"{x:.2f}" for x in v) for k, v in errs.items()))
    for name, e in errs.items():
        assert max(e) <= po.TOL_UNITS, (name, e)
    sweeps = _oracle(n)[2]
    assert (0 < sweeps).all() and (sweeps < po.DEFAULT_SWEEPS).all()


def test_tol_units_is_the_next_power_of_two_above_twice_the_worst():
    worst = max(max(e) for n in pc.SIZES for e in _errors(n).values())
    print(f"worst error of the oracle against eigh: {worst:.3f} units")
    assert po.TOL_UNITS == 2 ** math.ceil(math.log2(2 * worst)) and po.TOL_UNITS > 2 * worst


@pytest.mark.parametrize("n", (3, 17, 128))
def test_spectrum_case_has_its_eigenvalues(n):
    """The case's own construction, by eigh: the eigenvalues are LAMS."""
    from rna_clique_amd.pcoa import eigh_eigen
    D = pc.batch(n)[pc.NAMES.index("spectrum")]
    w, _ = eigh_eigen(D)
    lams = pc.spectrum_lams(n)
    u = po.unit(po.centre(D))
    assert np.abs(w[:len(lams)] - lams).max() <= u and np.abs(w[len(lams):]).max() <= u


def test_oracle_step_pairs_are_a_tournament():
    for n in (2, 3, 4, 5, 8, 9, 127, 128):
        m = (n + 1) & ~1
        seen = set()
        for s in range(m - 1):
            p, q = po.step_pairs(n, s)
            cols = np.concatenate([p, q])
            assert len(set(cols.tolist())) == len(cols) and (p < q).all() and (q < n).all()
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == n * (n - 1) // 2


def test_oracle_flags_nonfinite_and_k():
    Ds = np.array(pc.batch(5)[[0, 1, 3]])
    Ds[1, 0, 4] = np.nan
    Ds[0, 4, 0] = np.inf   # below the diagonal: not read
    values, vectors, sweeps, valid, _ = po.pcoa_batch(Ds, k=2)
    assert valid.tolist() == [1, 0, 1] and sweeps[1] == 0 and np.isnan(values[1]).all() and np.isnan(vectors[1]).all()
    full = _oracle(5)
    assert vectors.shape == (3, 5, 2)
    assert np.array_equal(values[[0, 2]], full[0][[0, 3]]) and np.array_equal(vectors[[0, 2]], full[1][[0, 3], :, :2])
    # one sweep on a matrix that needs more: still rotating
    _, _, sw, _, rotating = po.pcoa_batch(pc.batch(8)[1], max_sweeps=1)
    assert sw.tolist() == [1] and rotating.tolist() == [True]


# ---------------------------------------------------------------------------
# rna_clique_amd/pcoa.py
# ---------------------------------------------------------------------------

def test_result_clamp_rule_on_noneuclid():
    from rna_clique_amd.pcoa import PCoAResult, eigh_eigen
    n = 16
    D = pc.noneuclid(n, seed=1)
    w, V = eigh_eigen(D)
    assert (w < -1e-3).sum() >= 4 and (w > 1e-3).sum() >= 4
    w[5] = 1e-12    # close to zero: becomes 0 without counting as negative
    labels = [f"s{i}" for i in range(n)]
    with pytest.warns(RuntimeWarning, match="negative eigenvalues"):
        res = PCoAResult(labels, w, V[:, :6])
    pos = np.where(w > 1e-8, w, 0.0)
    assert list(res.samples.index) == labels and list(res.samples.columns) == [f"PC{i}" for i in range(1, 7)]
    assert list(res.eigvals.index) == [f"PC{i}" for i in range(1, n + 1)]
    assert np.array_equal(res.eigvals.to_numpy(), pos) and res.eigvals.iloc[5] == 0.0
    assert np.array_equal(res.proportion_explained.to_numpy(), pos / pos.sum())
    assert abs(res.proportion_explained.sum() - 1) < 1e-15
    assert np.array_equal(res.coordinates, V[:, :6] * np.sqrt(pos[:6])) and not res.coordinates[:, 5].any()
    assert np.array_equal(res.raw_eigvals, w)
    # negative axes are zero columns
    full = PCoAResult(labels, w, V, warn=False)
    assert not full.coordinates[:, w < 0].any() and full.coordinates[:, 0].any()
    # no warning without negative eigenvalues
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        PCoAResult(labels, np.abs(w), V)
    # all-zero eigenvalues: proportions are 0, not NaN
    assert not PCoAResult(labels, np.zeros(n), V).proportion_explained.to_numpy().any()


def test_pcoa_eigh_reproduces_euclidean_distances():
    from rna_clique_amd.pcoa import gower_centre, pcoa_eigh
    n = 12
    D = pc.euclid3(n, seed=3)
    res = pcoa_eigh(D, [f"s{i}" for i in range(n)], 3)
    X = res.coordinates
    assert X.shape == (n, 3) and np.abs(X.sum(axis=0)).max() < 1e-12
    got = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    assert np.abs(got - D).max() < 1e-12
    assert np.abs(res.eigvals.to_numpy()[3:]).max() == 0.0 and abs(res.proportion_explained.iloc[:3].sum() - 1) < 1e-12
    # the upper triangle alone is read; the centred matrix is the oracle's up to rounding
    G = np.array(D)
    G[np.tril_indices(n)] = np.nan
    assert np.array_equal(pcoa_eigh(G, dimensions=3).coordinates, X)
    assert np.abs(gower_centre(D) - po.centre(D)).max() <= 4 * 2.0 ** -52 * np.abs(po.centre(D)).max()
    # largest entry of every vector positive
    top = np.abs(X).argmax(axis=0)
    assert (X[top, range(3)] > 0).all()


def test_procrustes_recovers_a_rotation_reflection():
    from rna_clique_amd.pcoa import procrustes_align
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((20, 3))
    Qs = [np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(6)]
    Qs[0][:, 0] *= -np.sign(np.linalg.det(Qs[0]))   # a reflection (det -1) ...
    Qs[1][:, 0] *= np.sign(np.linalg.det(Qs[1]))    # ... and a proper rotation
    assert np.linalg.det(Qs[0]) < 0 < np.linalg.det(Qs[1])
    X = np.stack([ref @ Q for Q in Qs])
    assert np.abs(procrustes_align(X, ref) - ref).max() < 1e-14
    assert np.abs(procrustes_align(X[2], ref) - ref).max() < 1e-14
    # batched references too, and never farther than before
    Y = X + 0.1 * rng.standard_normal(X.shape)
    A = procrustes_align(Y, np.broadcast_to(ref, Y.shape))
    assert np.array_equal(A, procrustes_align(Y, ref))
    assert (np.linalg.norm(A - ref, axis=(1, 2)) <= np.linalg.norm(Y - ref, axis=(1, 2))).all()


def test_python_argument_checks():
    from rna_clique_amd.pcoa import PCoAResult, pcoa_eigh, procrustes_align
    from rna_clique_amd.similarity import SampleSimilarity
    D = pc.euclid3(5)
    for bad in (np.zeros((1, 1)), np.zeros((3, 4)), np.zeros(4)):
        with pytest.raises(ValueError):
            pcoa_eigh(bad)
    for k in (0, 6):
        with pytest.raises(ValueError):
            pcoa_eigh(D, dimensions=k)
    N = np.array(D)
    N[0, 1] = np.nan
    with pytest.raises(ValueError):
        pcoa_eigh(N)
    with pytest.raises(ValueError):
        PCoAResult(["a", "b"], np.zeros(3), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        procrustes_align(np.zeros((4, 3)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        procrustes_align(np.full((4, 2), np.nan), np.zeros((4, 2)))
    # SampleSimilarity's sample-count checks need no engine
    sim = SampleSimilarity.__new__(SampleSimilarity)
    sim._sim_pairs = None
    for count, match in ((1, "at least 2"), (129, "pcoa_eigh")):
        sim.labels, sim._samples = [f"s{i:03d}" for i in range(count)], None
        for fn in (sim.pcoa, lambda: sim.resampled_pcoa([[1]]), lambda: sim.bootstrap_pcoa(5)):
            with pytest.raises(ValueError, match=match):
                fn()
    sim.labels, sim._samples = ["a", "b", "c"], None
    for k in (0, 4):
        with pytest.raises(ValueError, match="dimensions"):
            sim.pcoa(k)
    assert sim._pcoa_order(3, clip=True)[1] == 3 and sim._pcoa_order(7, clip=True)[1] == 3
