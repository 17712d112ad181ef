"""PERMDISP's specification (tests/dispersion_oracle.py) against a plain
statement from coordinates and scipy's one-way ANOVA, its partition invariance,
and the host route rna_clique_amd.groups.dispersion_host against the oracle's
bits. No GPU."""

import numpy as np
import pytest
from scipy.stats import f_oneway

import dispersion_oracle as do
import group_cases as gc
import group_oracle as go
from rna_clique_amd import groups

U = 2.0 ** -53   # the unit roundoff of float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Two oracle-style tuples agree: floats as bits, the rest exactly."""
    return all(np.array_equal(_bits(x), _bits(y)) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y)
               for x, y in zip(a, b))


def _host_tuple(res):
    return (res.statistic, res.n_ge, res.total, res.within, res.perm_statistics, res.valid, res.distances)


# ---------------------------------------------------------------------------
# the oracle against coordinates
# ---------------------------------------------------------------------------

def _points(n, k, seed):
    """n points in R^k and their distance matrix, rounded once from extended
    precision (so every distance carries at most one rounding, U relative)."""
    x = np.random.default_rng(seed).normal(size=(n, k))
    xl = x.astype(np.longdouble)
    diff = xl[:, None, :] - xl[None, :, :]
    return x, np.sqrt((diff * diff).sum(axis=2)).astype(np.float64)


def _plain(x, labels):
    """(z, s2 per sample) from the coordinates in extended precision: the
    distance to the group mean, and the group's mean squared distance to it."""
    xl = x.astype(np.longdouble)
    z = np.zeros(len(x), dtype=np.longdouble)
    s2 = np.zeros(len(x), dtype=np.longdouble)
    for g in np.unique(labels):
        m = labels == g
        d = xl[m] - xl[m].mean(axis=0)
        z[m] = np.sqrt((d * d).sum(axis=1))
        s2[m] = (d * d).sum() / m.sum()
    return z.astype(np.float64), s2.astype(np.float64)


def _designs(n):
    two = np.arange(n) % 2
    three = np.arange(n) % 3
    single = np.zeros(n, dtype=np.int64)
    single[n // 2:] = 1
    single[n - 1] = 2                       # a singleton
    return {"two": two, "three": three, "singleton": single}


@pytest.mark.parametrize("k", (2, 5))
@pytest.mark.parametrize("n", (6, 9, 33))
def test_oracle_matches_coordinates_and_scipy(n, k):
    """For a point at distance z of its group's centroid, in a group whose mean
    squared distance to the centroid is s2: t / n_g = z^2 + s2 and
    b / (2 n_g^2) = s2, so z2 is the difference of two numbers of that size.
    A distance carries U (rounded once from extended precision), its square 3 U;
    t adds at most n terms ((n + 2) U in all), b adds n of those ((2 n + 1) U),
    each division and the subtraction one more: the error of z2 is at most
    U ((n + 4) z^2 + (3 n + 5) s2) <= (2 n + 4) U (z^2 + 2 s2), and as
    |sqrt(a + e) - sqrt(a)| <= |e| / sqrt(a), that of z at most
    e_i = (2 n + 4) U (z^2 + 2 s2) / z + U z. The plain statement runs in extended
    precision, its own error is 2^-11 of this.
    The sums of squares are squared lengths of projections of z, so an error
    vector of length E in z moves sqrt(SS) by at most E: |dSS| <= 2 E sqrt(SS) +
    E^2. The ANOVA itself forms z - m with m a mean of at most n terms:
    (n + 3) U max z per sample, once in the oracle and once in scipy, which
    joins e_i. SS_A = SS_T - SS_W carries both errors, so
    |dF| / F <= (dSS_T + dSS_W) / SS_A + dSS_W / SS_W, to first order."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    x, D = _points(n, k, seed=100 * n + k)
    for name, labels in _designs(n).items():
        sizes = np.bincount(labels)
        a = len(sizes)
        want, s2 = _plain(x, labels)
        z, z2 = do.centroid_distances(D, labels)
        alone = sizes[labels] == 1
        assert (z[alone] == 0).all() and (z2[alone] == 0).all()
        e = np.zeros(n)
        e[~alone] = (2 * n + 4) * U * (want[~alone] ** 2 + 2 * s2[~alone]) / want[~alone] + U * want[~alone]
        err = np.abs(z - want)
        print(f"n={n} k={k} {name}: z off by at most {err.max():.2e}, {np.max(err[~alone] / e[~alone]):.3f} of the bound")
        assert (err <= e).all()
        assert np.array_equal(_bits(z), _bits(groups.centroid_distances(D, labels)))
        F, n_ge, sst, ssw, pF, valid, dist = do.permdisp(D, labels, gc.perm_rows(labels, 5, seed=n))
        assert valid == 1 and np.array_equal(_bits(dist), _bits(z)) and _bits(pF[0]) == _bits(F) and n_ge >= 1
        E = np.linalg.norm(e + 2 * (n + 3) * U * want.max())
        if sizes.max() <= 2:   # two members are equally far from their mean: SS_W is 0 but for rounding, F is x / 0
            assert ssw <= E * E
            continue
        ref = f_oneway(*[want[labels == g] for g in range(a)]).statistic
        p_ssw = sum(((want[labels == g] - want[labels == g].mean()) ** 2).sum() for g in range(a))
        p_sst = ((want - want.mean()) ** 2).sum()
        dss = lambda ss: 2 * E * np.sqrt(ss) + E * E   # noqa: E731
        bound = (dss(p_sst) + dss(p_ssw)) / (p_sst - p_ssw) + dss(p_ssw) / p_ssw + 8 * U
        print(f"    F {F:.6g}, off by {abs(F - ref) / ref:.2e} of a bound of {bound:.2e}")
        assert abs(F - ref) <= bound * ref
        assert abs(sst - p_sst) <= dss(p_sst) + 4 * U * p_sst and abs(ssw - p_ssw) <= dss(p_ssw) + 4 * U * p_ssw


def test_a_negative_squared_distance_takes_the_absolute_value():
    """Samples 0, 1, 2 form a group with d(1, 2) = 10 far beyond d(0, 1) +
    d(0, 2) = 2: sample 0 lies at an imaginary distance of the centroid,
    z2 = 2 / 3 - 204 / 18 = -32 / 3."""
    n = 6
    D = go.mirrored(gc.matrices(n)[3])
    D[0, 1] = D[1, 0] = D[0, 2] = D[2, 0] = 1.0
    D[1, 2] = D[2, 1] = 10.0
    labels = np.array([0, 0, 0, 1, 1, 1])
    z, z2 = do.centroid_distances(D, labels)
    assert z2[0] < 0 and abs(z2[0] + 32 / 3) <= 8 * U * 12 and z2[1] > 0 and z2[2] > 0
    assert _bits(z[0]) == _bits(np.sqrt(-z2[0])) and (z > 0).all()
    perms = gc.perm_rows(labels, 30, seed=1)
    want = do.batch(D[None], labels, perms)
    assert np.isfinite(want[0]).all() and np.array_equal(_bits(want[6][0]), _bits(z))
    assert _same(_host_tuple(groups.dispersion_host(D, labels, perms, perm_stats=True)), want)
    assert np.array_equal(_bits(groups.centroid_distances(D, labels)), _bits(z))


# ---------------------------------------------------------------------------
# partition invariance, small designs, degenerate inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", (3, 4, 5, 8, 31, 33, 64, 65))
def test_the_same_partition_gives_the_same_bits(n):
    Ds = gc.matrices(n)
    for labels in gc.groupings(n).values():
        perms = gc.perm_rows(labels, 30, seed=n + 1)
        want = do.batch(Ds, labels, perms)
        assert _same(_host_tuple(groups.dispersion_host(Ds, labels, perms, perm_stats=True)), want)
        for m in gc.renumberings(labels, seed=n):
            assert _same(do.batch(Ds, m[labels], m[perms]), want)
            assert _same(_host_tuple(groups.dispersion_host(Ds, m[labels], m[perms], perm_stats=True)), want)
        rows = gc.same_partition_rows(labels, seed=n)
        stat, n_ge, _, _, ps, _, _ = do.batch(Ds, labels, rows)
        assert np.array_equal(_bits(ps), _bits(np.repeat(stat[:, None], len(rows), axis=1)))
        ok = ~np.isnan(stat)
        assert np.array_equal(n_ge[ok], np.full(ok.sum(), len(rows))) and (n_ge[~ok] == 0).all()


def test_six_samples_in_two_groups_of_three():
    labels = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    perms = gc.perm_rows(labels, 200, seed=6)
    for D in gc.matrices(6):
        want = do.six_sample_expected(D, labels, perms)
        assert want >= 1 or np.isnan(do.permdisp(D, labels)[0])
        assert do.permdisp(D, labels, perms)[1] == want
        res = groups.dispersion_host(D, labels, perms)
        assert int(res.n_ge[0]) == want and res.p_value[0] == (1 + want) / 201


def test_degenerate_matrices():
    """No distances at all: z = 0, F = 0 / 0. All distances equal with balanced
    groups: every z is the same, SS_W is 0 or a rounding residue, and the
    routes agree on whatever IEEE arithmetic makes of it."""
    for n in (5, 8, 33):
        for labels in gc.groupings(n).values():
            perms = gc.perm_rows(labels, 25, seed=n)
            for D in (np.zeros((n, n)), gc.nj_cases.all_equal(n)):
                want = do.batch(D[None], labels, perms)
                res = groups.dispersion_host(D, labels, perms, perm_stats=True)
                assert _same(_host_tuple(res), want) and res.valid[0] == 1
            assert np.isnan(want[0][0]) or np.any(D)
    res = groups.dispersion_host(np.zeros((8, 8)), gc.groupings(8)["balanced"], gc.perm_rows(gc.groupings(8)["balanced"], 9))
    assert np.isnan(res.statistic[0]) and res.n_ge[0] == 0 and res.p_value[0] == 0.1 and (res.distances == 0).all()


def test_invalid_matrix_leaves_the_others_alone():
    n = 8
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, 10)
    Ds = gc.matrices(n)
    clean = groups.dispersion_host(Ds, labels, perms, perm_stats=True)
    for poison in (np.nan, np.inf, -np.inf):
        bad = gc.with_nan(Ds)
        bad[2, 0, n - 1] = poison
        res = groups.dispersion_host(bad, labels, perms, perm_stats=True)
        assert _same(_host_tuple(res), do.batch(bad, labels, perms))
        assert res.valid.tolist() == [1, 1, 0, 1, 1, 1] and res.n_ge[2] == 0
        assert np.isnan([res.statistic[2], res.total[2], res.within[2], res.p_value[2]]).all()
        assert np.isnan(res.perm_statistics[2]).all() and np.isnan(res.distances[2]).all()
        keep = [0, 1, 3, 4, 5]
        assert _same([x[keep] for x in _host_tuple(res)], [x[keep] for x in _host_tuple(clean)])


def test_rejected_arguments_and_existing_methods():
    D = gc.matrices(6)[0]
    good = np.array([0, 0, 1, 1, 2, 2])
    for labels, perms in ((np.arange(6), None), (np.zeros(6, dtype=int), None), ([0, 0, 2, 2, 3, 3], None),
                          ([0, 0, -1, 1, 1, 1], None), (good, [[0, 0, 0, 1, 2, 2]]), (good, [[0, 0, 1, 1, 2]]),
                          (good[:5], None)):
        with pytest.raises(ValueError):
            groups.dispersion_host(D, labels, perms)
    res = groups.dispersion_host(D, good, None)
    assert res.permutations == 0 and res.p_value[0] == 1.0 and res.n_ge[0] == 0
    # the group tests' methods are what they were
    assert groups.METHODS == {"permanova": 0, "anosim": 1}
    for name in ("permdisp", "dispersion", "mantel", 2):
        with pytest.raises(ValueError):
            groups.method_code(name)


# ---------------------------------------------------------------------------
# the host function at every size
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", gc.SIZES + (129, 200))
def test_host_function_has_the_oracle_bits(n):
    Ds = gc.matrices(n)
    for gname, labels in gc.groupings(n).items():
        perms = gc.perm_rows(labels, 12 if n > 64 else 40, seed=n)
        want = do.batch(Ds, labels, perms)
        for threads in (1, 3):
            res = groups.dispersion_host(Ds, labels, perms, perm_stats=True, threads=threads)
            assert _same(_host_tuple(res), want), (n, gname)
        assert (res.sample_size, res.n_groups, res.permutations) == (n, labels.max() + 1, len(perms))
        assert np.array_equal(res.p_value, (1.0 + want[1]) / (1.0 + len(perms)))
        assert res.group_means.shape == (len(Ds), labels.max() + 1)
        assert np.array_equal(res.group_means[:, 1], res.distances[:, labels == 1].mean(axis=1))
    one = groups.dispersion_host(Ds[0], labels, perms).first()   # a 2-D matrix is one replicate
    assert one.statistic == want[0][0] and one.n_ge == want[1][0] and one.perm_statistics is None
    assert one.distances.shape == (n,) and one.group_means.shape == (labels.max() + 1,)
