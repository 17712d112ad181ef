"""The Mantel test's specification (tests/mantel_oracle.py) against scipy's
correlations of the permuted upper triangles, and the host route
rna_clique_amd.mantel.mantel_host against the oracle's bits. No GPU."""

import numpy as np
import pytest
from scipy.stats import pearsonr, rankdata, spearmanr

import group_cases as gc
import group_oracle as go
import mantel_oracle as mo
import nj_cases
from rna_clique_amd import mantel

U = 2.0 ** -53
HOST_SIZES = (3, 4, 5, 8, 33, 65)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y)
               for x, y in zip(a, b))


def _host_tuple(res):
    return (res.statistic, res.n_ge, res.n_le, res.n_abs_ge, res.perm_statistics, res.valid)


def _others(n):
    """Matrices to correlate with: a noisy additive one of another tree, one with tied integer distances."""
    return {"noisy": go.mirrored(nj_cases.noisy_additive(n, 500 + n)[0]),
            "integer": go.mirrored(nj_cases.additive(n, 700 + n, integer=True)[0])}


def _upper(D, p=None):
    n = len(D)
    A = go.mirrored(D)
    if p is not None:
        A = A[np.ix_(p, p)]
    return A[np.triu_indices(n, 1)]


@pytest.mark.parametrize("n", HOST_SIZES)
def test_pearson_oracle_matches_scipy(n):
    """C, sxx and syy are sums of products of centred values. A centred value
    carries one rounding and the error of the mean, a constant shift whose
    first-order effect on all three sums vanishes because the other factor sums
    to zero. A product adds U; the sum of N terms and at most 7 halvings
    (N + 6) U: (N + 8) U of the sum of |xc yc|, which is at most sqrt(sxx syy)
    (Cauchy-Schwarz), so (N + 8) U absolute in r. The square root carries half
    of sxx's and syy's (N + 8) U each, and a product, a root and a division
    3 U more, say 4: (2 N + 20) U for the oracle. scipy sums M terms pairwise, no worse
    than that: (4 N + 40) U between the two."""
    bound = (4 * n + 40) * U
    perms = mo.perm_rows(n, 12, seed=n)
    worst = 0.0
    for name, X in zip(gc.NAMES, gc.matrices(n)):
        for yname, Y in _others(n).items():
            r, n_ge, n_le, n_abs, pr, valid = mo.pearson(X, Y, perms)
            if name == "equal":
                assert np.isnan(r) and np.isnan(pr).all() and (n_ge, n_le, n_abs, valid) == (0, 0, 0, 1)
                continue
            assert valid == 1 and _bits(pr[0]) == _bits(r) and n_ge >= 1 and n_le >= 1 and n_abs >= 1
            for k, p in enumerate(perms):
                want = pearsonr(_upper(X, p), _upper(Y)).statistic
                worst = max(worst, abs(pr[k] - want))
                assert abs(pr[k] - want) <= bound, (n, name, yname, k)
            assert n_ge == int((pr >= r).sum()) and n_le == int((pr <= r).sum())
            assert n_abs == int((np.abs(pr) >= abs(r)).sum())
    print(f"n={n}: pearson off by at most {worst:.2e} of a bound of {bound:.2e}")


@pytest.mark.parametrize("n", HOST_SIZES)
def test_spearman_oracle_is_exact_on_the_integers(n):
    """The integer sums against scipy's average ranks (doubled: integers, exact
    in float64 at these sizes), r against scipy.stats.spearmanr within the
    rounding of one expression on each side: the integers below 2^53 convert
    exactly, a product, a root and a division 3 U relative, |r| <= 1;
    spearmanr's own correlation of M ranks (4 N + 40) U as above."""
    M = n * (n - 1) // 2
    perms = mo.perm_rows(n, 12, seed=n + 1)
    iu = np.triu_indices(n, 1)
    for name, X in zip(gc.NAMES, gc.matrices(n)):
        for yname, Y in _others(n).items():
            m, sa, sb, saa, sbb, sab = mo.spearman_sums(X, Y, perms)
            ry = 2 * rankdata(_upper(Y), method="average")
            assert m == M and sa == sb == M * (M + 1) and sbb == int((ry * ry).sum())
            for k, p in enumerate(np.concatenate([np.arange(n)[None], perms])):
                rx = 2 * rankdata(_upper(X, p), method="average")
                assert sab[k] == int((rx * ry).sum()) and saa == int((rx * rx).sum())
            r, n_ge, n_le, n_abs, pr, valid = mo.spearman(X, Y, perms)
            if name == "equal":
                assert np.isnan(r) and np.isnan(pr).all() and (n_ge, n_le, n_abs, valid) == (0, 0, 0, 1)
                continue
            num = M * sab - sa * sb
            assert n_ge == int((num[1:] >= num[0]).sum()) and n_abs == int((abs(num[1:]) >= abs(num[0])).sum())
            assert valid == 1 and _bits(pr[0]) == _bits(r) and n_ge >= 1 and n_le >= 1 and n_abs >= 1
            for k in (0, 5, 11):
                want = spearmanr(_upper(X, perms[k]), _upper(Y)).statistic
                assert abs(pr[k] - want) <= (4 * n + 44) * U, (n, name, yname, k)
            assert a_tie_exists(Y) == (yname == "integer") or n == 3


def a_tie_exists(D):
    d = _upper(D)
    return len(np.unique(d)) < len(d)


def test_three_samples_and_constant_matrices():
    n = 3
    X = go.mirrored(np.array([[0, 1.0, 2.0], [0, 0, 4.0], [0, 0, 0]]))
    Y = go.mirrored(np.array([[0, 2.0, 3.0], [0, 0, 9.0], [0, 0, 0]]))
    perms = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0], [1, 2, 0]], dtype=np.int32)
    for method in mo.METHODS:
        want = mo.TESTS[method](X, Y, perms)
        assert want[5] == 1 and want[1] >= 1 and _bits(want[4][0]) == _bits(want[0])
        assert _same(_host_tuple(mantel.mantel_host(X, Y, perms, method, perm_stats=True)), mo.batch(X[None], Y, perms, method))
        assert mo.TESTS[method](X, X, perms)[0] == 1.0 and mo.TESTS[method](Y, Y, perms)[0] == 1.0
        for A, B in ((nj_cases.all_equal(n), Y), (X, nj_cases.all_equal(n, 0.1)), (np.full((n, n), 0.1), np.full((n, n), 0.3))):
            r, n_ge, n_le, n_abs, pr, valid = mo.TESTS[method](A, B, perms)
            assert np.isnan(r) and np.isnan(pr).all() and (n_ge, n_le, n_abs, valid) == (0, 0, 0, 1)
            res = mantel.mantel_host(A, B, perms, method, perm_stats=True)
            assert _same(_host_tuple(res), mo.batch(A[None], B, perms, method))
            assert np.isnan(res.p_value("two-sided")).all()
    for D in gc.matrices(33)[[0, 1, 3, 5]]:   # a matrix against itself: sqrt(s * s) is s, r is exactly 1
        assert mo.pearson(D, D)[0] == 1.0 and mo.spearman(D, D)[0] == 1.0


@pytest.mark.parametrize("method", mo.METHODS)
@pytest.mark.parametrize("n", (3, 4, 8, 33, 64, 65, 128, 129, 150))
def test_host_function_has_the_oracle_bits(n, method):
    Xs = gc.with_nan(gc.matrices(n))
    Y = _others(n)["integer" if method == "spearman" else "noisy"]
    perms = mo.perm_rows(n, 10 if n > 64 else 40, seed=n)
    want = mo.batch(Xs, Y, perms, method)
    for threads in (1, 3):
        res = mantel.mantel_host(Xs, Y, perms, method, perm_stats=True, threads=threads)
        assert _same(_host_tuple(res), want)
    assert res.valid.tolist() == [1, 1, 0, 1, 1, 1] and np.isnan(res.statistic[2]) and np.isnan(res.statistic[1 + 1])
    assert (res.n, res.permutations, res.method) == (n, len(perms), method)
    ok = ~np.isnan(res.statistic)
    for alt, count in (("greater", res.n_ge), ("less", res.n_le), ("two-sided", res.n_abs_ge)):
        p = res.p_value(alt)
        assert np.array_equal(p[ok], (1.0 + count[ok]) / (1.0 + len(perms))) and np.isnan(p[~ok]).all()
    one = mantel.mantel_host(Xs[0], Y, perms, method).first()
    assert one.statistic == want[0][0] and one.n_abs_ge == want[3][0] and one.perm_statistics is None
    assert one.p_value() == (1 + want[3][0]) / (1 + len(perms))
    none = mantel.mantel_host(Xs[0], Y, None, method)
    assert none.permutations == 0 and none.p_value("greater")[0] == 1.0 and _bits(none.statistic[0]) == _bits(want[0][0])


def test_permutations_and_rejected_arguments():
    a = mantel.permutations(7, 50, seed=3)
    assert a.shape == (50, 7) and a.dtype == np.int32
    assert np.array_equal(np.sort(a, axis=1), np.tile(np.arange(7), (50, 1)))
    assert len({row.tobytes() for row in a}) > 40
    assert np.array_equal(a, mantel.permutations(7, 50, seed=3))
    assert not np.array_equal(a, mantel.permutations(7, 50, seed=4))
    assert mantel.permutations(7, 0).shape == (0, 7)
    X = gc.matrices(6)[0]
    Y = _others(6)["noisy"]
    bad = np.array(Y)
    bad[0, 5] = np.inf
    for args in ((X[:2, :2], Y[:2, :2]), (X, bad), (X, Y[:5, :5]), (X, Y, [[0, 1, 2, 3, 4, 4]]),
                 (X, Y, [[0, 1, 2, 3, 4, 6]]), (X, Y, [[0, 1, 2, 3, 4]]), (X, Y, None, "kendall")):
        with pytest.raises(ValueError):
            mantel.mantel_host(*args)
    bad = np.array(Y)
    bad[5, 0] = np.nan                                          # below the diagonal: not read
    assert mantel.mantel_host(X, bad, None).statistic[0] == mantel.mantel_host(X, Y, None).statistic[0]
    with pytest.raises(ValueError):
        mantel.mantel_host(X, Y, None).p_value("both")


def test_label_alignment():
    """What SampleSimilarity.mantel does with the other matrix's labels."""
    import pandas as pd
    samples = ["s0", "s1", "s2", "s3"]
    Y = _others(4)["noisy"]
    df = pd.DataFrame(Y, index=samples, columns=samples)
    common, pos, mat = mantel.align_matrix(samples, df)
    assert common == samples and pos == [0, 1, 2, 3] and np.array_equal(mat, Y)
    # the other matrix in another order: realigned to the samples' order
    o = [2, 0, 3, 1]
    shuffled = df.iloc[o, o]
    for other in (shuffled, (list(shuffled.index), shuffled.to_numpy())):
        common, pos, mat = mantel.align_matrix(samples, other)
        assert common == samples and pos == [0, 1, 2, 3] and np.array_equal(mat, Y)
    # a sample missing on one side or the other
    fewer = df.iloc[[3, 0, 1], [3, 0, 1]]
    more = pd.DataFrame(_others(5)["noisy"], index=samples + ["s9"], columns=samples + ["s9"])
    for other in (fewer, more):
        with pytest.raises(ValueError):
            mantel.align_matrix(samples, other)
    common, pos, mat = mantel.align_matrix(samples, fewer, strict=False)
    assert common == ["s0", "s1", "s3"] and pos == [0, 1, 3] and np.array_equal(mat, Y[np.ix_(pos, pos)])
    common, pos, mat = mantel.align_matrix(samples, more, strict=False)
    assert common == samples and np.array_equal(mat, more.to_numpy()[:4, :4])
    with pytest.raises(ValueError):
        mantel.align_matrix(samples, df.iloc[:2, :2], strict=False)          # fewer than 3 in common
    with pytest.raises(ValueError):
        mantel.align_matrix(samples, pd.DataFrame(Y, index=samples, columns=samples[::-1]))
    with pytest.raises(ValueError):
        mantel.align_matrix(samples, (["s0", "s0", "s1", "s2"], Y))
    with pytest.raises(ValueError):
        mantel.align_matrix(samples, (samples, Y[:3]))
