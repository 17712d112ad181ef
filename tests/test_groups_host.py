"""The group tests' specification (tests/group_oracle.py) against a second,
plain statement of PERMANOVA and ANOSIM, its partition invariance, and the host
route rna_clique_amd.groups.group_test_host against the oracle's bits. No GPU."""

import numpy as np
import pytest
from scipy.stats import rankdata

import group_cases as gc
import group_oracle as go
from rna_clique_amd import groups

HOST_SIZES = (3, 4, 5, 8, 31, 33, 64, 65)
METHODS = ("permanova", "anosim")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Two oracle-style tuples agree: floats as bits, the rest exactly."""
    return all(np.array_equal(_bits(x), _bits(y)) if np.asarray(x).dtype.kind == "f" else np.array_equal(x, y)
               for x, y in zip(a, b))


def _host_tuple(res):
    return (res.statistic, res.n_ge, res.total, res.within, res.perm_statistics, res.valid)


# ---------------------------------------------------------------------------
# the plain statements
# ---------------------------------------------------------------------------

def plain_permanova(D, labels):
    """(F, SS_T, SS_A) group by group with boolean masks."""
    n = len(D)
    iu = np.triu_indices(n, 1)
    v = (D * D)
    sst = v[iu].sum() / n
    ssw = 0.0
    for g in np.unique(labels):
        m = labels == g
        sub = v[np.ix_(m, m)]
        ssw += sub[np.triu_indices(m.sum(), 1)].sum() / m.sum()
    a = len(np.unique(labels))
    ssa = sst - ssw
    with np.errstate(all="ignore"):
        return (ssa / (a - 1)) / (ssw / (n - a)), sst, ssa


def plain_w2(D, labels):
    """Twice the sum of scipy's average ranks over the within-group pairs."""
    n = len(D)
    iu = np.triu_indices(n, 1)
    ranks = rankdata(D[iu], method="average")
    within = (labels[:, None] == labels[None, :])[iu]
    w2 = 2.0 * ranks[within].sum()
    assert w2 == int(w2)
    return int(w2)


def _clean(D):
    """The matrix as the tests read it: the part above the diagonal, mirrored."""
    return go.mirrored(D)


# ---------------------------------------------------------------------------
# oracle against the plain statements
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", HOST_SIZES)
def test_permanova_oracle_matches_the_plain_statement(n):
    """Each implementation squares (1 rounding, u = 2^-53), adds at most M
    non-negative terms ((M - 1) u) and divides by 2 n_g (2 u): SS_T and SS_W
    carry (M + 2) u each, relative. SS_A = SS_T - SS_W then carries (2 M + 5) u
    SS_T, and F -- three more divisions and SS_W's own error -- at most
    (2 M + 5) u SS_T / |SS_A| + (M + 5) u <= (3 M + 10) u SS_T / |SS_A|, as
    SS_T >= |SS_A|. Two implementations: (3 M + 10) 2^-52 SS_T / |SS_A|, and
    3 M + 10 <= 7 M for M >= 3 pairs, the smallest design. The multiple is 7."""
    M = n * (n - 1) // 2
    for name, D in zip(gc.NAMES, gc.matrices(n)):
        D = _clean(D)
        for gname, labels in gc.groupings(n).items():
            perms = gc.perm_rows(labels, 20, seed=n)
            F, n_ge, sst, ssw, pF, valid = go.permanova(D, labels, perms)
            assert valid == 1 and np.array_equal(_bits(pF[0]), _bits(F)) and n_ge >= 1
            want, p_sst, p_ssa = plain_permanova(D, labels)
            assert abs(sst - p_sst) <= (M + 2) * 2.0 ** -52 * p_sst
            if p_ssa == 0 or not np.isfinite(want):
                continue
            bound = 7 * M * 2.0 ** -52 * p_sst / abs(p_ssa)
            err = abs(F - want) / abs(want)
            print(f"n={n} {name} {gname}: F {F:.6g}, off by {err:.2e} of a bound of {bound:.2e}")
            assert err <= bound
            for k in (1, 7, 19):
                wk = plain_permanova(D, perms[k])
                if wk[2] != 0 and np.isfinite(wk[0]):
                    assert abs(pF[k] - wk[0]) <= 7 * M * 2.0 ** -52 * wk[1] / abs(wk[2]) * abs(wk[0])


@pytest.mark.parametrize("n", HOST_SIZES)
def test_anosim_oracle_matches_scipy_ranks_exactly(n):
    M = n * (n - 1) // 2
    for name, D in zip(gc.NAMES, gc.matrices(n)):
        D = _clean(D)
        iu = np.triu_indices(n, 1)
        assert np.array_equal(go.twice_ranks(D)[iu], (2 * rankdata(D[iu], method="average")).astype(np.int64))
        for labels in gc.groupings(n).values():
            perms = gc.perm_rows(labels, 40, seed=n)
            R, n_ge, total, w2, pR, valid = go.anosim(D, labels, perms)
            sizes = np.bincount(labels)
            mw = int((sizes * (sizes - 1) // 2).sum())
            want = plain_w2(D, labels)
            wperm = np.array([plain_w2(D, row) for row in perms])
            assert valid == 1 and w2 == want and total == M * (M + 1)
            assert n_ge == int((wperm <= want).sum()) >= 1
            # R as the textbook writes it, from mean ranks
            rw, rb = want / 2 / mw, (M * (M + 1) - want) / 2 / (M - mw)
            assert abs(R - (rb - rw) / (M / 2)) <= 8 * 2.0 ** -52
            assert np.array_equal(_bits(pR), _bits(go.anosim_r(wperm, M, mw)))
            # strictly decreasing in W2: counting on the integers is counting on R
            assert int((pR >= R).sum()) == n_ge


# ---------------------------------------------------------------------------
# partition invariance, small designs, degenerate inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", HOST_SIZES)
def test_the_same_partition_gives_the_same_bits(n, method):
    """Groups renumbered (labels and permutations alike): identical statistics
    and counts. Rearrangements that describe the observed partition among the
    permutations: each has the observed statistic's bits and is counted."""
    Ds = gc.matrices(n)
    for labels in gc.groupings(n).values():
        perms = gc.perm_rows(labels, 30, seed=n + 1)
        want = go.batch(Ds, labels, perms, method)
        host = groups.group_test_host(Ds, labels, perms, method, perm_stats=True)
        assert _same(_host_tuple(host), want)
        for m in gc.renumberings(labels, seed=n):
            assert _same(go.batch(Ds, m[labels], m[perms], method), want)
            assert _same(_host_tuple(groups.group_test_host(Ds, m[labels], m[perms], method, perm_stats=True)), want)
        rows = gc.same_partition_rows(labels, seed=n)
        stat, n_ge, _, _, ps, _ = go.batch(Ds, labels, rows, method)
        assert np.array_equal(_bits(ps), _bits(np.repeat(stat[:, None], len(rows), axis=1)))
        ok = ~np.isnan(stat)
        assert np.array_equal(n_ge[ok], np.full(ok.sum(), len(rows)))


@pytest.mark.parametrize("method", METHODS)
def test_six_samples_in_two_groups_of_three(method):
    assert len(gc.six_sample_partitions()) == 10
    labels = np.array([0, 1, 0, 1, 1, 0], dtype=np.int32)
    perms = gc.perm_rows(labels, 200, seed=6)
    for D in gc.matrices(6):
        want = gc.six_sample_expected(D, labels, perms, method)
        assert want >= 1 or np.isnan(go.TESTS[method](D, labels)[0])
        assert go.TESTS[method](D, labels, perms)[1] == want
        res = groups.group_test_host(D, labels, perms, method)
        assert int(res.n_ge[0]) == want and res.p_value[0] == (1 + want) / 201


def test_degenerate_matrices():
    for n in (5, 8, 33):
        for labels in gc.groupings(n).values():
            P = 25
            perms = gc.perm_rows(labels, P, seed=n)
            for fn in (lambda D, m: go.TESTS[m](D, labels, perms)[:2],
                       lambda D, m: (lambda r: (r.statistic[0], int(r.n_ge[0])))(
                           groups.group_test_host(D, labels, perms, m))):
                # all distances equal: every rank is the same, R = 0 for every labelling
                R, n_ge = fn(gc.nj_cases.all_equal(n), "anosim")
                assert R == 0.0 and n_ge == P
                # no distances at all: 0 / 0
                F, n_ge = fn(np.zeros((n, n)), "permanova")
                assert np.isnan(F) and n_ge == 0
            res = groups.group_test_host(gc.nj_cases.all_equal(n), labels, perms, "anosim")
            assert res.p_value[0] == 1.0
            res = groups.group_test_host(np.zeros((n, n)), labels, perms, "permanova")
            assert res.p_value[0] == 1 / (1 + P) and res.valid[0] == 1


@pytest.mark.parametrize("method", METHODS)
def test_invalid_matrix_leaves_the_others_alone(method):
    n = 8
    labels = gc.groupings(n)["singleton"]
    perms = gc.perm_rows(labels, 10)
    Ds = gc.matrices(n)
    clean = groups.group_test_host(Ds, labels, perms, method, perm_stats=True)
    for poison in (np.nan, np.inf, -np.inf):
        bad = gc.with_nan(Ds)
        bad[2, 0, n - 1] = poison
        res = groups.group_test_host(bad, labels, perms, method, perm_stats=True)
        assert _same(_host_tuple(res), go.batch(bad, labels, perms, method))
        assert res.valid.tolist() == [1, 1, 0, 1, 1, 1] and res.n_ge[2] == 0
        assert np.isnan([res.statistic[2], res.total[2], res.within[2], res.p_value[2]]).all()
        assert np.isnan(res.perm_statistics[2]).all()
        keep = [0, 1, 3, 4, 5]
        assert _same([x[keep] for x in _host_tuple(res)], [x[keep] for x in _host_tuple(clean)])


def test_rejected_arguments():
    D = gc.matrices(6)[0]
    good = np.array([0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError):
        groups.group_test_host(D, np.arange(6), None)                 # singletons only: a == N
    with pytest.raises(ValueError):
        groups.group_test_host(D, np.zeros(6, dtype=int), None)       # one group
    with pytest.raises(ValueError):
        groups.group_test_host(D, [0, 0, 2, 2, 3, 3], None)           # group 1 is empty
    with pytest.raises(ValueError):
        groups.group_test_host(D, [0, 0, -1, 1, 1, 1], None)
    with pytest.raises(ValueError):
        groups.group_test_host(D, good, [[0, 0, 0, 1, 2, 2]])         # not a rearrangement
    with pytest.raises(ValueError):
        groups.group_test_host(D, good, [[0, 0, 1, 1, 2, 3]])
    with pytest.raises(ValueError):
        groups.group_test_host(D, good, [[0, 0, 1, 1, 2]])
    with pytest.raises(ValueError):
        groups.group_test_host(D, good[:5], None)
    with pytest.raises(ValueError):
        groups.group_test_host(D, good, None, "mantel")
    res = groups.group_test_host(D, good, None)                       # no permutations: statistics only
    assert res.permutations == 0 and res.p_value[0] == 1.0 and res.n_ge[0] == 0


# ---------------------------------------------------------------------------
# the host function at every size
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", (3, 4, 8, 32, 63, 64, 65, 127, 128, 129, 200))
def test_host_function_has_the_oracle_bits(n, method):
    Ds = gc.matrices(n)[[0, 1, 2, 4]]
    gs = gc.groupings(n)
    for gname in ("balanced", "singleton" if n >= 4 else "one_pair"):
        labels = gs[gname]
        perms = gc.perm_rows(labels, 12 if n > 64 else 40, seed=n)
        want = go.batch(Ds, labels, perms, method)
        for threads in (1, 3):
            res = groups.group_test_host(Ds, labels, perms, method, perm_stats=True, threads=threads)
            assert _same(_host_tuple(res), want)
        assert (res.sample_size, res.n_groups, res.permutations) == (n, labels.max() + 1, len(perms))
        assert np.array_equal(res.p_value, (1.0 + want[1]) / (1.0 + len(perms)))
        if method == "permanova":
            assert np.array_equal(_bits(res.r2), _bits((want[2] - want[3]) / want[2]))
        else:
            assert res.r2 is None
    one = groups.group_test_host(Ds[0], labels, perms, method).first()   # a 2-D matrix is one replicate
    assert one.statistic == want[0][0] and one.n_ge == want[1][0] and one.perm_statistics is None


# ---------------------------------------------------------------------------
# labels
# ---------------------------------------------------------------------------

def test_encode_grouping():
    import pandas as pd
    samples = ["s3", "s1", "s2", "s0"]
    mapping = {"s0": "b", "s1": "a", "s2": "b", "s3": "c", "extra": "z"}
    labels, names = groups.encode_grouping(samples, mapping)
    assert labels.dtype == np.int32 and labels.tolist() == [0, 1, 2, 2] and names == ["c", "a", "b"]
    for other in (pd.Series(mapping), ["c", "a", "b", "b"], np.array(["c", "a", "b", "b"])):
        l2, n2 = groups.encode_grouping(samples, other)
        assert l2.tolist() == labels.tolist() and list(n2) == names
    with pytest.raises(KeyError):
        groups.encode_grouping(samples + ["s9"], mapping)
    with pytest.raises(ValueError):
        groups.encode_grouping(samples, ["a", "b"])


def test_permuted_labels_are_rearrangements_fixed_by_the_seed():
    labels = np.array([0, 0, 1, 2, 2, 2, 1], dtype=np.int32)
    a = groups.permuted_labels(labels, 50, seed=3)
    assert a.shape == (50, 7) and a.dtype == np.int32
    assert np.array_equal(np.sort(a, axis=1), np.tile(np.sort(labels), (50, 1)))
    assert len({row.tobytes() for row in a}) > 25
    assert np.array_equal(a, groups.permuted_labels(labels, 50, seed=3))
    assert not np.array_equal(a, groups.permuted_labels(labels, 50, seed=4))
    assert groups.permuted_labels(labels, 0).shape == (0, 7)
    groups.check_design(labels, a)
