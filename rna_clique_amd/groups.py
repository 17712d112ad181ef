"""Group tests on distance matrices: PERMANOVA (Anderson 2001, pseudo-F) and
ANOSIM (Clarke 1993, R) with label permutations -- what
skbio.stats.distance.permanova / anosim answer for one matrix, here for a
batch of replicate matrices at once: the result type the GPU calls fill
(Engine.group_test, Engine.resample_group_test, SampleSimilarity.permanova /
anosim / bootstrap_group_test / pairwise_group_tests), the label handling, and
a host route in numpy for matrices beyond the GPU's 128 samples
(group_test_host).

The definitions and the operation order are those of include/rcgpu.h
(rc_group_test) and DESIGN.md section 2. The p-value follows scikit-bio:
(1 + permutations whose statistic is >= the observed one) / (1 + permutations).
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

MAX_GPU_SAMPLES = 128   # rc_group_test: the matrix lives in LDS
GPU_PERM_CHUNK = 120    # permutations one workgroup walks (groups.hip: GROUP_PERM_CHUNK)
METHODS = {"permanova": 0, "anosim": 1}   # RC_GROUP_PERMANOVA, RC_GROUP_ANOSIM


def method_code(method) -> int:
    try:
        return METHODS[method]
    except (KeyError, TypeError):
        raise ValueError(f"method must be one of {sorted(METHODS)}, not {method!r}") from None


@dataclass
class GroupTestResult:
    """One group test per replicate matrix, arrays of length R (first(): the
    same with scalars, for a single matrix).

    statistic        F (permanova) or R (anosim); NaN for an invalid matrix
    p_value          (1 + n_ge) / (1 + permutations); NaN for an invalid matrix
    n_ge             permutations whose statistic is >= the observed one
    total, within    SS_T and SS_W (permanova); M (M + 1) and W2, the sum of
                     the within-group twice-ranks (anosim)
    r2               (SS_T - SS_W) / SS_T, permanova only (else None)
    valid            0 for a matrix with a non-finite entry above its diagonal
    perm_statistics  (R, permutations) when asked for, else None
    """
    method: str
    statistic: np.ndarray
    p_value: np.ndarray
    permutations: int
    sample_size: int
    n_groups: int
    n_ge: np.ndarray
    total: np.ndarray
    within: np.ndarray
    valid: np.ndarray
    r2: np.ndarray | None = None
    perm_statistics: np.ndarray | None = None

    @classmethod
    def from_counts(cls, method, n, n_groups, permutations, stat, n_ge, total, within, valid, perm_stat=None):
        stat, total, within = (np.asarray(x, dtype=np.float64) for x in (stat, total, within))
        valid = np.asarray(valid, dtype=np.uint8)
        n_ge = np.asarray(n_ge, dtype=np.uint32)
        p = np.where(valid != 0, (1.0 + n_ge) / (1.0 + permutations), np.nan)
        r2 = None
        if method == "permanova":
            with np.errstate(invalid="ignore", divide="ignore"):
                r2 = (total - within) / total
        return cls(method, stat, p, int(permutations), int(n), int(n_groups), n_ge, total, within, valid, r2, perm_stat)

    def __len__(self):
        return len(self.valid)

    def first(self):
        """The result of replicate 0 with scalar fields."""
        pick = lambda a: None if a is None else a[0]   # noqa: E731
        return GroupTestResult(self.method, float(self.statistic[0]), float(self.p_value[0]), self.permutations,
                               self.sample_size, self.n_groups, int(self.n_ge[0]), float(self.total[0]),
                               float(self.within[0]), int(self.valid[0]),
                               None if self.r2 is None else float(self.r2[0]), pick(self.perm_statistics))


# ---------------------------------------------------------------------------
# labels
# ---------------------------------------------------------------------------

def encode_grouping(samples, grouping):
    """(labels int32 (N,), group names) for `samples`: `grouping` is a mapping
    from sample label to group, a pandas Series indexed by sample, or a
    sequence in `samples` order. Groups are numbered by first occurrence in
    `samples`."""
    samples = list(samples)
    if hasattr(grouping, "index") and hasattr(grouping, "loc"):   # pandas Series
        missing = [s for s in samples if s not in grouping.index]
        if missing:
            raise KeyError(f"samples without a group: {missing}")
        values = [grouping.loc[s] for s in samples]
    elif hasattr(grouping, "keys"):
        missing = [s for s in samples if s not in grouping]
        if missing:
            raise KeyError(f"samples without a group: {missing}")
        values = [grouping[s] for s in samples]
    else:
        values = list(grouping)
        if len(values) != len(samples):
            raise ValueError("grouping must hold one group per sample")
    names, number = [], {}
    labels = np.zeros(len(samples), dtype=np.int32)
    for i, v in enumerate(values):
        if v not in number:
            number[v] = len(names)
            names.append(v)
        labels[i] = number[v]
    return labels, names


def permuted_labels(labels, permutations, seed=0):
    """`permutations` rearrangements of `labels` as an int32 (P, N) array, drawn
    from numpy.random.default_rng(seed): deterministic for a seed. The same
    rows serve every replicate matrix of a batched call, so the replicates'
    statistics are compared under one set of permutations."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 1:
        raise ValueError("labels must be one-dimensional")
    p = int(permutations)
    if p < 0:
        raise ValueError("permutations must be >= 0")
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.permuted(np.tile(lab, (p, 1)), axis=1), dtype=np.int32).reshape(p, len(lab))


def check_design(labels, perm_labels=None):
    """(labels int32 (N,), perm_labels int32 (P, N), group sizes) after the
    checks rc_group_test makes: labels 0..a-1 with no group empty, 2 <= a < N,
    every row of perm_labels a rearrangement of labels. ValueError otherwise."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if lab.ndim != 1:
        raise ValueError("labels must be one-dimensional")
    n = len(lab)
    if n == 0 or lab.min() < 0:
        raise ValueError("labels must be group numbers 0..a-1")
    sizes = np.bincount(lab)
    a = len(sizes)
    if (sizes == 0).any():
        raise ValueError("an empty group")
    if a < 2 or a >= n:
        raise ValueError("a group test needs at least 2 groups and fewer groups than samples")
    if perm_labels is None:
        perms = np.zeros((0, n), dtype=np.int32)
    else:
        perms = np.ascontiguousarray(perm_labels, dtype=np.int32)
        if perms.size == 0:
            perms = perms.reshape(0, n)
        if perms.ndim != 2 or perms.shape[1] != n:
            raise ValueError("perm_labels must have shape (permutations, N)")
        if perms.size and not np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.sort(lab), perms.shape)):
            raise ValueError("a row of perm_labels is not a rearrangement of labels")
    return lab, perms, sizes


# ---------------------------------------------------------------------------
# the host route
# ---------------------------------------------------------------------------

def _halving_sum(x):
    """Sum along the last axis: padded with zeros to a power of two, then
    x[..., :h] + x[..., h:2h] until one column is left."""
    n = x.shape[-1]
    w = 1
    while w < n:
        w *= 2
    y = np.zeros(x.shape[:-1] + (w,), dtype=x.dtype)
    y[..., :n] = x
    while w > 1:
        w //= 2
        y = y[..., :w] + y[..., w:2 * w]
    return y[..., 0]


def _permanova_sums(V, G, div):
    """S of every row of G (K, N) on the squared distances V (N, N): t[k, i]
    grows over j ascending by V[j, i] where G[k, j] == G[k, i]."""
    K, n = G.shape
    out = np.zeros(K, dtype=np.float64)
    step = max(1, (1 << 23) // (n * n))   # rows of G per block: masks of about 8 MB
    for k0 in range(0, K, step):
        g = G[k0:k0 + step]
        t = np.zeros(g.shape, dtype=np.float64)
        for j in range(n):
            np.add(t, V[j], out=t, where=g[:, j:j + 1] == g)
        out[k0:k0 + step] = _halving_sum(t / div[k0:k0 + step])
    return out


def _twice_ranks(d):
    """2 * (average rank) of every entry of d: 2 #{less} + #{equal} + 1."""
    s = np.sort(d)
    return np.searchsorted(s, d, "left") + np.searchsorted(s, d, "right") + 1


def _one_host(D, G, div, sizes, anosim):
    """(stat, n_ge, total, within, perm_stat, valid) of one matrix; G: row 0 one
    group of everything, row 1 the observed labels, then the permutations."""
    n = D.shape[0]
    P = len(G) - 2
    iu = np.triu_indices(n, 1)
    d = D[iu]
    nan = np.float64(np.nan)
    if not np.isfinite(d).all():
        return nan, 0, nan, nan, np.full(P, nan), 0
    a = len(sizes)
    with np.errstate(all="ignore"):
        if anosim:
            M = n * (n - 1) // 2
            mw = int((sizes * (sizes - 1) // 2).sum())
            Rk = np.zeros((n, n), dtype=np.float64)
            Rk[iu] = _twice_ranks(d)
            Rk = Rk + Rk.T
            w22 = np.zeros(len(G), dtype=np.float64)   # integers below 2^53: exact in any order
            for g in range(a):
                X = (G[1:] == g).astype(np.float64)
                w22[1:] += ((X @ Rk) * X).sum(axis=1)
            w2 = (w22[1:] / 2).astype(np.int64)
            allr = M * (M + 1)
            rw = w2.astype(np.float64) / np.float64(2 * mw)
            rb = (allr - w2).astype(np.float64) / np.float64(2 * (M - mw))
            stats = (rb - rw) / (np.float64(M) / 2.0)
            n_ge = int((w2[1:] <= w2[0]).sum())
            total, within = np.float64(allr), np.float64(w2[0])
        else:
            V = np.zeros((n, n), dtype=np.float64)
            V[iu] = d * d
            V = V + V.T
            S = _permanova_sums(V, G, div)
            sst, ssw = S[0], S[1:]
            stats = ((sst - ssw) / np.float64(a - 1)) / (ssw / np.float64(n - a))
            n_ge = int((stats[1:] >= stats[0]).sum())
            total, within = sst, ssw[0]
    return stats[0], n_ge, total, within, stats[1:], 1


def group_test_host(matrices, labels, perm_labels=None, method="permanova", *, perm_stats=False, threads=None):
    """The group test of distance matrices (R, N, N) or (N, N) in numpy, for any
    N: the same definitions and operation order as the GPU route
    (Engine.group_test), so the same bits. Returns GroupTestResult with one
    entry per matrix. `threads`: matrices tested at a time (default: up to 16,
    no more than the machine's CPUs)."""
    code = method_code(method)
    D = np.asarray(matrices, dtype=np.float64)
    if D.ndim == 2:
        D = D[None]
    if D.ndim != 3 or D.shape[1] != D.shape[2]:
        raise ValueError("matrices must have shape (replicates, N, N)")
    lab, perms, sizes = check_design(labels, perm_labels)
    n = len(lab)
    if D.shape[1] != n:
        raise ValueError("one label per sample")
    R, P = len(D), len(perms)
    G = np.concatenate([np.zeros((1, n), dtype=np.int32), lab[None], perms])
    div = 2.0 * sizes[G].astype(np.float64)
    div[0] = 2.0 * n
    if threads is None:
        threads = min(16, os.cpu_count() or 1)
    work = lambda r: _one_host(D[r], G, div, sizes, code == 1)   # noqa: E731
    if threads > 1 and R > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(threads, R)) as ex:
            rows = list(ex.map(work, range(R)))
    else:
        rows = [work(r) for r in range(R)]
    stat, n_ge, total, within, ps, valid = (list(c) for c in zip(*rows)) if rows else ([], [], [], [], [], [])
    pstat = np.array(ps, dtype=np.float64).reshape(R, P) if perm_stats else None
    return GroupTestResult.from_counts(method, n, len(sizes), P, stat, n_ge, total, within, valid, pstat)


# ---------------------------------------------------------------------------
# PERMDISP: are the groups equally spread?
# ---------------------------------------------------------------------------

GPU_DISP_PERM_CHUNK = 124   # permutations one workgroup walks (dispersion.hip: DISP_PERM_CHUNK)


@dataclass
class DispersionResult:
    """PERMDISP (Anderson 2006, centroid form) per replicate matrix, arrays of
    length R (first(): the same with scalars, for a single matrix). What
    skbio.stats.distance.permdisp(test="centroid") and vegan's betadisper
    answer: the one-way ANOVA F of the samples' distances to their group's
    centroid in the full principal-coordinate space, with the labels permuted.
    Read it beside PERMANOVA, which cannot tell location from spread.

    statistic        F; NaN for an invalid matrix
    p_value          (1 + n_ge) / (1 + permutations); NaN for an invalid matrix
    n_ge             permutations whose F is >= the observed one
    total, within    SS_T and SS_W of the distances
    distances        (R, N): the distance of every sample to its group's centroid
    group_means      (R, a): the mean distance in every group, in group order
    valid            0 for a matrix with a non-finite entry above its diagonal
    perm_statistics  (R, permutations) when asked for, else None
    """
    statistic: np.ndarray
    p_value: np.ndarray
    permutations: int
    sample_size: int
    n_groups: int
    n_ge: np.ndarray
    total: np.ndarray
    within: np.ndarray
    distances: np.ndarray
    group_means: np.ndarray
    valid: np.ndarray
    perm_statistics: np.ndarray | None = None

    @classmethod
    def from_counts(cls, labels, permutations, stat, n_ge, total, within, dist, valid, perm_stat=None):
        lab = np.asarray(labels, dtype=np.int64)
        n, a = len(lab), int(lab.max()) + 1
        stat, total, within = (np.asarray(x, dtype=np.float64) for x in (stat, total, within))
        dist = np.asarray(dist, dtype=np.float64).reshape(len(stat), n)
        valid = np.asarray(valid, dtype=np.uint8)
        n_ge = np.asarray(n_ge, dtype=np.uint32)
        p = np.where(valid != 0, (1.0 + n_ge) / (1.0 + permutations), np.nan)
        means = np.stack([dist[:, lab == g].mean(axis=1) for g in range(a)], axis=1)
        return cls(stat, p, int(permutations), n, a, n_ge, total, within, dist, means, valid, perm_stat)

    def __len__(self):
        return len(self.valid)

    def first(self):
        """The result of replicate 0: scalar fields, distances (N,), group_means (a,)."""
        return DispersionResult(float(self.statistic[0]), float(self.p_value[0]), self.permutations, self.sample_size,
                                self.n_groups, int(self.n_ge[0]), float(self.total[0]), float(self.within[0]),
                                self.distances[0], self.group_means[0], int(self.valid[0]),
                                None if self.perm_statistics is None else self.perm_statistics[0])


def _own_sums(G, X):
    """out[k, i] = the sum over j ascending of X[k, j] where G[k, j] == G[k, i]."""
    out = np.zeros(X.shape, dtype=np.float64)
    for j in range(G.shape[1]):
        np.add(out, X[:, j:j + 1], out=out, where=G[:, j:j + 1] == G)
    return out


def _dispersion_rows(V, G, ng, a):
    """(F, SS_T, SS_W, z) of every row of G (K, N) on the squared distances V;
    ng (K, N): the size of every sample's group."""
    K, n = G.shape
    F, sst, ssw, z = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros((K, n))
    step = max(1, (1 << 23) // (n * n))   # rows of G per block: masks of about 8 MB
    for k0 in range(0, K, step):
        g, m = G[k0:k0 + step], ng[k0:k0 + step]
        t = np.zeros(g.shape, dtype=np.float64)
        for j in range(n):
            np.add(t, V[j], out=t, where=g[:, j:j + 1] == g)
        zz = np.sqrt(np.abs(t / m - _own_sums(g, t) / (2.0 * m * m)))
        dw = zz - _own_sums(g, zz) / m
        w = _halving_sum(dw * dw)
        dt = zz - (_halving_sum(zz) / np.float64(n))[:, None]
        s = _halving_sum(dt * dt)
        F[k0:k0 + step] = ((s - w) / np.float64(a - 1)) / (w / np.float64(n - a))
        sst[k0:k0 + step], ssw[k0:k0 + step], z[k0:k0 + step] = s, w, zz
    return F, sst, ssw, z


def _squared(D):
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    V = np.zeros((n, n), dtype=np.float64)
    V[iu] = D[iu] * D[iu]
    return V + V.T


def centroid_distances(D, labels):
    """The distance of every sample of distance matrix D (N, N; the part above
    the diagonal is read) to the centroid of its group in the full
    principal-coordinate space, from the squared distances alone:
    sqrt(|t / n_g - b / (2 n_g^2)|), t the sum of the squared distances to the
    group's members, b the sum of t over them (include/rcgpu.h,
    rc_group_dispersion). A sample alone in its group is at distance 0. Unlike
    dispersion_host this takes any labelling, one group or singletons only
    included."""
    D = np.asarray(D, dtype=np.float64)
    lab = np.ascontiguousarray(labels, dtype=np.int64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or lab.shape != (D.shape[0],):
        raise ValueError("one square matrix and one label per sample")
    if len(lab) == 0 or lab.min() < 0:
        raise ValueError("labels must be group numbers 0..a-1")
    sizes = np.bincount(lab)
    G = lab[None]
    with np.errstate(all="ignore"):
        return _dispersion_rows(_squared(D), G, sizes[G].astype(np.float64), 2)[3][0]


def _one_dispersion(D, G, ng, a):
    """(stat, n_ge, total, within, perm_stat, valid, dist) of one matrix; G: row
    0 the observed labels, then the permutations."""
    n = D.shape[0]
    P = len(G) - 1
    nan = np.float64(np.nan)
    if not np.isfinite(D[np.triu_indices(n, 1)]).all():
        return nan, 0, nan, nan, np.full(P, nan), 0, np.full(n, nan)
    with np.errstate(all="ignore"):
        F, sst, ssw, z = _dispersion_rows(_squared(D), G, ng, a)
        n_ge = int((F[1:] >= F[0]).sum())
    return F[0], n_ge, sst[0], ssw[0], F[1:], 1, z[0]


def dispersion_host(matrices, labels, perm_labels=None, *, perm_stats=False, threads=None):
    """PERMDISP of distance matrices (R, N, N) or (N, N) in numpy, for any N:
    the same definitions and operation order as the GPU route
    (Engine.group_dispersion), so the same bits. Returns DispersionResult with
    one entry per matrix. `threads`: matrices tested at a time (default: up to
    16, no more than the machine's CPUs)."""
    D = np.asarray(matrices, dtype=np.float64)
    if D.ndim == 2:
        D = D[None]
    if D.ndim != 3 or D.shape[1] != D.shape[2]:
        raise ValueError("matrices must have shape (replicates, N, N)")
    lab, perms, sizes = check_design(labels, perm_labels)
    n = len(lab)
    if D.shape[1] != n:
        raise ValueError("one label per sample")
    R, P = len(D), len(perms)
    G = np.concatenate([lab[None], perms])
    ng = sizes[G].astype(np.float64)
    if threads is None:
        threads = min(16, os.cpu_count() or 1)
    work = lambda r: _one_dispersion(D[r], G, ng, len(sizes))   # noqa: E731
    if threads > 1 and R > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(threads, R)) as ex:
            rows = list(ex.map(work, range(R)))
    else:
        rows = [work(r) for r in range(R)]
    stat, n_ge, total, within, ps, valid, dist = (list(c) for c in zip(*rows)) if rows else ([],) * 7
    pstat = np.array(ps, dtype=np.float64).reshape(R, P) if perm_stats else None
    return DispersionResult.from_counts(lab, P, stat, n_ge, total, within, np.array(dist).reshape(R, n), valid, pstat)
