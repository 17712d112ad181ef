"""The Mantel test: the permutation correlation of distance matrices -- what
skbio.stats.distance.mantel answers for one pair of matrices, here for a batch
of replicate matrices X against one matrix Y at once: the result type the GPU
calls fill (Engine.mantel, Engine.resample_mantel, SampleSimilarity.mantel /
bootstrap_mantel), the permutations, and a host route in numpy for matrices
beyond the GPU's 128 samples (mantel_host).

The definitions and the operation order are those of include/rcgpu.h
(rc_mantel) and DESIGN.md section 2. The p-value follows scikit-bio:
(1 + permutations at least as extreme as the observed r) / (1 + permutations),
"at least as extreme" by the alternative. Not included: the partial Mantel test.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from .groups import _halving_sum, _twice_ranks

MAX_GPU_SAMPLES = 128        # rc_mantel: the matrix lives in LDS
GPU_PERM_CHUNK = 124         # permutations one workgroup walks (mantel.hip: MANTEL_PERM_CHUNK)
METHODS = {"pearson": 0, "spearman": 1}   # RC_MANTEL_PEARSON, RC_MANTEL_SPEARMAN
ALTERNATIVES = ("two-sided", "greater", "less")


def method_code(method) -> int:
    try:
        return METHODS[method]
    except (KeyError, TypeError):
        raise ValueError(f"method must be one of {sorted(METHODS)}, not {method!r}") from None


@dataclass
class MantelResult:
    """One Mantel test per replicate matrix, arrays of length R (first(): the
    same with scalars, for a single matrix).

    statistic        r of X against Y; NaN for an invalid or a constant matrix
    n_ge, n_le, n_abs_ge   permutations with r >= , <= the observed r, and with
                     |r| >= |observed r|
    n                samples
    permutations     permutations
    valid            0 for a matrix with a non-finite entry above its diagonal
    perm_statistics  (R, permutations) when asked for, else None
    """
    method: str
    statistic: np.ndarray
    n: int
    permutations: int
    n_ge: np.ndarray
    n_le: np.ndarray
    n_abs_ge: np.ndarray
    valid: np.ndarray
    perm_statistics: np.ndarray | None = None

    @classmethod
    def from_counts(cls, method, n, permutations, stat, n_ge, n_le, n_abs_ge, valid, perm_stat=None):
        u32 = lambda x: np.asarray(x, dtype=np.uint32)   # noqa: E731
        return cls(method, np.asarray(stat, dtype=np.float64), int(n), int(permutations), u32(n_ge), u32(n_le),
                   u32(n_abs_ge), np.asarray(valid, dtype=np.uint8), perm_stat)

    def p_value(self, alternative="two-sided"):
        """(1 + count) / (1 + permutations) with the count of `alternative`
        ("two-sided", "greater", "less"); NaN where the statistic is (an
        invalid or a constant matrix), as scikit-bio reports it."""
        if alternative not in ALTERNATIVES:
            raise ValueError(f"alternative must be one of {ALTERNATIVES}, not {alternative!r}")
        count = {"two-sided": self.n_abs_ge, "greater": self.n_ge, "less": self.n_le}[alternative]
        p = (1.0 + np.asarray(count, dtype=np.float64)) / (1.0 + self.permutations)
        p = np.where(np.isnan(self.statistic), np.nan, p)
        return float(p) if np.ndim(self.statistic) == 0 else p

    def __len__(self):
        return len(self.valid)

    def first(self):
        """The result of replicate 0 with scalar fields."""
        return MantelResult(self.method, float(self.statistic[0]), self.n, self.permutations, int(self.n_ge[0]),
                            int(self.n_le[0]), int(self.n_abs_ge[0]), int(self.valid[0]),
                            None if self.perm_statistics is None else self.perm_statistics[0])


def permutations(n, P, seed=0):
    """P permutations of 0..n-1 as an int32 (P, n) array, drawn from
    numpy.random.default_rng(seed): deterministic for a seed. The same rows
    serve every replicate matrix of a batched call."""
    n, P = int(n), int(P)
    if n < 0 or P < 0:
        raise ValueError("n and P must be >= 0")
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.permuted(np.tile(np.arange(n, dtype=np.int32), (P, 1)), axis=1),
                                dtype=np.int32).reshape(P, n)


def check_inputs(Y, perms, n=None):
    """(Y float64 (N, N), perms int32 (P, N)) after the checks rc_mantel makes:
    N >= 3, Y finite above its diagonal, every row of perms a rearrangement of
    0..N-1. ValueError otherwise."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[0] != Y.shape[1] or (n is not None and Y.shape[0] != n):
        raise ValueError("Y must be a square matrix of the samples of X")
    n = Y.shape[0]
    if n < 3:
        raise ValueError("a Mantel test needs at least 3 samples")
    if not np.isfinite(Y[np.triu_indices(n, 1)]).all():
        raise ValueError("a non-finite entry above Y's diagonal")
    if perms is None:
        perms = np.zeros((0, n), dtype=np.int32)
    else:
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.size == 0:
            perms = perms.reshape(0, n)
        if perms.ndim != 2 or perms.shape[1] != n:
            raise ValueError("perms must have shape (permutations, N)")
        if perms.size and not np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(n), perms.shape)):
            raise ValueError("a row of perms is not a rearrangement of 0..N-1")
    return Y, perms


# ---------------------------------------------------------------------------
# the host route
# ---------------------------------------------------------------------------

def _mirrored(D):
    U = np.triu(D, 1)
    return U + U.T


def _centred(D):
    """(xc, sxx, constant) of one matrix: centred off the diagonal, zero on it."""
    n = len(D)
    A = _mirrored(D)
    constant = bool((A[np.triu_indices(n, 1)] == A[0, 1]).all())
    mx = _halving_sum(np.cumsum(A, axis=0)[-1]) / (np.float64(n) * np.float64(n - 1))
    xc = A - mx
    xc[np.diag_indices(n)] = 0.0
    return xc, _halving_sum(np.cumsum(xc * xc, axis=0)[-1]), constant


def _ranks(D):
    """The twice-ranks of one matrix as an int64 (N, N) matrix, zero diagonal."""
    n = len(D)
    iu = np.triu_indices(n, 1)
    out = np.zeros((n, n), dtype=np.int64)
    out[iu] = _twice_ranks(D[iu])
    return out + out.T


def _one_host(X, rows, ypre, spearman):
    """(stat, n_ge, n_le, n_abs_ge, perm_stat, valid) of one matrix; rows: the
    identity, then the permutations."""
    n = X.shape[0]
    P = len(rows) - 1
    iu = np.triu_indices(n, 1)
    nan = np.float64(np.nan)
    if not np.isfinite(X[iu]).all():
        return nan, 0, 0, 0, np.full(P, nan), 0
    undefined = (nan, 0, 0, 0, np.full(P, nan), 1)
    step = max(1, (1 << 21) // (n * n))   # permutations per block: gathers of about 16 MB
    with np.errstate(all="ignore"):
        if spearman:
            b, sb, sbb = ypre
            a = _ranks(X)
            M = n * (n - 1) // 2
            sa, saa = int(a[iu].sum()), int((a[iu] * a[iu]).sum())
            vx, vy = M * saa - sa * sa, M * sbb - sb * sb
            if vx == 0 or vy == 0:
                return undefined
            s2 = np.zeros(len(rows), dtype=np.int64)   # twice Sab: the whole symmetric matrix
            for k0 in range(0, len(rows), step):
                p = rows[k0:k0 + step]
                s2[k0:k0 + step] = (a[p[:, :, None], p[:, None, :]] * b).sum(axis=(1, 2))
            num = M * (s2 // 2) - sa * sb
            r = num.astype(np.float64) / np.sqrt(np.float64(vx) * np.float64(vy))
            cmp, absr = num, np.abs(num)
        else:
            yc, syy, yconst = ypre
            xc, sxx, xconst = _centred(X)
            if xconst or yconst:
                return undefined
            scale = np.sqrt(sxx * syy)
            r = np.zeros(len(rows))
            for k0 in range(0, len(rows), step):
                p = rows[k0:k0 + step]
                c = np.cumsum(xc[p[:, :, None], p[:, None, :]] * yc, axis=1)[:, -1, :]
                r[k0:k0 + step] = _halving_sum(c) / scale
            cmp, absr = r, np.abs(r)
        return (r[0], int((cmp[1:] >= cmp[0]).sum()), int((cmp[1:] <= cmp[0]).sum()),
                int((absr[1:] >= absr[0]).sum()), r[1:], 1)


def mantel_host(X, Y, perms=None, method="pearson", *, perm_stats=False, threads=None):
    """The Mantel test of distance matrices X (R, N, N) or (N, N) against Y
    (N, N) in numpy, for any N: the same definitions and operation order as
    the GPU route (Engine.mantel), so the same bits. perms (P, N): permutations
    of 0..N-1 (permutations()); none: the statistics only. Returns
    MantelResult with one entry per matrix. `threads`: matrices tested at a
    time (default: up to 16, no more than the machine's CPUs)."""
    code = method_code(method)
    D = np.asarray(X, dtype=np.float64)
    if D.ndim == 2:
        D = D[None]
    if D.ndim != 3 or D.shape[1] != D.shape[2]:
        raise ValueError("X must have shape (replicates, N, N)")
    n = D.shape[1]
    Y, perms = check_inputs(Y, perms, n)
    R, P = len(D), len(perms)
    rows = np.concatenate([np.arange(n, dtype=np.int32)[None], perms]).astype(np.intp)
    if code == 1:
        b = _ranks(Y)
        bu = b[np.triu_indices(n, 1)]
        ypre = (b, int(bu.sum()), int((bu * bu).sum()))
    else:
        with np.errstate(all="ignore"):
            ypre = _centred(Y)
    if threads is None:
        threads = min(16, os.cpu_count() or 1)
    work = lambda r: _one_host(D[r], rows, ypre, code == 1)   # noqa: E731
    if threads > 1 and R > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(threads, R)) as ex:
            out = list(ex.map(work, range(R)))
    else:
        out = [work(r) for r in range(R)]
    stat, n_ge, n_le, n_abs, ps, valid = (list(c) for c in zip(*out)) if out else ([],) * 6
    pstat = np.array(ps, dtype=np.float64).reshape(R, P) if perm_stats else None
    return MantelResult.from_counts(method, n, P, stat, n_ge, n_le, n_abs, valid, pstat)


def align_matrix(samples, other, strict=True):
    """`other` -- a pandas DataFrame with sample labels on both axes, or a
    (labels, matrix) pair -- as (common samples in `samples` order, their
    positions in `samples`, the matrix in that order). Samples missing on
    either side raise ValueError unless strict is False, which restricts the
    test to the common ones (scikit-bio's rule)."""
    samples = list(samples)
    if hasattr(other, "index") and hasattr(other, "columns"):
        labels, mat = list(other.index), np.asarray(other.to_numpy(), dtype=np.float64)
        if list(other.columns) != labels:
            raise ValueError("the other matrix must carry the same labels on its rows and columns")
    else:
        labels, mat = other
        labels, mat = list(labels), np.asarray(mat, dtype=np.float64)
    if mat.ndim != 2 or mat.shape != (len(labels), len(labels)):
        raise ValueError("the other matrix must be square, one row per label")
    if len(set(labels)) != len(labels):
        raise ValueError("the other matrix has a label twice")
    where = {s: i for i, s in enumerate(labels)}
    common = [s for s in samples if s in where]
    if strict and (len(common) != len(samples) or len(common) != len(labels)):
        missing = sorted(set(map(str, samples)) ^ set(map(str, labels)))
        raise ValueError(f"samples on one side only: {missing} (strict=False tests the common ones)")
    if len(common) < 3:
        raise ValueError("a Mantel test needs at least 3 common samples")
    idx = [where[s] for s in common]
    position = {s: i for i, s in enumerate(samples)}
    return common, [position[s] for s in common], np.ascontiguousarray(mat[np.ix_(idx, idx)])
