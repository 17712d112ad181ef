"""Distance matrices for the principal coordinates tests (tests/pcoa_oracle.py,
test_pcoa_host.py, test_gpu_pcoa.py). Every function returns a symmetric
float64 (n, n) matrix with a zero diagonal."""
import functools

import numpy as np

SIZES = (2, 3, 4, 5, 8, 9, 10, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
NAMES = ("euclid3", "noneuclid", "all_equal", "manhattan", "zero", "duplicate", "spectrum")
LAMS = (9e-4, 4e-4, 1e-4)
GAP = 1e-4   # the smallest gap between the values of LAMS and 0


def _pairwise(X, p):
    diff = np.abs(X[:, None, :] - X[None, :, :])
    D = diff.sum(axis=2) if p == 1 else np.sqrt((diff * diff).sum(axis=2))
    D = (D + D.T) / 2
    np.fill_diagonal(D, 0.0)
    return D


def euclid3(n, seed=0):
    """Points in R^3 with axis scales 3:2:1."""
    X = np.random.default_rng(seed).standard_normal((n, 3)) * np.array([3.0, 2.0, 1.0])
    return _pairwise(X, 2)


def noneuclid(n, seed=0):
    """Random symmetric, uniform [0.1, 1]: about half its eigenvalues are negative."""
    U = np.random.default_rng(seed).uniform(0.1, 1.0, size=(n, n))
    D = np.triu(U, 1)
    return D + D.T


def all_equal(n):
    """Every distance 0.25: an (n - 1)-fold eigenvalue."""
    D = np.full((n, n), 0.25)
    np.fill_diagonal(D, 0.0)
    return D


def manhattan(n, seed=0):
    """L1 distances of 40 uniform coordinates in [0, 0.02]: the scale of real
    dissimilarities, mildly non-Euclidean."""
    return _pairwise(np.random.default_rng(seed).uniform(0.0, 0.02, size=(n, 40)), 1)


def zero(n):
    return np.zeros((n, n))


def duplicate(n, seed=0):
    """manhattan with samples 0 and 1 identical: B is rank deficient."""
    X = np.random.default_rng(seed).uniform(0.0, 0.02, size=(n, 40))
    X[1] = X[0]
    return _pairwise(X, 1)


def spectrum(n, lams=LAMS, seed=0):
    """Orthonormal centred columns scaled by sqrt(lams): B has exactly those
    eigenvalues (as many of them as n - 1 allows) and zeros."""
    lams = np.asarray(lams, dtype=np.float64)[:n - 1]
    G = np.random.default_rng(seed).standard_normal((n, len(lams)))
    G = G - G.mean(axis=0)
    Q, _ = np.linalg.qr(G)
    Q = Q - Q.mean(axis=0)
    Q, _ = np.linalg.qr(Q)
    return _pairwise(Q * np.sqrt(lams), 2)


def spectrum_lams(n):
    """The non-zero eigenvalues of spectrum(n), descending."""
    return np.asarray(LAMS, dtype=np.float64)[:n - 1]


@functools.lru_cache(maxsize=None)
def batch(n):
    """All named cases at n samples, in the order of NAMES (read-only)."""
    Ds = np.stack([euclid3(n, seed=n), noneuclid(n, seed=n + 1), all_equal(n), manhattan(n, seed=n + 2), zero(n),
                   duplicate(n, seed=n + 3), spectrum(n, seed=n + 4)])
    Ds.setflags(write=False)
    return Ds
