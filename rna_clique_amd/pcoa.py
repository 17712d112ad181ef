"""Principal coordinates analysis (PCoA, classical scaling) of dissimilarity
matrices: the result type the GPU calls fill (Engine.pcoa, Engine.resample_pcoa,
SampleSimilarity.pcoa / bootstrap_pcoa), a host route through
numpy.linalg.eigh, and the Procrustes alignment of replicate ordinations.

PCoAResult carries the fields the reference's viz/pcoa.py reads from
scikit-bio's OrdinationResults (samples, eigvals, proportion_explained) and
applies the rule scikit-bio documents for skbio.stats.ordination.pcoa:
eigenvalues that np.isclose to 0 become 0; negative eigenvalues and their axes
become 0, with a warning; coordinates = eigenvectors * sqrt(eigenvalues);
proportion explained = eigenvalues / their sum. This restates that documented
method; scikit-bio is not a dependency and the numbers are not pinned against
it."""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import pandas as pd

MAX_GPU_SAMPLES = 128


@dataclass
class PCoAEigen:
    """What rc_pcoa / rc_resample_pcoa return, with a leading replicate axis:
    values (R, n) descending, vectors (R, n, k) unit eigenvectors (sample-major,
    largest entry positive), sweeps (R,) Jacobi sweeps run, valid (R,) 0 for a
    matrix with a non-finite entry (its values and vectors are NaN)."""
    values: np.ndarray
    vectors: np.ndarray
    sweeps: np.ndarray
    valid: np.ndarray


def clamp(values, vectors):
    """scikit-bio's rule on eigenvalues (..., n) descending and eigenvectors
    (..., n, k): (eigvals, coordinates, had_negative). The eigenvalues that
    np.isclose to 0 are set to 0, then the negative ones and their axes."""
    lam = np.array(values, dtype=np.float64)
    vec = np.asarray(vectors, dtype=np.float64)
    lam[np.isclose(lam, 0.0)] = 0.0
    negative = lam < 0
    lam[negative] = 0.0
    k = vec.shape[-1]
    return lam, vec * np.sqrt(lam[..., None, :k]), bool(negative.any())


class PCoAResult:
    """One ordination. samples: DataFrame indexed by sample, columns PC1...;
    eigvals (all n of them) and proportion_explained: Series indexed PC1...
    (the fields viz/pcoa.py reads from OrdinationResults). raw_eigvals keeps
    the eigenvalues before the clamp."""

    def __init__(self, labels, values, vectors, *, warn=True):
        values = np.asarray(values, dtype=np.float64)
        vectors = np.asarray(vectors, dtype=np.float64)
        if values.ndim != 1 or vectors.ndim != 2 or vectors.shape[0] != len(values) or len(labels) != len(values):
            raise ValueError("values (n,), vectors (n, k) and n labels are needed")
        lam, coords, negative = clamp(values, vectors)
        if negative and warn:
            warnings.warn("The result contains negative eigenvalues: the distances are not Euclidean. "
                          f"Their axes are set to zero (most negative {values.min():.6g}, "
                          f"largest {values.max():.6g}).", RuntimeWarning, stacklevel=2)
        names = [f"PC{i + 1}" for i in range(len(lam))]
        total = lam.sum()
        self.raw_eigvals = values
        self.eigvals = pd.Series(lam, index=names)
        self.proportion_explained = pd.Series(lam / total if total > 0 else np.zeros_like(lam), index=names)
        self.samples = pd.DataFrame(coords, index=list(labels), columns=names[:coords.shape[1]])

    @property
    def coordinates(self) -> np.ndarray:
        return self.samples.to_numpy()


def gower_centre(D):
    """B = -1/2 J D^2 J of a symmetric distance matrix (the upper triangle is read)."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError("a square distance matrix is needed")
    n = D.shape[0]
    up = np.triu(D, 1)
    E = -0.5 * (up + up.T) ** 2
    rm = E.mean(axis=1)
    B = E - rm[:, None] - rm[None, :] + E.mean()
    return (B + B.T) / 2 if n else B


def sign_rule(V):
    """Columns (..., n, k) with their entry of largest magnitude positive
    (the lowest sample among equal magnitudes), as the GPU writes them."""
    V = np.asarray(V, dtype=np.float64)
    top = np.argmax(np.abs(V), axis=-2)
    lead = np.take_along_axis(V, top[..., None, :], axis=-2)
    return np.where(lead < 0, -V, V)


def eigh_eigen(D, k=None):
    """(values (n,) descending, vectors (n, k)) of gower_centre(D) by
    numpy.linalg.eigh, in the GPU's conventions."""
    B = gower_centre(D)
    n = B.shape[0]
    if n < 2:
        raise ValueError("principal coordinates need at least 2 samples")
    if not np.isfinite(B).all():
        raise ValueError("the distance matrix has a non-finite entry")
    k = n if k is None else int(k)
    if not 1 <= k <= n:
        raise ValueError("k must lie in 1..n")
    w, W = np.linalg.eigh(B)
    return w[::-1].copy(), sign_rule(W[:, ::-1][:, :k])


def pcoa_eigh(D, labels=None, dimensions=None, *, warn=True) -> PCoAResult:
    """PCoAResult of one distance matrix on the host (numpy.linalg.eigh): the
    route for more than 128 samples, and the reference of the GPU tests."""
    D = np.asarray(D, dtype=np.float64)
    values, vectors = eigh_eigen(D, dimensions)
    return PCoAResult(list(range(len(values))) if labels is None else labels, values, vectors, warn=warn)


def procrustes_align(X, ref):
    """X (..., n, k) rotated and reflected onto ref (n, k) or (..., n, k): X R
    with the orthogonal R = U V^T of the SVD X^T ref = U S V^T, which
    minimises ||X R - ref||_F (no translation, no scaling: principal
    coordinates are centred, and a replicate's spread is part of what a
    bootstrap shows). The matrices are k x k, so this runs on the host."""
    X = np.asarray(X, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if X.ndim < 2 or ref.ndim < 2 or X.shape[-2:] != ref.shape[-2:]:
        raise ValueError("X (..., n, k) and ref (n, k) must agree in n and k")
    if not np.isfinite(X).all() or not np.isfinite(ref).all():
        raise ValueError("non-finite coordinates")
    U, _, Vt = np.linalg.svd(np.swapaxes(X, -1, -2) @ ref)
    return X @ (U @ Vt)
