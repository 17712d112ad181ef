"""Host statement of the GPU's principal coordinates (pcoa.hip, include/rcgpu.h):
Gower centring, the shift by sigma = ||B||_F and one-sided Jacobi sweeps in
round-robin order, in numpy, vectorised over the pairs of a step and over the
batch. The kernel differs from it only in the order in which the terms of a
dot product are added and in the last bit of sqrt and /, so the two are
compared through the same bound, not as bits.

TOL_UNITS bounds the four errors of errors() in units of u = n 2^-52 ||B||_F,
the form of a backward-stable solver's bound. It is the next power of two
above twice the worst value this oracle shows against numpy.linalg.eigh over
tests/pcoa_cases.py (test_pcoa_host.py measures it; DESIGN.md section 6 has
the table): the factor two is the room for the kernel's summation order."""
import numpy as np

TOL_UNITS = 16
DEFAULT_SWEEPS = 30
EPS = 2.0 ** -52


def centre(D):
    """B of the upper triangle of D (..., n, n), by the kernel's operation order."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[-1]
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    E = np.where(up, -0.5 * (D * D), 0.0)
    E = E + np.swapaxes(E, -1, -2)
    rowmean = np.zeros(D.shape[:-1])
    for j in range(n):
        rowmean = rowmean + E[..., j]
    rowmean = rowmean / n
    grand = np.zeros(D.shape[:-2])
    for i in range(n):
        grand = grand + rowmean[..., i]
    grand = grand / n
    B = ((E - rowmean[..., :, None]) - rowmean[..., None, :]) + grand[..., None, None]
    B = np.where(up | np.eye(n, dtype=bool), B, 0.0)
    return B + np.swapaxes(np.where(up, B, 0.0), -1, -2)


def step_pairs(n, s):
    """The (p, q) index arrays, p < q < n, of step s of a sweep over n columns."""
    m = (n + 1) & ~1
    g = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (s + g) % (m - 1)])
    b = np.concatenate([[s], (s - g) % (m - 1)])
    p, q = np.minimum(a, b), np.maximum(a, b)
    keep = q < n
    return p[keep], q[keep]


def pcoa_batch(D, k=None, max_sweeps=0):
    """(values (R, n), vectors (R, n, k), sweeps (R,), valid (R,), rotating
    (R,)) of the matrices D (R, n, n); rotating: still rotated in its last
    allowed sweep."""
    D = np.array(D, dtype=np.float64)
    if D.ndim == 2:
        D = D[None]
    R, n = D.shape[0], D.shape[1]
    k = n if k is None else k
    max_sweeps = max_sweeps or DEFAULT_SWEEPS
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    valid = np.isfinite(np.where(up, D, 0.0)).all(axis=(1, 2))
    D[~valid] = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        B = centre(D)
        colsq = np.zeros((R, n))
        for i in range(n):
            colsq = colsq + B[:, i, :] * B[:, i, :]
        ss = np.zeros(R)
        for c in range(n):
            ss = ss + colsq[:, c]
        sigma = np.sqrt(ss)
    bad = ~np.isfinite(sigma)
    valid &= ~bad
    B[bad] = 0.0
    sigma = np.where(bad, 0.0, sigma)
    A = B + sigma[:, None, None] * np.eye(n)       # A[r, row, column]
    sweeps = np.zeros(R, dtype=np.int32)
    live = np.ones(R, dtype=bool)
    m = (n + 1) & ~1
    for _ in range(max_sweeps):
        rotated = np.zeros(R, dtype=bool)
        for s in range(m - 1):
            p, q = step_pairs(n, s)
            if not len(p):
                continue
            x, y = A[:, :, p], A[:, :, q]
            al, be, ga = (x * x).sum(axis=1), (y * y).sum(axis=1), (x * y).sum(axis=1)
            rot = (al != 0) & (be != 0) & (np.abs(ga) > (EPS * np.sqrt(al)) * np.sqrt(be)) & live[:, None]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                zeta = (be - al) / (2.0 * ga)
                t = 1.0 / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                t = np.where(zeta < 0, -t, t)
                c = 1.0 / np.sqrt(1.0 + t * t)
                sn = c * t
            c = np.where(rot, c, 1.0)[:, None, :]
            sn = np.where(rot, sn, 0.0)[:, None, :]
            A[:, :, p] = np.where(rot[:, None, :], c * x - sn * y, x)
            A[:, :, q] = np.where(rot[:, None, :], sn * x + c * y, y)
            rotated |= rot.any(axis=1)
        sweeps[live] += 1
        live &= rotated
        if not live.any():
            break
    norm = np.sqrt((A * A).sum(axis=1))
    lam = norm - sigma[:, None]
    # descending, ties by the lower column: a stable sort of -lam
    order = np.argsort(-lam, axis=1, kind="stable")
    values = np.take_along_axis(lam, order, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        V = np.where(norm[:, None, :] != 0, A / norm[:, None, :], 0.0)
    V = apply_sign_rule(V)
    vectors = np.take_along_axis(V, order[:, None, :], axis=2)[:, :, :k]
    values[~valid] = np.nan
    vectors[~valid] = np.nan
    sweeps[~valid] = 0
    return values, np.ascontiguousarray(vectors), sweeps, valid.astype(np.uint8), live & valid


def apply_sign_rule(V):
    """Each column (..., n, k) with its entry of largest magnitude positive,
    the lowest row among equal magnitudes."""
    V = np.asarray(V, dtype=np.float64)
    top = np.argmax(np.abs(V), axis=-2)   # the first maximum
    lead = np.take_along_axis(V, top[..., None, :], axis=-2)
    return np.where(lead < 0, -V, V)


def pcoa(D, k=None, max_sweeps=0):
    values, vectors, sweeps, valid, _ = pcoa_batch(D, k, max_sweeps)
    return values[0], vectors[0], int(sweeps[0]), int(valid[0])


def unit(B):
    """u = n 2^-52 ||B||_F."""
    return B.shape[-1] * EPS * float(np.linalg.norm(B))


def errors(D, values, vectors):
    """(E_gram, E_val, E_res in units of u; E_orth in units of n 2^-52) of a
    full (k = n) result against numpy.linalg.eigh on the numpy-centred B. On a
    zero B (u = 0) the first three are 0 when the error is exactly 0, else
    inf; E_orth is then left to the caller (every vector is zero)."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    Ds = np.triu(D, 1) + np.triu(D, 1).T
    J = np.eye(n) - np.full((n, n), 1.0 / n)
    B = J @ (-0.5 * Ds * Ds) @ J
    B = (B + B.T) / 2
    w, W = np.linalg.eigh(B)
    Bplus = (W * np.maximum(w, 0)) @ W.T
    X = vectors * np.sqrt(np.maximum(values, 0))
    u = unit(B)
    e_gram = float(np.linalg.norm(X @ X.T - Bplus))
    e_val = float(np.abs(np.sort(values)[::-1] - w[::-1]).max())
    e_res = float(np.linalg.norm(B @ vectors - vectors * values))
    e_orth = float(np.linalg.norm(vectors.T @ vectors - np.eye(n))) / (n * EPS)

    def rel(e):
        return e / u if u > 0 else (0.0 if e == 0 else np.inf)
    return rel(e_gram), rel(e_val), rel(e_res), e_orth
