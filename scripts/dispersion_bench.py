"""Time PERMDISP on the GPU (rc_group_dispersion, rc_resample_group_dispersion)
against the host route in numpy (rna_clique_amd.groups.dispersion_host) and a
plain scipy statement (distances to the centroid from the coordinates of a
classical scaling, scipy.stats.f_oneway per permutation).

* a graph-only engine of 32 and of 128 samples (pair-major ideal cliques, as
  scripts/nj_bench.py builds it): resample_group_dispersion(W) for 1000
  bootstrap rows x 999 permutations in four balanced groups, where the
  matrices stay on the device -- the device time of the kernel
  (rc_timing.disp_ms) and the wall time of the whole call, median and spread of
  --runs calls after one warm-up; PERMANOVA's group_ms of the same call shape
  beside it;
* one matrix of each size x 9999 permutations through Engine.group_dispersion;
* the baselines: dispersion_host on the same matrices with up to 16 threads,
  timed on the first --host-reps of them and scaled, and the scipy statement
  on one matrix x --scipy-perms permutations, scaled.

The first --host-reps results of the GPU are checked against the host route
bit for bit before any time is reported.

    python scripts/dispersion_bench.py [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from nj_bench import clique_engine   # noqa: E402
from rna_clique_amd import groups   # noqa: E402
from rna_clique_amd.similarity import bootstrap_weights   # noqa: E402


def timed(fn, runs):
    """(median, min, max) seconds of `runs` calls after one warm-up."""
    ts = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = ts[1:]
    return statistics.median(ts), min(ts), max(ts)


def same(a, b, rows):
    bits = lambda x: np.ascontiguousarray(x[:rows], dtype=np.float64).view(np.uint64)   # noqa: E731
    return (np.array_equal(bits(a.statistic), bits(b.statistic)) and np.array_equal(a.n_ge[:rows], b.n_ge[:rows])
            and np.array_equal(bits(a.total), bits(b.total)) and np.array_equal(bits(a.within), bits(b.within))
            and np.array_equal(bits(a.distances), bits(b.distances)))


def scipy_permdisp(D, labels, perms):
    """PERMDISP as scikit-bio states it: coordinates of a classical scaling (all
    axes with a positive eigenvalue), distances to the group centroids, f_oneway."""
    from scipy.stats import f_oneway
    n = len(D)
    J = np.eye(n) - 1.0 / n
    w, v = np.linalg.eigh(-0.5 * J @ (D * D) @ J)
    X = v[:, w > 1e-12] * np.sqrt(w[w > 1e-12])
    out = []
    for g in np.concatenate([labels[None], perms]):
        z = np.zeros(n)
        for k in range(int(g.max()) + 1):
            m = g == k
            z[m] = np.linalg.norm(X[m] - X[m].mean(axis=0), axis=1)
        out.append(f_oneway(*[z[g == k] for k in range(int(g.max()) + 1)]).statistic)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--perms", type=int, default=999)
    ap.add_argument("--single-perms", type=int, default=9999)
    ap.add_argument("--cliques", type=int, default=400)
    ap.add_argument("--host-reps", type=int, default=16)
    ap.add_argument("--scipy-perms", type=int, default=99)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    R, P = a.reps, a.perms
    for N in a.sizes:
        eng = clique_engine(N, a.cliques)
        C = eng.n_components()
        W = bootstrap_weights(C, R, seed=N)
        labels = (np.arange(N) % 4).astype(np.int32)
        perms = groups.permuted_labels(labels, P, seed=N)
        many = groups.permuted_labels(labels, a.single_perms, seed=N + 1)
        order = list(range(N))
        mats = eng.resample(W[:a.host_reps], order)[1]
        say(f"dispersion_bench: engine of {N} samples x {C} components, {R} bootstrap rows, {P} permutations, 4 groups "
            f"({R * P * N * N / 1e9:.2f} G pair visits)")
        kern, res = [], []

        def call():
            res.append(eng.resample_group_dispersion(W, labels, perms, order)[1])
            kern.append(eng.timings()["disp_ms"])
        t, lo, hi = timed(call, a.runs)
        k = kern[1:]
        t0 = time.perf_counter()
        host = groups.dispersion_host(mats, labels, perms)
        t_host = (time.perf_counter() - t0) / len(mats) * R
        if not same(res[-1], host, len(mats)):
            raise SystemExit(f"PERMDISP at {N} samples: the GPU and the host route disagree")
        t0 = time.perf_counter()
        f = scipy_permdisp(mats[0], labels, perms[:a.scipy_perms])
        t_scipy = (time.perf_counter() - t0) / (a.scipy_perms + 1) * (P + 1) * R
        say(f"  permdisp: disp_ms median {statistics.median(k):.3f} (min {min(k):.3f}, max {max(k):.3f}); whole call "
            f"median {t * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}); dispersion_host on {len(mats)} matrices "
            f"scaled to {R}: {t_host * 1e3:.0f} ms = {t_host / t:.0f}x the call; scipy (eigh + f_oneway, one matrix x "
            f"{a.scipy_perms} permutations scaled): {t_scipy:.0f} s; F of matrix 0: {res[-1].statistic[0]:.6g} against "
            f"scipy's {f[0]:.6g}; p-values of the replicates: median {np.median(res[-1].p_value):.3f}")
        gk = []
        for _ in range(a.runs + 1):
            eng.resample_group_test(W, labels, perms, order, "permanova")
            gk.append(eng.timings()["group_ms"])
        say(f"    PERMANOVA on the same call: group_ms median {statistics.median(gk[1:]):.3f}")
        kern.clear()

        def single():
            res.append(eng.group_dispersion(mats[0], labels, many))
            kern.append(eng.timings()["disp_ms"])
        t, lo, hi = timed(single, a.runs)
        k = kern[1:]
        t0 = time.perf_counter()
        host = groups.dispersion_host(mats[0], labels, many)
        t_host = time.perf_counter() - t0
        if not same(res[-1], host, 1):
            raise SystemExit(f"PERMDISP at {N} samples: the GPU and the host route disagree")
        say(f"    one matrix x {len(many)} permutations: disp_ms median {statistics.median(k):.3f} (min {min(k):.3f}, "
            f"max {max(k):.3f}); whole call median {t * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}); "
            f"dispersion_host {t_host * 1e3:.0f} ms = {t_host / t:.0f}x the call")
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
