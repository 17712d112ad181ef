"""Time the Mantel test on the GPU (rc_mantel, rc_resample_mantel) against the
host route in numpy (rna_clique_amd.mantel.mantel_host) and scipy
(scipy.stats.pearsonr / spearmanr of the permuted upper triangles, what
skbio.stats.distance.mantel does per permutation).

For pearson and spearman each:

* a graph-only engine of 32 and of 128 samples (pair-major ideal cliques, as
  scripts/nj_bench.py builds it): resample_mantel(W) for 1000 bootstrap rows x
  999 permutations against a jittered copy of the engine's own matrix, where
  the replicate matrices stay on the device -- the device time of the ranking
  and test kernels (rc_timing.mantel_ms) and the wall time of the whole call,
  median and spread of --runs calls after one warm-up;
* the same call with --identity: every permutation the identity, so the
  gathered LDS reads of X fall on consecutive addresses -- the difference is
  what the permutation's bank conflicts cost;
* one matrix of each size x 9999 permutations through Engine.mantel;
* the baselines: mantel_host on the same matrices with up to 16 threads, timed
  on the first --host-reps of them and scaled, and scipy on one matrix x
  --scipy-perms permutations, scaled.

The first --host-reps results of the GPU are checked against the host route
bit for bit before any time is reported.

    python scripts/mantel_bench.py [--out FILE]
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
from rna_clique_amd import mantel   # noqa: E402
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
            and np.array_equal(a.n_le[:rows], b.n_le[:rows]) and np.array_equal(a.n_abs_ge[:rows], b.n_abs_ge[:rows]))


def scipy_mantel(X, Y, perms, method):
    from scipy.stats import pearsonr, spearmanr
    corr = pearsonr if method == "pearson" else spearmanr
    iu = np.triu_indices(len(X), 1)
    y = Y[iu]
    return np.array([corr(X[np.ix_(p, p)][iu], y).statistic for p in perms])


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
        order = list(range(N))
        mats = eng.resample(W[:a.host_reps], order)[1]
        rng = np.random.default_rng(N)
        U = np.triu(eng.distance(order)[1] * rng.uniform(0.7, 1.3, size=(N, N)), 1)
        Y = U + U.T
        perms = mantel.permutations(N, P, seed=N)
        ident = np.tile(np.arange(N, dtype=np.int32), (P, 1))
        many = mantel.permutations(N, a.single_perms, seed=N + 1)
        say(f"mantel_bench: engine of {N} samples x {C} components, {R} bootstrap rows, {P} permutations "
            f"({R * P * N * N / 1e9:.2f} G pair visits)")
        for method in ("pearson", "spearman"):
            kern, res = [], []

            def call(pm=perms):
                res.append(eng.resample_mantel(W, Y, pm, order, method)[1])
                kern.append(eng.timings()["mantel_ms"])
            t, lo, hi = timed(call, a.runs)
            k = kern[1:]
            t0 = time.perf_counter()
            host = mantel.mantel_host(mats, Y, perms, method)
            t_host = (time.perf_counter() - t0) / len(mats) * R
            if not same(res[-1], host, len(mats)):
                raise SystemExit(f"{method} at {N} samples: the GPU and the host route disagree")
            t0 = time.perf_counter()
            r = scipy_mantel(mats[0], Y, np.concatenate([np.arange(N)[None], perms[:a.scipy_perms]]), method)
            t_scipy = (time.perf_counter() - t0) / (a.scipy_perms + 1) * (P + 1) * R
            say(f"  {method}: mantel_ms median {statistics.median(k):.3f} (min {min(k):.3f}, max {max(k):.3f}); whole "
                f"call median {t * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}); mantel_host on {len(mats)} "
                f"matrices scaled to {R}: {t_host * 1e3:.0f} ms = {t_host / t:.0f}x the call; scipy (one matrix x "
                f"{a.scipy_perms} permutations scaled): {t_scipy:.0f} s; r of matrix 0: {res[-1].statistic[0]:.6g} "
                f"against scipy's {r[0]:.6g}; two-sided p of the replicates: median {np.median(res[-1].p_value()):.3f}")
            kern.clear()
            timed(lambda: call(ident), a.runs)
            k = kern[1:]
            say(f"    every permutation the identity (no gather conflicts): mantel_ms median {statistics.median(k):.3f} "
                f"(min {min(k):.3f}, max {max(k):.3f})")
            kern.clear()
            for _ in range(a.runs + 1):
                eng.resample_mantel(W, Y, None, order, method)
                kern.append(eng.timings()["mantel_ms"])
            say(f"    no permutations (staging{', ranking' if method == 'spearman' else ''} and the identity): mantel_ms "
                f"median {statistics.median(kern[1:]):.3f}")
            kern.clear()

            def single():
                res.append(eng.mantel(mats[0], Y, many, method))
                kern.append(eng.timings()["mantel_ms"])
            t, lo, hi = timed(single, a.runs)
            k = kern[1:]
            t0 = time.perf_counter()
            host = mantel.mantel_host(mats[0], Y, many, method)
            t_host = time.perf_counter() - t0
            if not same(res[-1], host, 1):
                raise SystemExit(f"{method} at {N} samples: the GPU and the host route disagree")
            say(f"    one matrix x {len(many)} permutations: mantel_ms median {statistics.median(k):.3f} (min "
                f"{min(k):.3f}, max {max(k):.3f}); whole call median {t * 1e3:.2f} ms (min {lo * 1e3:.2f}, max "
                f"{hi * 1e3:.2f}); mantel_host {t_host * 1e3:.0f} ms = {t_host / t:.0f}x the call")
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
