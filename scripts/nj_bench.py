"""Time neighbour joining and split support on the GPU (rc_nj,
rc_resample_trees) against what a user had before them.

R = 1000 replicate matrices at 32 and at 128 samples: one additive
birth-death tree per size, every distance of a replicate scaled by its own
factor in [0.7, 1.3] (tests/nj_cases.py). For each size, median of 5 calls
after one warm-up:

* Engine.nj(matrices, ref_splits): the wall time of the call (upload of
  R x N x N doubles, kernels, copy back) and the kernels alone
  (rc_timing.nj_ms, device events); at 128 samples on both paths (matrix in
  LDS, and RC_NJ_LDS=0: matrix in the global workspace);
* a graph-only engine of that many samples (pair-major ideal cliques):
  resample_trees(W) for 1000 bootstrap rows, where the matrices stay on the
  device, against bootstrap_dissimilarity_matrices plus a host loop -- with
  tests/treecheck.py's nj_splits and with tests/nj_oracle.py -- over the first
  --host-reps matrices, scaled to 1000.

    python scripts/nj_bench.py [--out FILE]
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

import nj_cases as nc   # noqa: E402
import nj_oracle as no   # noqa: E402
import treecheck   # noqa: E402
from rna_clique_amd import _native as nat   # noqa: E402
from rna_clique_amd.engine import Engine   # noqa: E402
from rna_clique_amd.similarity import SampleSimilarity, bootstrap_weights   # noqa: E402


def median_time(fn, runs=5):
    ts = []
    for _ in range(runs + 1):   # the first run is the warm-up
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:])


def clique_engine(n_samples, n_cliques, seed=0):
    """A graph-only engine of n_cliques complete cliques over all samples."""
    eng = Engine(device=0)
    for s in range(n_samples):
        eng.add_sample(f"S{s:03d}", np.zeros(0, np.uint8), np.zeros(n_cliques + 1, np.uint64),
                       np.arange(1, n_cliques + 1, dtype=np.int32), np.ones(n_cliques, np.int32))
    rng = np.random.default_rng(seed)
    order = eng.pair_order()
    k = np.arange(n_cliques, dtype=np.uint32)
    arr = np.zeros(len(order) * n_cliques, dtype=nat.EDGE_RECORD_DTYPE)
    for p, (a, b) in enumerate(order):
        blk = arr[p * n_cliques:(p + 1) * n_cliques]
        blk["a"], blk["b"], blk["pair"] = a * n_cliques + k, b * n_cliques + k, p
        num = rng.integers(200, 3000, size=n_cliques, dtype=np.int32)
        blk["nident"] = num
        blk["den"] = num + rng.integers(0, 60 + 10 * abs(a - b), size=n_cliques, dtype=np.int32)
    eng.import_edges(arr.view(np.uint8))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--cliques", type=int, default=400)
    ap.add_argument("--host-reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    R = a.reps
    for N in a.sizes:
        base = nc.additive(N, seed=N)[0]
        Ds = np.stack([nc.jitter(base, seed=r) for r in range(R)])
        ref = no.nj(base)[2]
        say(f"nj_bench: {R} matrices of {N} samples ({Ds.nbytes / 1e6:.0f} MB), {len(ref)} reference splits")
        for knob in (None, "0") if N == max(a.sizes) else (None,):
            if knob is None:
                os.environ.pop("RC_NJ_LDS", None)
            else:
                os.environ["RC_NJ_LDS"] = knob
            eng = Engine(device=0)
            kern, res = [], []

            def call():
                res.append(eng.nj(Ds, ref))
                kern.append(eng.timings()["nj_ms"])
            t_call = median_time(call)
            path = "matrix in LDS" if knob is None and N <= 128 else "matrix in the global workspace"
            say(f"  rc_nj, {path}: call {t_call * 1e3:.2f} ms, kernels {statistics.median(kern[1:]):.3f} ms "
                f"(support of the true tree's splits: mean {res[-1].support.mean() / R:.3f})")
            want = no.nj_batch(Ds[:4])
            same = all(np.array_equal(x, y) for x, y in zip((res[-1].joins[:4], res[-1].splits[:4]), (want[0], want[2])))
            same = same and res[-1].lengths[:4].tobytes() == want[1].tobytes()
            say(f"    first 4 trees equal the oracle's bit for bit: {same}")
            if not same:
                raise SystemExit("GPU and oracle trees differ")
            eng.close()
        os.environ.pop("RC_NJ_LDS", None)
        # the engine path and what a user had before it
        eng = clique_engine(N, a.cliques)
        sim = SampleSimilarity.from_engine(eng)
        C = eng.n_components()
        W = bootstrap_weights(C, R, seed=N)
        kern = []

        def trees():
            eng.resample_trees(W)
            kern.append((eng.timings()["resample_ms"], eng.timings()["nj_ms"]))
        t_trees = median_time(trees)
        say(f"  engine of {N} samples x {C} components: resample_trees({R} bootstrap rows) call {t_trees * 1e3:.2f} ms "
            f"(product kernel {statistics.median(k[0] for k in kern[1:]):.3f} ms, "
            f"tree and support kernels {statistics.median(k[1] for k in kern[1:]):.3f} ms)")
        t_mats = median_time(lambda: sim.resampled_dissimilarity_matrices(W), 3)
        mats = sim.resampled_dissimilarity_matrices(W)[:a.host_reps]
        labels = sim.samples
        t0 = time.perf_counter()
        for m in mats:
            treecheck.nj_splits(m, labels)
        t_tc = (time.perf_counter() - t0) / len(mats) * R
        t0 = time.perf_counter()
        for m in mats:
            no.nj(m)
        t_or = (time.perf_counter() - t0) / len(mats) * R
        say(f"  before: resampled matrices to the host {t_mats * 1e3:.1f} ms + a host loop over {R} matrices "
            f"(timed on {len(mats)}): treecheck.nj_splits {t_tc:.2f} s, nj_oracle.nj {t_or:.2f} s "
            f"= {(t_mats + min(t_tc, t_or)) / t_trees:.0f}x the resample_trees call")
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
