"""Time the per-component tables and rc_resample at C3 size.

A graph-only engine of 32 samples x 50 000 pair-major ideal cliques (one gene
per sample and clique: 496 pairs x 50 000 = 24.8 M edge records), built in
vectorised numpy. Timed with time.perf_counter around blocking calls, median
of 5 runs after one warm-up:

* the table build (ranks, members, sums, packed cells): the first
  n_components() after an import_edges;
* Engine.resample for R = 100 and R = 1000 bootstrap replicates -- the whole
  call (weight check and upload, product, distances, copy back) and the
  product kernel alone (rc_timing.resample_ms, device events).

Beside them the same W @ S as an int64 numpy product on 16 host threads (the
tests' restatement at this size, in int64 instead of Python integers; median
of 3 after one warm-up), and a check that both give the same integers.

The kernel's algorithmic reads of S are the packed cells (8 bytes per
component and pair) once per block row of 32 replicates.

    python scripts/resample_bench.py [--samples 32] [--cliques 50000] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rna_clique_amd import _native as nat   # noqa: E402
from rna_clique_amd.engine import Engine   # noqa: E402
from rna_clique_amd.similarity import bootstrap_weights   # noqa: E402

REPS_PER_BLOCK = 32   # components.hip: RS_WAVES * RS_REPS


def clique_records(n_samples, n_cliques, pair_order, seed=0):
    """Pair-major records of n_cliques complete cliques over all samples."""
    rng = np.random.default_rng(seed)
    k = np.arange(n_cliques, dtype=np.uint32)
    arr = np.zeros(len(pair_order) * n_cliques, dtype=nat.EDGE_RECORD_DTYPE)
    for p, (a, b) in enumerate(pair_order):
        blk = arr[p * n_cliques:(p + 1) * n_cliques]
        blk["a"] = a * n_cliques + k
        blk["b"] = b * n_cliques + k
        blk["pair"] = p
        num = rng.integers(200, 3000, size=n_cliques, dtype=np.int32)
        blk["nident"] = num
        blk["den"] = num + rng.integers(0, 60, size=n_cliques, dtype=np.int32)
    return arr


def median_time(fn, runs, before=None):
    ts = []
    for i in range(runs + 1):   # the first run is the warm-up
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:])


def host_product(W, S_num, S_den, threads=16):
    """W @ S for both tables in int64, replicate rows split over threads."""
    W64 = W.astype(np.int64)
    cuts = np.array_split(np.arange(W.shape[0]), min(threads, W.shape[0]))
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda r: (W64[r] @ S_num, W64[r] @ S_den), cuts))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--cliques", type=int, default=50000)
    ap.add_argument("--reps", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, C = a.samples, a.cliques
    eng = Engine(device=0)
    for s in range(N):
        eng.add_sample(f"S{s:02d}", np.zeros(0, np.uint8), np.zeros(C + 1, np.uint64),
                       np.arange(1, C + 1, dtype=np.int32), np.ones(C, np.int32))
    recs = clique_records(N, C, eng.pair_order()).view(np.uint8)
    P = N * (N - 1) // 2
    say(f"resample_bench: {N} samples x {C} ideal cliques, {P} pairs, {P * C} records")
    t_build = median_time(eng.n_components, 5, before=lambda: eng.import_edges(recs))
    assert eng.n_components() == C
    say(f"table build (ranks, members, sums, packed cells): {t_build * 1e3:.2f} ms "
        f"({16 * C * P / 1e6:.0f} MB of 64-bit sums + {8 * C * P / 1e6:.0f} MB packed)")
    S_num, S_den = eng.component_sums()
    for R in a.reps:
        W = bootstrap_weights(C, R, seed=R)
        kern = []

        def call():
            eng.resample(W)
            kern.append(eng.timings()["resample_ms"])
        t_call = median_time(call, 5)
        t_kern = statistics.median(kern[1:]) * 1e-3
        tiles = (R + REPS_PER_BLOCK - 1) // REPS_PER_BLOCK
        s_bytes = tiles * C * P * 8
        macs = 2.0 * R * C * P
        say(f"R = {R}: rc_resample call {t_call * 1e3:.2f} ms; product kernel {t_kern * 1e3:.3f} ms = "
            f"{s_bytes / t_kern / 1e9:.1f} GB/s over its {s_bytes / 1e9:.2f} GB of algorithmic reads of S, "
            f"{macs / t_kern / 1e12:.2f} T multiply-adds/s (zero weights: {float((W == 0).mean()):.3f})")
        host = []
        t_host = median_time(lambda: host.append(host_product(W, S_num, S_den)), 3)
        _, _, (gn, gd) = eng.resample(W, sums=True)
        same = np.array_equal(gn, host[-1][0]) and np.array_equal(gd, host[-1][1])
        say(f"R = {R}: host int64 product on 16 threads {t_host * 1e3:.1f} ms "
            f"({t_host / t_call:.1f}x the GPU call, {t_host / t_kern:.0f}x the kernel); same integers: {same}")
        if not same:
            raise SystemExit("GPU and host products differ")
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
