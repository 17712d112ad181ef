"""Time the census of replicate trees' splits and their Robinson-Foulds
distances on the GPU (rc_split_census, rc_tree_rf) against the host route on
the same trees.

R = 1000 replicate matrices at 128 and at 1024 samples: one additive
coalescent tree per size (random merges at growing heights plus a random
length per leaf), every distance of a replicate scaled by its own factor in
[1 - rel, 1 + rel]. Per size, median and range of --runs rounds after one
warm-up round; every round builds the trees again (Engine.nj: that drops the
census), then times, by device events (rc_timing.split_ms) and by
time.perf_counter around the blocking call:

* the census alone: the query call that builds it, and the call that returns
  splits, counts and ids;
* the distances to the first tree, and the pairwise distances, one call each
  (the census is then already built: their split_ms is the RF kernels alone).

The host route on the trees of the last round, as Engine.nj returned them: the
download of `splits` (one more nj call with and without that output),
np.unique(axis=0) over all R x (N - 3) rows, and the set-based pairwise
distance of tests/consensus_oracle.py (a set of split keys per tree, the size
of the symmetric difference per pair) over --procs worker processes, each
taking a share of the rows. The device results are checked against both.

    python scripts/split_bench.py [--sizes 128 1024] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import multiprocessing
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def coalescent(n, seed):
    """Distances of a random additive tree over n leaves."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    groups = [np.array([i]) for i in range(n)]
    h = 0.0
    while len(groups) > 1:
        a, b = sorted(rng.choice(len(groups), size=2, replace=False))
        h += rng.exponential(1.0 / len(groups))
        D[np.ix_(groups[a], groups[b])] = 2 * h
        D[np.ix_(groups[b], groups[a])] = 2 * h
        groups[a] = np.concatenate([groups[a], groups[b]])
        groups.pop(b)
    leaf = rng.uniform(0.0, 0.5 * h / n, size=n)
    D += leaf[:, None] + leaf[None, :]
    np.fill_diagonal(D, 0.0)
    return D


def replicates(base, R, rel, seed):
    """R x N x N: base scaled entry by entry (neighbour joining reads only the
    part above the diagonal)."""
    rng = np.random.default_rng(seed)
    Ds = rng.random((R,) + base.shape)
    Ds *= 2 * rel
    Ds += 1 - rel
    Ds *= base
    return Ds


_SETS = None


def _load_sets(path):
    global _SETS
    s = np.load(path, mmap_mode="r")
    _SETS = [set(row.tobytes() for row in np.asarray(t)) for t in s]


def _rf_rows(bounds):
    lo, hi = bounds
    return [[len(_SETS[a] ^ s) for s in _SETS] for a in range(lo, hi)]


def host_pairwise(path, R, procs):
    """(seconds, (R, R) uint32) of the set-based pairwise distances over
    `procs` processes; the time includes building every process's sets."""
    t0 = time.perf_counter()
    step = (R + 4 * procs - 1) // (4 * procs)
    ctx = multiprocessing.get_context("spawn")   # workers that never open the GPU
    with ctx.Pool(procs, initializer=_load_sets, initargs=(path,)) as pool:
        rows = pool.map(_rf_rows, [(lo, min(lo + step, R)) for lo in range(0, R, step)])
    out = np.array([r for block in rows for r in block], dtype=np.uint32)
    return time.perf_counter() - t0, out


def spread(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f}-{max(xs):.3f})"


def main():
    from rna_clique_amd import _native as nat
    from rna_clique_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rel", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    R = a.reps
    vp = ctypes.c_void_p
    for N in a.sizes:
        t0 = time.perf_counter()
        Ds = replicates(coalescent(N, seed=N), R, a.rel, seed=N + 1)
        say(f"split_bench: {R} matrices of {N} samples ({Ds.nbytes / 1e6:.0f} MB, made in "
            f"{time.perf_counter() - t0:.1f} s), rel {a.rel}")
        eng = Engine(device=0)
        L = nat.lib()
        ev = {k: [] for k in ("build", "fetch", "to_ref", "pairwise")}
        wall = {k: [] for k in ev}
        nj_ms = []

        def timed(key, fn):
            t0 = time.perf_counter()
            out = fn()
            wall[key].append((time.perf_counter() - t0) * 1e3)
            ev[key].append(eng.timings()["split_ms"])
            return out
        res = census = rf = None
        for _ in range(a.runs + 1):   # the first round is the warm-up
            res = eng.nj(Ds)
            nj_ms.append(eng.timings()["nj_ms"])
            k = ctypes.c_uint64()
            timed("build", lambda: nat.check(L.rc_split_census(eng._h, None, None, None, 0, ctypes.byref(k), None)))
            census = timed("fetch", eng.split_census)
            to_ref = timed("to_ref", lambda: eng.tree_rf(res.splits[0]))[0]
            rf = timed("pairwise", lambda: eng.tree_rf(pairwise=True))[1]
        for d in (ev, wall):
            for key in d:
                d[key] = d[key][1:]
        K = len(census.counts)
        say(f"  trees: nj kernels {spread(nj_ms[1:])} ms; {K} distinct splits among {R * (N - 3)} "
            f"({int((census.counts == 1).sum())} in one replicate only, {int((census.counts > R / 2).sum())} in a majority)")
        say(f"  census built (query call): split_ms {spread(ev['build'])} ms, call {spread(wall['build'])} ms")
        say(f"  census returned (splits, counts, ids; already built): split_ms {spread(ev['fetch'])} ms, "
            f"call {spread(wall['fetch'])} ms ({(census.splits.nbytes + census.ids.nbytes) / 1e6:.1f} MB)")
        say(f"  distances to a reference tree: split_ms {spread(ev['to_ref'])} ms, call {spread(wall['to_ref'])} ms")
        say(f"  pairwise distances: split_ms {spread(ev['pairwise'])} ms, call {spread(wall['pairwise'])} ms "
            f"({rf.nbytes / 1e6:.1f} MB)")
        dev_census = statistics.median(ev["build"]) + statistics.median(ev["fetch"])
        dev_all = dev_census + statistics.median(ev["to_ref"]) + statistics.median(ev["pairwise"])
        call_census = statistics.median(wall["build"]) + statistics.median(wall["fetch"])
        call_all = call_census + statistics.median(wall["to_ref"]) + statistics.median(wall["pairwise"])
        say(f"  sums of medians: census split_ms {dev_census:.3f} ms (calls {call_census:.2f} ms); census and both "
            f"distance arrays split_ms {dev_all:.3f} ms (calls {call_all:.2f} ms)")
        # the host route
        t_with, t_without = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.nj(Ds)
            t_with.append(time.perf_counter() - t0)
            bufs = Engine._nj_buffers(R, N, None)[1]
            nv = ctypes.c_uint32()
            t0 = time.perf_counter()
            nat.check(L.rc_nj(eng._h, Ds.ctypes.data_as(vp), R, N, bufs["joins"].ctypes.data_as(vp),
                              bufs["lengths"].ctypes.data_as(vp), None, bufs["valid"].ctypes.data_as(vp), None, 0, None,
                              ctypes.byref(nv)))
            t_without.append(time.perf_counter() - t0)
        t_down = max(0.0, statistics.median(t_with) - statistics.median(t_without))
        flat = res.splits.reshape(R * (N - 3), -1)
        t0 = time.perf_counter()
        uniq, inverse, counts = np.unique(flat, axis=0, return_inverse=True, return_counts=True)
        t_unique = time.perf_counter() - t0
        same = len(uniq) == K and np.array_equal(np.sort(counts), np.sort(census.counts.astype(counts.dtype)))
        back = uniq[inverse.reshape(R, N - 3)]
        same = same and np.array_equal(census.splits[census.ids], back)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "splits.npy")
            np.save(path, res.splits)
            t_pairs, host_rf = host_pairwise(path, R, a.procs)
        same = same and np.array_equal(host_rf, rf) and np.array_equal(host_rf[0], to_ref)
        say(f"  host route: download of splits {t_down * 1e3:.1f} ms ({res.splits.nbytes / 1e6:.1f} MB; nj call with "
            f"minus without that output, median of 3), np.unique(axis=0) {t_unique:.2f} s, set-based pairwise "
            f"distances on {a.procs} processes {t_pairs:.2f} s")
        host_census = t_down + t_unique
        say(f"  ratios (host seconds over the calls' wall time): census {host_census / (call_census / 1e3):.0f}x, "
            f"census and pairwise distances {(host_census + t_pairs) / (call_all / 1e3):.0f}x")
        say(f"  device results equal the host's: {same}")
        if not same:
            raise SystemExit("device and host results differ")
        eng.close()
        del Ds
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
