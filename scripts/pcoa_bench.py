"""Time principal coordinates on the GPU (rc_pcoa, rc_resample_pcoa) against
what a user had before them.

R = 1000 replicate matrices at 32 and at 128 samples, those of
scripts/nj_bench.py: one additive birth-death tree per size, every distance of
a replicate scaled by its own factor in [0.7, 1.3]. For each size, median of 5
calls after one warm-up:

* Engine.pcoa(matrices, 3): the wall time of the call (upload of R x N x N
  doubles, kernel, copy back) and the kernel alone (rc_timing.pcoa_ms, device
  events), the sweeps per matrix, and from them the LDS traffic of the
  rotations (two columns read and written per rotation) over the kernel time;
* a graph-only engine of that many samples (pair-major ideal cliques):
  resample_pcoa(W, k=3) for 1000 bootstrap rows, where the matrices stay on
  the device, against bootstrap_dissimilarity_matrices plus a host loop of
  numpy.linalg.eigh over the first --host-reps matrices, scaled to 1000.

The first 4 results are checked against numpy.linalg.eigh within the tests'
bound before any time is reported.

    python scripts/pcoa_bench.py [--out FILE]
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

import nj_cases as nc   # noqa: E402
import pcoa_oracle as po   # noqa: E402
from nj_bench import clique_engine, median_time   # noqa: E402
from rna_clique_amd.engine import Engine   # noqa: E402
from rna_clique_amd.pcoa import eigh_eigen   # noqa: E402
from rna_clique_amd.similarity import SampleSimilarity, bootstrap_weights   # noqa: E402


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
        say(f"pcoa_bench: {R} matrices of {N} samples ({Ds.nbytes / 1e6:.0f} MB)")
        eng = Engine(device=0)
        kern, res = [], []

        def call():
            res.append(eng.pcoa(Ds, 3))
            kern.append(eng.timings()["pcoa_ms"])
        t_call = median_time(call)
        k_ms = statistics.median(kern[1:])
        sw = res[-1].sweeps
        # every sweep but a matrix's last rotates (nearly) every pair: 2 columns of N doubles read and written
        rot = float((sw - 1).sum()) * N * (N - 1) / 2
        say(f"  rc_pcoa: call {t_call * 1e3:.2f} ms, kernel {k_ms:.3f} ms; sweeps per matrix min {sw.min()} "
            f"mean {sw.mean():.2f} max {sw.max()}; about {rot:.3g} rotations = {rot * 4 * N * 8 / 1e9:.2f} GB of LDS "
            f"reads and writes = {rot * 4 * N * 8 / 1e9 / (k_ms / 1e3) / 1e3:.2f} TB/s over the kernel time")
        full = eng.pcoa(Ds[:4])
        worst = max(max(po.errors(Ds[r], full.values[r], full.vectors[r])) for r in range(4))
        say(f"    first 4 results against numpy.linalg.eigh: worst error {worst:.2f} units (bound {po.TOL_UNITS})")
        if not worst <= po.TOL_UNITS:
            raise SystemExit("GPU principal coordinates outside the bound")
        eng.close()
        # the engine path and what a user had before it
        eng = clique_engine(N, a.cliques)
        sim = SampleSimilarity.from_engine(eng)
        C = eng.n_components()
        W = bootstrap_weights(C, R, seed=N)
        kern = []

        def boot():
            eng.resample_pcoa(W, None, 3)
            kern.append((eng.timings()["resample_ms"], eng.timings()["pcoa_ms"]))
        t_boot = median_time(boot)
        say(f"  engine of {N} samples x {C} components: resample_pcoa({R} bootstrap rows, k=3) call "
            f"{t_boot * 1e3:.2f} ms (product kernel {statistics.median(k[0] for k in kern[1:]):.3f} ms, "
            f"eigensolver kernel {statistics.median(k[1] for k in kern[1:]):.3f} ms)")
        t_mats = median_time(lambda: sim.resampled_dissimilarity_matrices(W), 3)
        mats = sim.resampled_dissimilarity_matrices(W)[:a.host_reps]
        t0 = time.perf_counter()
        for m in mats:
            eigh_eigen(m, 3)
        t_eigh = (time.perf_counter() - t0) / len(mats) * R
        say(f"  before: resampled matrices to the host {t_mats * 1e3:.1f} ms + a host loop of numpy.linalg.eigh over "
            f"{R} matrices (timed on {len(mats)}) {t_eigh * 1e3:.0f} ms = {(t_mats + t_eigh) / t_boot:.1f}x the "
            f"resample_pcoa call")
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
