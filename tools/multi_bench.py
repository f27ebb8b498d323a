#!/usr/bin/env python3
"""mgx_solve_multi (up to four right-hand sides per operator read) next to four mgx_solve calls on the same
handle, and its K-column Jacobi sweep next to the K = 1 sweep, all in one process (the tables of
profiles/multi_rhs_kernel_trace_summary.md).

    python tools/multi_bench.py [--quick] [--only kernels|solves]

Kernels: at a 4096^2 finest level (--quick: 1024^2), GALERKIN fp64 and fp32 handles with a five-point (contrast 10) and a
nine-point (rotated anisotropy) finest operator: mgx_time_multi_smoother - HIP events around 20 sweeps, median of 5 -
for nrhs = 1 (k_jacobi_var<T, NQ, 1> on a workspace column, the yardstick of the same run) and nrhs = 2, 3, 4
(k_jacobi_var<T, NQ, K>).  Bytes are the algorithm's: (NQ + 3 K) sizeof(T) per point; no counter run is made.
Target: the K = 4 instances move their bytes at 0.8 of the K = 1 instance's bytes/s.

Solves: time to 1e-8 at 2047^2 and 4095^2 (--quick: 511^2), GALERKIN, levels L..5, fp64, Jacobi V(2,2), four columns
b_j = default_rng(3 + j).uniform(-1, 1) from zero guesses; contrast 10 with the operator-dependent P and rotated
anisotropy (45 degrees, eps = 0.5) with the bilinear P.  One solve_multi call against four set_rhs / set_guess / solve /
get_solution rounds on ONE handle, alternating, median of 5 each after a pair that captures the graphs and allocates the
columns; both on the host clock around everything the caller waits for (the copies of b and u in, the solves, the copies
of u out, device-synchronised)."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
import nine_ref  # noqa: E402
from pcg_ref import contrast_coefficient  # noqa: E402

pkg = ge.load_package()
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
LK = 10 if QUICK else 12
SIZES = (9,) if QUICK else (11, 12)
TOL = 1e-8


def problems(L):
    yield "contrast 10", "OPERATOR", (lambda mg: mg.set_coefficient(contrast_coefficient(L, 10.0))), pkg.TRANSFER_OPERATOR, 5
    yield ("rotated anisotropy 45 degrees, eps = 0.5", "BILINEAR", (lambda mg: mg.set_tensor(*nine_ref.rotated_tensor(L, 45.0, 0.5))),
           pkg.TRANSFER_BILINEAR, 9)


def kernels():
    n = (1 << LK) - 1
    print(f"\n| {1 << LK}^2 finest level | nrhs | B per point | ms per sweep | TB/s (of 8) | over nrhs = 1 | ms per column, over nrhs = 1 |")
    print("|---|---|---|---|---|---|---|")
    for dtype, tname, es in ((pkg.DTYPE_F64, "double", 8), (pkg.DTYPE_F32, "float", 4)):
        for what, _, setter, transfer, nq in problems(LK):
            with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, dtype=dtype) as mg:
                setter(mg)
                mg.build_galerkin(transfer)
                b = np.random.default_rng(3).uniform(-1, 1, (4, n, n))
                mg.solve_multi(b, tol=0.0, max_cycles=1)             # allocates four columns, every kernel has run once
                del b
                rate1 = t1 = None
                for nrhs in (1, 2, 3, 4):
                    mg.time_multi_smoother(nrhs, 20)
                    t = statistics.median(mg.time_multi_smoother(nrhs, 20) for _ in range(5)) / 20
                    nbytes = es * (nq + 3 * nrhs)
                    rate = nbytes * n * n / (t * 1e-3)
                    if nrhs == 1:
                        rate1, t1 = rate, t
                    kernel = f"`k_jacobi_var<{tname}, {nq}, {nrhs}>`"
                    print(f"| {kernel} | {nrhs} | {nbytes} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate1:.2f} | "
                          f"{t / nrhs:.4f}, {t / nrhs / t1:.2f} |", flush=True)


def solves():
    for L in SIZES:
        n = (1 << L) - 1
        b = np.stack([np.random.default_rng(3 + j).uniform(-1, 1, (n, n)) for j in range(4)])
        zero = np.zeros((n, n))
        print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), to {TOL:g} | P | cycles per column | four solve calls, ms | one solve_multi call, ms | "
              "multi / four | same bits |")
        print("|---|---|---|---|---|---|---|")
        for what, tname, setter, transfer, _ in problems(L):
            cfg = dict(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN)
            with pkg.Multigrid(**cfg) as mg:
                setter(mg)
                mg.build_galerkin(transfer)
                ts, tm = [], []
                for rep in range(6):                            # the first pair captures the graphs and allocates: not timed
                    mg.synchronize()
                    t0 = time.perf_counter()
                    seq = []
                    for j in range(4):
                        mg.set_rhs(b[j])
                        mg.set_guess(zero)
                        st, hist = mg.solve(tol=TOL, max_cycles=100)
                        seq.append((st, hist, mg.get_solution()))
                    t1 = time.perf_counter()
                    stats, hists, u = mg.solve_multi(b, tol=TOL, max_cycles=100)
                    t2 = time.perf_counter()
                    if rep:
                        ts.append((t1 - t0) * 1e3)
                        tm.append((t2 - t1) * 1e3)
                same = all(np.array_equal(u[j], seq[j][2]) and np.array_equal(hists[j], seq[j][1]) for j in range(4))
                ms_s, ms_m = statistics.median(ts), statistics.median(tm)
                conv = "" if all(st.converged for st in stats) else " (NOT all converged)"
                print(f"| {what} | {tname} | {[st.cycles for st in stats]}{conv} | {ms_s:.2f} (min {min(ts):.2f}, max {max(ts):.2f}) | "
                      f"{ms_m:.2f} (min {min(tm):.2f}, max {max(tm):.2f}) | {ms_m / ms_s:.2f} | {'yes' if same else 'NO'} |", flush=True)
                # the device's share: stats.seconds of the calls (host copies of the columns excluded for solve)
                print(f"|   of which in the solve loops: four solves {sum(s[0].seconds for s in seq) * 1e3:.2f} ms, solve_multi "
                      f"{stats[0].seconds * 1e3:.2f} ms (its copies included) | | | | | | |", flush=True)


if __name__ == "__main__":
    if ONLY in ("", "kernels"):
        kernels()
    if ONLY in ("", "solves"):
        solves()
