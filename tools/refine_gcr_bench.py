#!/usr/bin/env python3
"""mgx_solve_refine_gcr (fp64 restarted GCR around the float cycle) next to mgx_solve_gcr and
mgx_solve_refine on the same F64 handle, and its two mixed passes next to the fp64 passes they replace, all in one process
(the tables of profiles/refine_gcr_kernel_trace_summary.md).

    python tools/refine_gcr_bench.py [--quick] [--only kernels|solves]

Kernels: at a 4096^2 finest level (--quick: 1024^2), GALERKIN fp64 handles with a five-point (contrast 10) and a nine-point
(rotated anisotropy) finest operator, HIP events around 20 launches, median of 5: k_refine_direction<5 | 9> and
k_refine_update through mgx_time_refine_gcr_pass, k_pcg_direction<double, 1 | 2> and k_pcg_update<double> through
mgx_time_gcr_pass (slot 0).  The kernels' own durations come from running this mode under `rocprofv3 --kernel-trace
--stats` (no counters in the same run), which is what the profile document quotes.  Bytes are the algorithm's: direction 60 /
92 per point against 64 / 96 (z and the NQ grids in, z and q out), update 52 against 48.  Target, guessed in advance: 0.8 of
the yardstick's bytes/s.

Solves: time to 1e-10 at 2047^2 and 4095^2 (--quick: 511^2), GALERKIN, levels L..5, fp64, b =
default_rng(3).uniform(-1, 1), zero guess: the four rows of DESIGN.md 5.4's table (contrast 10 with the operator-dependent P
and rotated anisotropy eps = 0.5 with the bilinear P; Jacobi V(2,2) and COLOR_GS V(1,1)) and rotated anisotropy eps = 0.1
and 0.01 with the operator-dependent P, Jacobi V(2,2).  solve_refine_gcr(4), solve_gcr(4) and solve_refine alternate on
ONE handle, median of 5 each after a round that captures the graphs (stats.seconds: the wall time of the call,
device-synchronised, profiler off), at most 100 iterations each."""
import os
import statistics
import sys

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
TOL, CAP, RESTART = 1e-10, 100, 4
J, GS = pkg.SMOOTHER_JACOBI, pkg.SMOOTHER_COLOR_GS


def contrast(L):
    return lambda mg: mg.set_coefficient(contrast_coefficient(L, 10.0))


def rotated(L, eps):
    return lambda mg: mg.set_tensor(*nine_ref.rotated_tensor(L, 45.0, eps))


def kernels():
    n = (1 << LK) - 1
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    print(f"\n| {1 << LK}^2 finest level, f64 | B per point | ms per launch | TB/s (of 8) | over its fp64 yardstick |\n|---|---|---|---|---|")
    for setter, transfer, nq in ((contrast(LK), pkg.TRANSFER_OPERATOR, 5), (rotated(LK, 0.5), pkg.TRANSFER_BILINEAR, 9)):
        with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            setter(mg)
            mg.build_galerkin(transfer)
            mg.set_rhs(b)
            mg.solve_refine_gcr(tol=0.0, max_iters=2, restart=1)     # the float copy and slot 0; every kernel has run once

            def med(f):
                f()
                return statistics.median(f() for _ in range(5))

            rows = [(f"`k_pcg_direction<double, {1 if nq == 5 else 2}>`", 8 * nq + 24, med(lambda: mg.time_gcr_pass(3, 0, 20)), None),
                    (f"`k_refine_direction<{nq}, 1>`", 8 * nq + 20, med(lambda: mg.time_refine_gcr_pass(1, 20)), 0),
                    ("`k_pcg_update<double>`", 48, med(lambda: mg.time_gcr_pass(0, 0, 20)), None),
                    ("`k_refine_update`", 52, med(lambda: mg.time_refine_gcr_pass(0, 20)), 2)]
        rates = [nbytes * n * n / (t * 1e-3) for _, nbytes, t, _ in rows]
        for (kernel, nbytes, t, yard), rate in zip(rows, rates):
            over = "1.00" if yard is None else f"{rate / rates[yard]:.2f}"
            print(f"| {kernel} ({nq}-point level) | {nbytes} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {over} |", flush=True)


def solves():
    for L in SIZES:
        n = (1 << L) - 1
        b = np.random.default_rng(3).uniform(-1, 1, (n, n))
        zero = np.zeros((n, n))
        print(f"\n| {n}^2, levels {L}..5, to {TOL:g} | P | cycle | solve_gcr(4): iterations, ms | solve_refine: cycles, ms | "
              "solve_refine_gcr(4): iterations, ms | over solve_gcr | over solve_refine |")
        print("|---|---|---|---|---|---|---|---|")
        problems = [("contrast 10", "OPERATOR", contrast(L), pkg.TRANSFER_OPERATOR, "Jacobi V(2,2)", J, 2),
                    ("contrast 10", "OPERATOR", contrast(L), pkg.TRANSFER_OPERATOR, "COLOR_GS V(1,1)", GS, 1),
                    ("rotated anisotropy 45 degrees, eps = 0.5", "BILINEAR", rotated(L, 0.5), pkg.TRANSFER_BILINEAR, "Jacobi V(2,2)", J, 2),
                    ("rotated anisotropy 45 degrees, eps = 0.5", "BILINEAR", rotated(L, 0.5), pkg.TRANSFER_BILINEAR, "COLOR_GS V(1,1)", GS, 1),
                    ("rotated anisotropy 45 degrees, eps = 0.1", "OPERATOR", rotated(L, 0.1), pkg.TRANSFER_OPERATOR, "Jacobi V(2,2)", J, 2),
                    ("rotated anisotropy 45 degrees, eps = 0.01", "OPERATOR", rotated(L, 0.01), pkg.TRANSFER_OPERATOR, "Jacobi V(2,2)", J, 2)]
        for what, tname, setter, transfer, label, sm, mu in problems:
            cfg = dict(finest_level=L, coarsest_level=5, mu1=mu, mu2=mu, schedule=0, op=pkg.OP_GALERKIN, smoother=sm)
            with pkg.Multigrid(**cfg) as mg:
                setter(mg)
                mg.build_galerkin(transfer)
                mg.set_rhs(b)
                calls = (lambda: mg.solve_gcr(tol=TOL, max_iters=CAP, restart=RESTART), lambda: mg.solve_refine(tol=TOL, max_cycles=CAP),
                         lambda: mg.solve_refine_gcr(tol=TOL, max_iters=CAP, restart=RESTART))
                times, last = [[], [], []], [None] * 3
                for rep in range(6):                            # the first round captures the graphs: not timed
                    for i, f in enumerate(calls):
                        mg.set_guess(zero)
                        st, hist = f()
                        last[i] = (st, hist)
                        if rep:
                            times[i].append(st.seconds * 1e3)
            ms = [statistics.median(t) for t in times]

            def cell(i):
                st, hist = last[i]
                end = "" if st.converged else f", NOT converged ({hist[-1] / hist[0]:.1e})"
                return f"{st.cycles}, {ms[i]:.2f} ms (min {min(times[i]):.2f}, max {max(times[i]):.2f}){end}"

            print(f"| {what} | {tname} | {label} | {cell(0)} | {cell(1)} | {cell(2)} | {ms[2] / ms[0]:.2f} | {ms[2] / ms[1]:.2f} |", flush=True)


if __name__ == "__main__":
    if ONLY in ("", "kernels"):
        kernels()
    if ONLY in ("", "solves"):
        solves()
