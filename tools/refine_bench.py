#!/usr/bin/env python3
"""mgx_solve_refine (fp64 defect correction around the float cycle) next to mgx_solve on the same F64
handle and on an F32 handle, and its pass next to the residual-norm kernel, all in one process (the tables of
profiles/refine_kernel_trace_summary.md).

    python tools/refine_bench.py [--quick] [--only kernels|solves]

Kernels: at a 4096^2 finest level (--quick: 1024^2; a vector is 134 MB in fp64, beyond the 256 MB last-level cache for
every pass here), GALERKIN fp64 handles with a five-point (contrast 10) and a nine-point (rotated anisotropy) finest
operator: k_refine_pass<NQ, true> through mgx_time_refine_pass - HIP events around 20 launches, median of 5, each launch
followed by its k_reduce_partials - and k_residual_var<double, NQ, 1> through mgx_residual_norm - a host clock around 20
calls, median of 5, each call with its k_reduce_partials, an 8-byte copy and a synchronisation.  Those are upper bounds of
the kernels' times; the kernels' own durations come from running this mode under `rocprofv3 --kernel-trace --stats`,
which is what the profile document quotes.  Bytes are the algorithm's: 72 / 104 per point for the pass (NQ = 5 / 9), 56 /
88 for the norm (u, b and the NQ grids in, nothing out); no counter run is made.  Target: the pass at 0.8 of the norm
kernel's bytes/s.

Solves: time to 1e-10 at 2047^2 and 4095^2 (--quick: 511^2), GALERKIN, levels L..5, fp64, b =
default_rng(3).uniform(-1, 1), zero guess; contrast 10 with the operator-dependent P and rotated anisotropy (45 degrees,
eps = 0.5) with the bilinear P; Jacobi V(2,2) and COLOR_GS V(1,1).  solve_refine and solve alternate on ONE handle,
median of 5 each after a pair that captures the graphs (stats.seconds: the wall time of the call, device-synchronised,
profiler off).  Then an F32 handle of the same configuration: the relative residual its solve stalls at in as many
cycles, and its time per cycle."""
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
TOL = 1e-10


def problems(L):
    yield "contrast 10", "OPERATOR", (lambda mg: mg.set_coefficient(contrast_coefficient(L, 10.0))), pkg.TRANSFER_OPERATOR, 5
    yield ("rotated anisotropy 45 degrees, eps = 0.5", "BILINEAR", (lambda mg: mg.set_tensor(*nine_ref.rotated_tensor(L, 45.0, 0.5))),
           pkg.TRANSFER_BILINEAR, 9)


def kernels():
    n = (1 << LK) - 1
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    print(f"\n| {1 << LK}^2 finest level, f64 | B per point | ms per launch | TB/s (of 8) | over k_residual_var |\n|---|---|---|---|---|")
    for what, _, setter, transfer, nq in problems(LK):
        with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            setter(mg)
            mg.build_galerkin(transfer)
            mg.set_rhs(b)
            mg.solve_refine(tol=0.0, max_cycles=2)                 # creates the float copy, every kernel has run once
            t_pass = statistics.median(mg.time_refine_pass(20) for _ in range(5))

            def norm_ms():
                mg.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    mg.residual_norm()
                return (time.perf_counter() - t0) * 1e3 / 20

            norm_ms()
            t_norm = statistics.median(norm_ms() for _ in range(5))
        rows = [(f"`k_residual_var<double, {nq}, 1>` + reduction, copy and synchronisation (host clock)", 8 * (nq + 2), t_norm),
                (f"`k_refine_pass<{nq}, true>` + reduction (HIP events)", 8 * nq + 32, t_pass)]
        rate0 = rows[0][1] * n * n / (t_norm * 1e-3)
        for kernel, nbytes, t in rows:
            rate = nbytes * n * n / (t * 1e-3)
            print(f"| {kernel} | {nbytes} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate0:.2f} |", flush=True)


def timed(mg, n, f):
    mg.set_guess(np.zeros((n, n), dtype=mg.level_dtype(mg.cfg.finest_level)))
    st, hist = f()
    return st, hist


def solves():
    for L in SIZES:
        n = (1 << L) - 1
        b = np.random.default_rng(3).uniform(-1, 1, (n, n))
        print(f"\n| {n}^2, levels {L}..5, to {TOL:g} | P | cycle | solve (f64): cycles, ms | solve_refine: cycles, ms | refine / solve | "
              "F32 handle: stalls at, ms per cycle |")
        print("|---|---|---|---|---|---|---|")
        for what, tname, setter, transfer, _ in problems(L):
            for label, sm, mu in (("Jacobi V(2,2)", pkg.SMOOTHER_JACOBI, 2), ("COLOR_GS V(1,1)", pkg.SMOOTHER_COLOR_GS, 1)):
                cfg = dict(finest_level=L, coarsest_level=5, mu1=mu, mu2=mu, schedule=0, op=pkg.OP_GALERKIN, smoother=sm)
                with pkg.Multigrid(**cfg) as mg:
                    setter(mg)
                    mg.build_galerkin(transfer)
                    mg.set_rhs(b)
                    ts, tr = [], []
                    for rep in range(6):                        # the first pair captures the graphs: not timed
                        sr, hr = timed(mg, n, lambda: mg.solve_refine(tol=TOL, max_cycles=100))
                        ss, hs = timed(mg, n, lambda: mg.solve(tol=TOL, max_cycles=100))
                        if rep:
                            tr.append(sr.seconds * 1e3)
                            ts.append(ss.seconds * 1e3)
                with pkg.Multigrid(dtype=pkg.DTYPE_F32, **cfg) as f32:
                    setter(f32)
                    f32.build_galerkin(transfer)
                    f32.set_rhs(b.astype(np.float32))
                    t32 = []
                    for rep in range(4):
                        s32, h32 = timed(f32, n, lambda: f32.solve(tol=0.0, max_cycles=ss.cycles))
                        if rep:
                            t32.append(s32.seconds * 1e3 / max(s32.cycles, 1))
                ms_s, ms_r = statistics.median(ts), statistics.median(tr)

                def cell(st, hist, ms, t):
                    end = "" if st.converged else f", NOT converged ({hist[-1] / hist[0]:.1e})"
                    return f"{st.cycles}, {ms:.2f} ms (min {min(t):.2f}, max {max(t):.2f}){end}"

                print(f"| {what} | {tname} | {label} | {cell(ss, hs, ms_s, ts)} | {cell(sr, hr, ms_r, tr)} | {ms_r / ms_s:.2f} | "
                      f"{np.min(h32) / h32[0]:.1e}, {statistics.median(t32):.3f} (f64: {ms_s / max(ss.cycles, 1):.3f}, refine: "
                      f"{ms_r / max(sr.cycles, 1):.3f}) |", flush=True)


if __name__ == "__main__":
    if ONLY in ("", "kernels"):
        kernels()
    if ONLY in ("", "solves"):
        solves()
