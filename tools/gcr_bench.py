#!/usr/bin/env python3
"""mgx_solve_gcr (restarted GCR around one cycle) next to mgx_solve and mgx_solve_pcg, and its kernels
next to k_pcg_update, all in one process (the tables of profiles/gcr_kernel_trace_summary.md).

    python tools/gcr_bench.py [--quick] [--only kernels|solves] [--level L]

Solves: time to 1e-8 at 2047^2 (--quick: 511^2; --level L: (2^L - 1)^2), GALERKIN, bilinear P, levels L..5, fp64, b = default_rng(3).uniform(-1, 1),
zero guess, median of 5 after a run that captures the graphs: the x-strong problem (eps = 1e-2) with LINE_X V(1,1), the
layers problem (eps = 1e-2) with LINE_ALT V(1,1), both also with Jacobi V(2,2), and upwind convection-diffusion
(a = (1, 0.5), cell Peclet number 1) with LINE_ALT V(1,1) and Jacobi V(2,2); mgx_solve (cap 100), mgx_solve_pcg (cap 300),
mgx_solve_gcr with restart 4 and 8 (cap 300).

Kernels: mgx_time_gcr_pass at 4095^2 (--quick: 1023^2; a vector is 134 MB in fp64, so that no pass's working set fits
the 256 MB last-level cache) in fp64 and fp32 - HIP events around 20 launches, median of 5 - of
k_pcg_update (6 sizeof(T) per point: the yardstick), k_gcr_dots<J> ((1 + J) sizeof(T)), k_gcr_orth<J> ((5 + 2J) sizeof(T),
J = 0: 2 sizeof(T)) and k_pcg_direction (4 sizeof(T) + 5 sizeof(T) of coefficients); bytes are the algorithm's, no
counter run is made.  The last column is the pass's bytes/s over k_pcg_update's of the same run (target: at least 0.8)."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
import gcr_ref  # noqa: E402
import line_ref  # noqa: E402

pkg = ge.load_package()
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
L = int(sys.argv[sys.argv.index("--level") + 1]) if "--level" in sys.argv else 9 if QUICK else 11
N = (1 << L) - 1
LK = 10 if QUICK else 12
NK = (1 << LK) - 1
UPDATE, DOTS, ORTH, DIRECTION = 0, 1, 2, 3


def problems():
    yield "x-strong, eps = 1e-2", line_ref.aniso_stencil(L, 1e-2, "x"), (("LINE_X V(1,1)", pkg.SMOOTHER_LINE_X, 1),)
    yield "layers, eps = 1e-2", line_ref.aniso_stencil(L, 1e-2, "layers"), (("LINE_ALT V(1,1)", pkg.SMOOTHER_LINE_ALT, 1),)
    yield "upwind a = (1, 0.5), Peclet 1", gcr_ref.upwind_stencil(L, (1.0, 0.5), 1.0), (("LINE_ALT V(1,1)", pkg.SMOOTHER_LINE_ALT, 1),)


def cell(mg, f):
    ts = []
    for rep in range(6):                                # the first run captures the graphs: not timed
        mg.set_guess(np.zeros((N, N)))
        st, hist = f()
        if rep:
            ts.append(st.seconds * 1e3)
    end = "" if st.converged else f", NOT converged, residual ratio {hist[-1] / hist[0]:.1e}"
    return f"{st.cycles}, {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}){end}"


def solves():
    b = np.random.default_rng(3).uniform(-1, 1, (N, N))
    print(f"\n| {N}^2, levels {L}..5, f64, BILINEAR | cycle | mgx_solve (cap 100) | mgx_solve_pcg (cap 300) | mgx_solve_gcr(4) | mgx_solve_gcr(8) |")
    print("|---|---|---|---|---|---|")
    for what, st5, smoothers in problems():
        for label, sm, mu in smoothers + (("Jacobi V(2,2), omega = 2/3", pkg.SMOOTHER_JACOBI, 2),):
            with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=mu, mu2=mu, schedule=0, op=pkg.OP_GALERKIN, smoother=sm) as mg:
                mg.set_stencil(L, *st5)
                mg.build_galerkin()
                mg.set_rhs(b)
                cells = [cell(mg, f) for f in (lambda: mg.solve(tol=1e-8, max_cycles=100), lambda: mg.solve_pcg(tol=1e-8, max_iters=300),
                                               lambda: mg.solve_gcr(tol=1e-8, max_iters=300, restart=4),
                                               lambda: mg.solve_gcr(tol=1e-8, max_iters=300, restart=8))]
            print(f"| {what} | {label} | " + " | ".join(cells) + " |", flush=True)


def kernels():
    st5 = line_ref.aniso_stencil(LK, 1e-2, "layers")
    b = np.random.default_rng(3).uniform(-1, 1, (NK, NK))
    for dtype, name, size in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, dtype=dtype) as mg:
            mg.set_stencil(LK, *[a.astype(np.float64 if size == 8 else np.float32) for a in st5])
            mg.build_galerkin()
            mg.set_rhs(b)
            mg.solve_gcr(tol=0.0, max_iters=9, restart=8)          # allocates the eight pairs, every kernel has run once

            def ms(which, j):
                return statistics.median(mg.time_gcr_pass(which, j, 20) for _ in range(5))

            rows = [("k_pcg_update", 6, ms(UPDATE, 0)), ("k_pcg_direction<T, 1>", 9, ms(DIRECTION, 0))]
            rows += [(f"k_gcr_dots<T, {j}>", 1 + j, ms(DOTS, j)) for j in range(1, 8)]
            rows += [(f"k_gcr_orth<T, {j}>", 5 + 2 * j if j else 2, ms(ORTH, j)) for j in range(8)]
        rate0 = 6 * size * NK * NK / (rows[0][2] * 1e-3)
        print(f"\n| {NK}^2, {name} | sizeof(T) per point | ms per launch | TB/s (of 8) | over k_pcg_update |\n|---|---|---|---|---|")
        for kernel, words, t in rows:
            rate = words * size * NK * NK / (t * 1e-3)
            print(f"| `{kernel}` | {words} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate0:.2f} |", flush=True)


if __name__ == "__main__":
    if ONLY in ("", "kernels"):
        kernels()
    if ONLY in ("", "solves"):
        solves()
