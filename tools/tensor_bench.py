#!/usr/bin/env python3
"""Nine-point finest operators (mgx_set_tensor): the finest-level kernels next to the same instances on a
coarse level, the nine-point Krylov direction pass next to the five-point one, and the time to 1e-8 on the rotated
anisotropy problem - all in one process (the tables of profiles/tensor_kernel_trace_summary.md).

    python tools/tensor_bench.py [--quick] [--only kernels|direction|solves] [--theta DEG]

The tensor: principal values 1 and eps, the strong direction at angle theta (default 45 degrees) to the x axis:
axx = cos^2 + eps sin^2, ayy = sin^2 + eps cos^2, axy = (1 - eps) sin cos.

Kernels (4096^2; --quick: 512^2): k_jacobi_var<T, 9> (40 sweeps per timed call) and k_residual_var<T, 9, 0> (20 passes,
one host synchronise each) on a nine-point FINEST level 12, and on level 12 of a 13..5 hierarchy built from a scalar
coefficient, where the same instances run on a coarse level (the configuration of profiles/galerkin_kernel_trace_summary.md).
Wall time around calls that end in a device synchronise, median of 5; bytes are the algorithm's: 12 sizeof(T) per point.

Direction (4095^2; --quick: 1023^2): mgx_time_gcr_pass(DIRECTION) on a nine-point finest level (k_pcg_direction<T, 2>,
13 sizeof(T) per point) and on a five-point one (k_pcg_direction<T, 1>, 9 sizeof(T)), with k_pcg_update (6 sizeof(T)) of
the same handle - HIP events around 20 launches, median of 5.  The yardstick: bytes/s of <T, 2> over bytes/s of <T, 1>,
target at least 0.8.

Solves (2047^2, levels 11..5, fp64; --quick: 511^2): eps = 0.5, 0.1, 0.01; Jacobi V(2,2) (omega = 2/3) and LINE_ALT V(1,1);
bilinear and operator-dependent P; mgx_solve and mgx_solve_gcr(restart 4), cap 100 cycles each; b = default_rng(3).uniform(-1, 1),
zero guess; median of 5 after a run that captures the graphs."""
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
THETA = float(sys.argv[sys.argv.index("--theta") + 1]) if "--theta" in sys.argv else 45.0
LK = 9 if QUICK else 12
LS = 9 if QUICK else 11
UPDATE, DIRECTION = 0, 3


def tensor(level, theta_deg, eps):
    c, s = math.cos(math.radians(theta_deg)), math.sin(math.radians(theta_deg))
    shape = ((1 << level) + 1,) * 2
    return np.full(shape, c * c + eps * s * s), np.full(shape, (1.0 - eps) * s * c), np.full(shape, s * s + eps * c * c)


def wall(f, reps=5):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def kernels():
    n = (1 << LK) - 1
    rng = np.random.default_rng(0)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    x = np.linspace(0.0, 1.0, (1 << (LK + 1)) + 1)
    a = 1.0 + 0.8 * np.sin(3 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    print("\n| kernel | that level is | dtype | ms per pass | bytes per point | achieved GB/s | fraction of the 8 TB/s HBM peak |")
    print("|---|---|---|---|---|---|---|")
    rate = {}
    for dtype, name, es in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        for where, finest in (("the finest level (mgx_set_tensor)", LK), ("a coarse level (R A P)", LK + 1)):
            with pkg.Multigrid(finest_level=finest, coarsest_level=5, mu1=2, mu2=2, schedule=pkg.SCHEDULE_V, op=pkg.OP_GALERKIN, dtype=dtype, omega=0.8) as mg:
                if finest == LK:
                    mg.set_tensor(*tensor(LK, THETA, 0.5))
                else:
                    mg.set_coefficient(a)
                mg.build_galerkin()
                mg.set_level(LK, pkg.VEC_U, u)
                mg.set_level(LK, pkg.VEC_B, b)
                mg.smooth(LK, 4)
                sweeps = 40
                ms = wall(lambda: mg.smooth(LK, sweeps)) / sweeps
                gbs = 12 * es * n * n / (ms * 1e-3) / 1e9
                rate["jacobi", name, finest == LK] = gbs
                print(f"| k_jacobi_var<{name}, 9> | {where} | {name} | {ms:.4f} | {12 * es} | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
                mg.residual(LK, u, b)
                lib, h = pkg.lib(), mg._h

                def res20():
                    for _ in range(20):
                        lib.mgx_residual(h, LK)
                ms = wall(res20) / 20
                gbs = 12 * es * n * n / (ms * 1e-3) / 1e9
                rate["residual", name, finest == LK] = gbs
                print(f"| k_residual_var<{name}, 9, 0> (one host synchronise per pass) | {where} | {name} | {ms:.4f} | {12 * es} | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
    for k in ("jacobi", "residual"):
        for name in ("f64", "f32"):
            print(f"k_{k}_var<{name}, 9> on the finest level over the same instance on a coarse level, bytes/s: {rate[k, name, True] / rate[k, name, False]:.3f}")


def direction():
    LD = 10 if QUICK else 12
    n = (1 << LD) - 1
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    print(f"\n| {n}^2 | dtype | sizeof(T) per point | ms per launch | TB/s | over k_pcg_update |\n|---|---|---|---|---|---|")
    for dtype, name, es in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        rates = {}
        for op in (2, 1):
            with pkg.Multigrid(finest_level=LD, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, dtype=dtype) as mg:
                axx, axy, ayy = tensor(LD, THETA, 0.5)
                if op == 2:
                    mg.set_tensor(axx, axy, ayy)
                else:
                    mg.set_coefficient(axx)
                mg.build_galerkin()
                mg.set_rhs(b)
                mg.solve_gcr(tol=0.0, max_iters=2, restart=1)          # allocates the pair, every kernel has run once

                def ms(which):
                    return statistics.median(mg.time_gcr_pass(which, 0, 20) for _ in range(5))
                words = 4 + (9 if op == 2 else 5)
                t_dir, t_upd = ms(DIRECTION), ms(UPDATE)
                r_dir, r_upd = words * es * n * n / (t_dir * 1e-3), 6 * es * n * n / (t_upd * 1e-3)
                rates[op] = r_dir
                print(f"| `k_pcg_direction<{name}, {op}>` | {name} | {words} | {t_dir:.4f} | {r_dir / 1e12:.2f} | {r_dir / r_upd:.2f} |")
                print(f"| `k_pcg_update<{name}>` (same handle) | {name} | 6 | {t_upd:.4f} | {r_upd / 1e12:.2f} | 1.00 |", flush=True)
        print(f"k_pcg_direction<{name}, 2> over k_pcg_direction<{name}, 1>, bytes/s: {rates[2] / rates[1]:.3f} (target: at least 0.8)")


def cell(mg, n, f):
    ts = []
    for rep in range(6):                                # the first run captures the graphs: not timed
        mg.set_guess(np.zeros((n, n)))
        st, hist = f()
        if rep:
            ts.append(st.seconds * 1e3)
    end = "" if st.converged else f", NOT converged, residual ratio {hist[-1] / hist[0]:.1e}"
    return f"{st.cycles}, {statistics.median(ts):.2f} ms{end}"


def solves():
    n = (1 << LS) - 1
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    print(f"\n| {n}^2, levels {LS}..5, f64, theta = {THETA:g} | eps | cycle | P | mgx_solve: cycles, time (cap 100) | mgx_solve_gcr(4): iterations, time (cap 100) |")
    print("|---|---|---|---|---|---|")
    for eps in (0.5, 0.1, 0.01):
        for label, sm, mu in (("Jacobi V(2,2)", pkg.SMOOTHER_JACOBI, 2), ("LINE_ALT V(1,1)", pkg.SMOOTHER_LINE_ALT, 1)):
            for pname, transfer in (("bilinear", pkg.TRANSFER_BILINEAR), ("operator-dependent", pkg.TRANSFER_OPERATOR)):
                with pkg.Multigrid(finest_level=LS, coarsest_level=5, mu1=mu, mu2=mu, schedule=0, op=pkg.OP_GALERKIN, smoother=sm) as mg:
                    mg.set_tensor(*tensor(LS, THETA, eps))
                    mg.build_galerkin(transfer)
                    mg.set_rhs(b)
                    cells = [cell(mg, n, f) for f in (lambda: mg.solve(tol=1e-8, max_cycles=100), lambda: mg.solve_gcr(tol=1e-8, max_iters=100, restart=4))]
                print(f"| rotated anisotropy | {eps:g} | {label} | {pname} | " + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    if ONLY in ("", "kernels"):
        kernels()
    if ONLY in ("", "direction"):
        direction()
    if ONLY in ("", "solves"):
        solves()
