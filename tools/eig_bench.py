#!/usr/bin/env python3
"""mgx_eigs (LOBPCG around the block cycle): its four passes next to k_pcg_update, one iteration next to one
block cycle of mgx_solve_multi, and the time to four eigenpairs (the tables of profiles/eig_kernel_trace_summary.md).

    python tools/eig_bench.py [--quick] [--only kernels|iteration|solves] [--levels 11,12]

The tool itself never opens the GPU: every step is a child process of this file (--step NAME) under its own time limit, one
after the other, and the first step that fails or runs out of time ends the run with its exit status.

Kernels (one step per dtype): at a 4096^2 finest level (--quick: 1024^2), GALERKIN handles with a five-point (contrast 10)
and a nine-point (rotated anisotropy) finest operator: mgx_time_eig_pass - HIP events around 20 launches, median of 5 - for
nev = 1, 2, 4, next to mgx_time_gcr_pass(UPDATE) = k_pcg_update (6 sizeof(T) per point) in the same run.  Bytes are the
algorithm's (mgx.h, mgx_time_eig_pass); no counter run is made.  Target, reported and not gated: 0.8 of k_pcg_update's
bytes/s.

Iteration (one step per size, 2047^2 and 4095^2; --quick: 511^2): GALERKIN, levels L..5, fp64, Jacobi V(2,2), contrast 10
with the operator-dependent P, four columns.  tol = 0 keeps every column active; stats.seconds of eigs(max_iters = 8) minus
that of eigs(max_iters = 3), over 5, is one iteration (the copies of the vectors in and out cancel); the same difference of
solve_multi(max_cycles = 8) and (3) is one block cycle with its norm.  Median of 3.

Solves (one step per size): iterations and time (stats.seconds: the whole call, the host copies of the four vectors in
and out included) to tol = 1e-8 for four modes from the binding's seeded guesses, cap 100: the Poisson operator (bilinear
P), contrast 10 (operator-dependent P), rotated anisotropy 45 degrees eps = 0.5 (bilinear P).  Second call of two."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
STEP = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else ""
LK = 10 if QUICK else 12
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--levels") + 1].split(",")) if "--levels" in sys.argv else (9,) if QUICK else (11, 12)
STEP_LIMIT = 400                                        # seconds, each child


def problems(pkg, np, L, poisson=False):
    import nine_ref
    from pcg_ref import contrast_coefficient
    n = (1 << L) - 1
    if poisson:
        full = lambda v: np.full((n, n), v)
        yield "Poisson", "BILINEAR", (lambda mg: mg.set_stencil(L, full(4.0), full(-1.0), full(-1.0), full(-1.0), full(-1.0))), pkg.TRANSFER_BILINEAR, 5
    yield "contrast 10", "OPERATOR", (lambda mg: mg.set_coefficient(contrast_coefficient(L, 10.0))), pkg.TRANSFER_OPERATOR, 5
    yield ("rotated anisotropy 45 degrees, eps = 0.5", "BILINEAR", (lambda mg: mg.set_tensor(*nine_ref.rotated_tensor(L, 45.0, 0.5))),
           pkg.TRANSFER_BILINEAR, 9)


def new_handle(pkg, L, setter, transfer, dtype=None):
    kw = {} if dtype is None else dict(dtype=dtype)
    mg = pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, **kw)
    setter(mg)
    mg.build_galerkin(transfer)
    return mg


def kernels(pkg, np, dname):
    n = (1 << LK) - 1
    dtype, tname, es = (pkg.DTYPE_F64, "double", 8) if dname == "f64" else (pkg.DTYPE_F32, "float", 4)
    med = lambda f: (f(), statistics.median(f() for _ in range(5)))[1]
    print(f"\n| {1 << LK}^2 finest level, {tname} | nev | words per point | ms per launch | TB/s (of 8) | over k_pcg_update |")
    print("|---|---|---|---|---|---|")
    for what, _, setter, transfer, nq in problems(pkg, np, LK):
        with new_handle(pkg, LK, setter, transfer, dtype) as mg:
            mg.fill_rhs()
            mg.solve_gcr(tol=0.0, max_iters=1, restart=1)                    # allocates the Krylov workspace of the yardstick
            mg.eigs(4, tol=0.0, max_iters=1)                                 # allocates four columns, every kernel has run once
            t0 = med(lambda: mg.time_gcr_pass(0, 0, 20))
            rate0 = 6 * es * n * n / (t0 * 1e-3)
            print(f"| `k_pcg_update<{tname}>` ({what}) | | 6 | {t0:.4f} | {rate0 / 1e12:.2f} ({rate0 / 8e12:.2f}) | 1.00 |", flush=True)
            for which, name, words in ((pkg.EIG_PASS_GRAM, "k_eig_gram<{t}, {k}, {k}, false>", lambda k: 3 * k),
                                       (pkg.EIG_PASS_COMBINE, "k_eig_combine<{t}, {k3}, {k}>", lambda k: 4 * k),
                                       (pkg.EIG_PASS_RESIDUAL, "k_eig_residual<{t}, {k}>", lambda k: 3 * k),
                                       (pkg.EIG_PASS_APPLY, "k_apply_var_multi<{t}, {q}, {k}>", lambda k: nq + 2 * k)):
                for nev in (1, 2, 4):
                    t = med(lambda: mg.time_eig_pass(which, nev, 20))
                    rate = words(nev) * es * n * n / (t * 1e-3)
                    print(f"| `{name.format(t=tname, k=nev, k3=3 * nev, q=nq)}` | {nev} | {words(nev)} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | "
                          f"{rate / rate0:.2f} |", flush=True)


def iteration(pkg, np, L):
    n = (1 << L) - 1
    what, tname, setter, transfer, _ = next(problems(pkg, np, L))
    b = np.stack([np.random.default_rng(3 + j).uniform(-1, 1, (n, n)) for j in range(4)])
    with new_handle(pkg, L, setter, transfer) as mg:
        g = np.random.default_rng(0).uniform(-1.0, 1.0, (4, n, n))
        eig_ms = lambda k: mg.eigs(4, x0=g, tol=0.0, max_iters=k)[2][0].seconds * 1e3        # stats.seconds: the C call alone
        cyc_ms = lambda k: mg.solve_multi(b, tol=0.0, max_cycles=k)[0][0].seconds * 1e3
        eig_ms(1)
        cyc_ms(1)
        it, cy = [], []
        for _ in range(3):
            it.append((eig_ms(8) - eig_ms(3)) / 5)
            cy.append((cyc_ms(8) - cyc_ms(3)) / 5)
        mi, mc = statistics.median(it), statistics.median(cy)
        print(f"\n| {n}^2, levels {L}..5, fp64, {what}, P {tname}, four columns | ms |\n|---|---|")
        print(f"| one mgx_eigs iteration (cycle, A W, six Gram pairs, two combines, A X, A P, residuals; two host synchronisations) | {mi:.3f} "
              f"(min {min(it):.3f}, max {max(it):.3f}) |")
        print(f"| one mgx_solve_multi cycle with its residual norms | {mc:.3f} (min {min(cy):.3f}, max {max(cy):.3f}) |")
        print(f"| iteration / cycle | {mi / mc:.2f} |", flush=True)


def solves(pkg, np, L):
    n = (1 << L) - 1
    print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), nev = 4, tol 1e-8, cap 100 | P | iterations | cycles per column | converged | "
          "seconds (whole call) | lambda_0 .. lambda_3 |")
    print("|---|---|---|---|---|---|---|")
    for what, tname, setter, transfer, _ in problems(pkg, np, L, poisson=True):
        with new_handle(pkg, L, setter, transfer) as mg:
            for _ in range(2):
                theta, X, stats, hists = mg.eigs(4, tol=1e-8, max_iters=100)
            print(f"| {what} | {tname} | {len(hists[0]) - 1} | {[st.cycles for st in stats]} | {[st.converged for st in stats]} | {stats[0].seconds:.3f} | "
                  f"{' '.join(f'{t:.6e}' for t in theta)} |", flush=True)
            print(f"|   last residuals / (tol theta): {' '.join(f'{h[-1] / (1e-8 * t):.2g}' for h, t in zip(hists, theta))} | | | | | | |", flush=True)


def run_step(name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    kind, arg = name.split(":")
    if kind == "kernels":
        kernels(pkg, np, arg)
    elif kind == "iteration":
        iteration(pkg, np, int(arg))
    else:
        solves(pkg, np, int(arg))


if __name__ == "__main__":
    if STEP:
        run_step(STEP)
        sys.exit(0)
    steps = ([f"kernels:{d}" for d in ("f64", "f32")] if ONLY in ("", "kernels") else []) + \
            ([f"iteration:{L}" for L in SIZES] if ONLY in ("", "iteration") else []) + \
            ([f"solves:{L}" for L in SIZES] if ONLY in ("", "solves") else [])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", step] + (["--quick"] if QUICK else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
