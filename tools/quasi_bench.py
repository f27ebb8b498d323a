#!/usr/bin/env python3
"""mgx_quasi (Picard and Newton multigrid for -div(a k(u) grad u) = f): the fused pass next to
k_residual_var, and whole solves next to the host composition.  Writes profiles/quasi_pass_summary.md (--out PATH:
elsewhere); what follows the line `<!-- notes -->` in an existing file is kept.

    python tools/quasi_bench.py [--quick] [--only kernels|solve] [--levels 11,12] [--out PATH]

The tool itself never opens the GPU: every step is a child process of this file (--step NAME) under its own time limit, one
after the other, and the first step that fails or runs out of time ends the run with its exit status.

Kernels (one step per dtype): at a 4096^2 finest level (--quick: 1024^2), a GALERKIN handle after a one-step mgx_quasi call
(contrast 10, k = (1, 0, 1)) that allocates the workspace and leaves a five-point operator: mgx_time_quasi_pass - HIP events
around 20 launches, median of 5 - for the four instances k_quasi_pass<T, STEP, NEWTON>; a launch is the pass and the
k_reduce_partials that follows it.  Words of T per point: u, f and the nodal a in (a is double: two words in float), five
coefficients and b out; STEP adds de in and the trial out.  The yardstick in the same run: k_residual_var<T, 5, 0, 1> through
mgx_residual (7 words in, 1 out; a host clock around 20 calls, one host synchronisation per pass, as tools/newton_bench.py
times it - the synchronisation is in its time).  Bytes are the algorithm's; no counter run is made.  Target, reported and
not gated: 0.8 of k_residual_var's bytes/s.

Solve (one step per size, 2047^2 and 4095^2; --quick: 511^2): GALERKIN, levels L..5, fp64, Jacobi V(2,2), contrast 10, k = (1, 0, 1),
f = 100 h^2, a zero guess, tol = 1e-8, the operator-dependent P, mgx_solve to 1e-6 in 30 cycles at the most per step, eight
halvings at the most, 30 iterations at the most; Newton and Picard.  mgx_quasi (a host clock around the one call, from
mgx_set_rhs / mgx_set_guess on) next to the host composition on the same handle from the same guess: the pass in numpy
(tests/quasi_ref.py), mgx_set_stencil, mgx_build_galerkin_transfer, mgx_set_rhs, a zero guess, mgx_solve, mgx_get_solution,
the trial in numpy and its norm through mgx_residual_norm - copies and numpy's passes included.  The iterates are the same
bits, so the iteration counts are; the difference is the host round trip and numpy's pass."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
STEP = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else ""
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "quasi_pass_summary.md")
LK = 10 if QUICK else 12
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--levels") + 1].split(",")) if "--levels" in sys.argv else (9,) if QUICK else (11, 12)
STEP_LIMIT = 400                                        # seconds, each child
MARK = "<!-- notes -->"
K = (1.0, 0.0, 1.0)


def kernels(pkg, np, contrast, dname):
    n = (1 << LK) - 1
    h2 = 1.0 / float(1 << LK) ** 2
    dtype, tname, es, awords = (pkg.DTYPE_F64, "double", 8, 1) if dname == "f64" else (pkg.DTYPE_F32, "float", 4, 2)
    dt = np.float64 if dname == "f64" else np.float32
    med = lambda f: (f(), statistics.median(f() for _ in range(5)))[1]
    lib = pkg.lib()
    print(f"\n| {1 << LK}^2 finest level, {tname}, contrast 10 | words per point | ms per launch | TB/s (of 8) | over k_residual_var |")
    print("|---|---|---|---|---|")
    with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, dtype=dtype) as mg:
        mg.fill_guess_random(7)
        mg.set_rhs(np.full((n, n), 100.0 * h2, dtype=dt))
        mg.quasi(contrast(LK, 10.0), K, method="picard", lin_tol=1e-2, lin_max_iters=2, tol=0.0, max_iters=1)     # allocates the workspace

        def residual_ms():
            mg.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                lib.mgx_residual(mg._h, LK)
            return (time.perf_counter() - t0) / 20 * 1e3
        t0 = med(residual_ms)
        rate0 = 8 * es * n * n / (t0 * 1e-3)
        rows = [(f"`k_residual_var<{tname}, 5, 0, 1>` (host clock, one synchronisation per pass)", 8, t0)]
        for method, flag in (("picard", "false"), ("newton", "true")):
            for step in (0, 1):
                rows.append((f"`k_quasi_pass<{tname}, {'true' if step else 'false'}, {flag}>` + `k_reduce_partials` (events)",
                             8 + awords + 2 * step, med(lambda: mg.time_quasi_pass(step, method, 20))))
        for name, words, t in rows:
            rate = words * es * n * n / (t * 1e-3)
            print(f"| {name} | {words} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate0:.2f} |", flush=True)


def solve(pkg, np, contrast, L):
    import quasi_ref as qr
    n = (1 << L) - 1
    h2 = 1.0 / float(1 << L) ** 2
    print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), contrast 10, k = (1, 0, 1), f = 100 h^2, operator-dependent P, tol 1e-8 | steps | "
          "backtracks | cycles per step | ms, mgx_quasi | ms, host composition | ratio |")
    print("|---|---|---|---|---|---|---|")
    a = contrast(L, 10.0)
    f, zero = np.full((n, n), 100.0 * h2), np.zeros((n, n))
    transfer = pkg.TRANSFER_OPERATOR
    opts = dict(lin_tol=1e-6, lin_max_iters=30, tol=1e-8, max_iters=30, max_backtracks=8)
    with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
        def lin(op, b, it):
            mg.set_stencil(L, *op)
            mg.build_galerkin(transfer)
            mg.set_rhs(b)
            mg.set_guess(zero)
            st, _ = mg.solve(tol=opts["lin_tol"], max_cycles=opts["lin_max_iters"])
            return mg.get_solution(), st.cycles

        def norm(b):
            mg.set_rhs(b)
            mg.set_guess(zero)
            return mg.residual_norm()

        for method in ("newton", "picard"):
            for rep in range(2):                              # the second of two: workspaces and graphs exist
                mg.synchronize()
                t0 = time.perf_counter()
                mg.set_rhs(f)
                mg.set_guess(zero)
                ns, hist, stats, lam = mg.quasi(a, K, method=method, solver="solve", transfer=transfer, **opts)
                u_dev = mg.get_solution()
                t_dev = time.perf_counter() - t0
                if rep == 0:
                    continue                                  # (the composition is timed once: it has nothing to warm up but the first pass's pages)
                t0 = time.perf_counter()
                o = qr.quasi(a, K, f, zero, lin, opts["tol"], opts["max_iters"], opts["max_backtracks"], method=qr.NEWTON if method == "newton" else qr.PICARD,
                             norm=norm)
                t_host = time.perf_counter() - t0
            same = "" if np.array_equal(o["u"], u_dev) and np.array_equal(o["hist"], hist) else " (the iterates DIFFER)"
            print(f"| {method} | {ns.iterations}{'' if ns.converged else ' (not converged)'} | {ns.backtracks} | {[s.cycles for s in stats]} | "
                  f"{t_dev * 1e3:.1f} | {t_host * 1e3:.1f}{same} | {t_host / t_dev:.2f} |", flush=True)


def run_step(name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    from pcg_ref import contrast_coefficient
    pkg = ge.load_package()
    kind, arg = name.split(":")
    if kind == "kernels":
        kernels(pkg, np, contrast_coefficient, arg)
    else:
        solve(pkg, np, contrast_coefficient, int(arg))


HEAD = """# mgx_quasi: the fused pass and the time of a Newton and a Picard solve

Written by `tools/quasi_bench.py` on one MI355X (HIP events and host clocks as the rows say; no profiler run, no counters).
Bytes per point are the algorithm's; 8 TB/s is the HBM figure the other summaries use.  Target, reported and not gated:
0.8 of `k_residual_var`'s rate for the eight instances of `k_quasi_pass`.
"""


if __name__ == "__main__":
    if STEP:
        run_step(STEP)
        sys.exit(0)
    todo = ([f"kernels:{d}" for d in ("f64", "f32")] if ONLY in ("", "kernels") else []) + ([f"solve:{L}" for L in SIZES] if ONLY in ("", "solve") else [])
    notes = ""
    if os.path.exists(OUT) and MARK in open(OUT).read():
        notes = open(OUT).read().split(MARK, 1)[1]
    text, rc = HEAD, 0
    for step in todo:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", step] + (["--quick"] if QUICK else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        text += r.stdout
        rc = r.returncode
        if rc != 0:
            text += f"\nstep {step} ended with status {rc}: not measured from here on\n"
            print(f"step {step} ended with status {rc}: stopping", flush=True)
            break
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n" + MARK + notes)
    sys.exit(rc)
