#!/usr/bin/env python3
"""mgx_newton_steps (implicit time stepping of rho u_t = div(a grad u) - kappa phi(u) + f): its passes next
to k_residual_var, and a time step next to the host composition.  Writes profiles/newton_steps_summary.md (--out PATH:
elsewhere); what follows the line `<!-- notes -->` in an existing file is kept.

    python tools/newton_steps_bench.py [--quick] [--only kernels|steps] [--levels 11,12] [--out PATH]

The tool itself never opens the GPU: every step is a child process of this file (--step NAME) under its own time limit, one
after the other, and the first step that fails or runs out of time ends the run with its exit status.

Kernels (one step per dtype): at a 4096^2 finest level (--quick: 1024^2), GALERKIN handles with the contrast-10 operator
(five-point) and the rotated anisotropy (nine-point), after a one-step mgx_newton_steps call (Allen-Cahn, a source) that
allocates the workspace: mgx_time_newton_step_pass - HIP events around 20 launches, median of 5 - for pass 0 with theta = 1/2
(k_newton_step_rhs<T, NQ, false>, NQ + 4 words in, 1 out) and theta = 1 (k_newton_step_rhs<T, 5, true>, 3 in, 1 out), pass 1
(k_newton_pass<T, NQ, false, true>, NQ + 4 in, 2 out) and pass 2 (k_newton_pass<T, NQ, true, true>, NQ + 5 in, 3 out); a
launch of pass 1 or 2 is the pass and the k_reduce_partials that follows it.  The yardstick in the same run:
k_residual_var<T, NQ, 0, 1> through mgx_residual (NQ + 2 words in, 1 out; a host clock around 20 calls, one host
synchronisation per pass, as tools/newton_bench.py times it - the synchronisation is in its time).  Bytes are the
algorithm's; no counter run is made.  Target: 0.8 of k_residual_var's bytes/s, stated as hit or missed per instance.

Steps (one step per size, 2047^2 and 4095^2; --quick: 511^2): GALERKIN, levels L..5, fp64, Jacobi V(2,2), contrast 10
(operator-dependent P), Allen-Cahn phi = u^3 - u with kappa = 100 h^2, rho = 1, dt = 1e-4 (mass = h^2 / (theta dt)), no
source, a seeded random start of amplitude 1, Newton to tol = 1e-8 in ten iterations at the most, mgx_solve to 1e-6 in 30
cycles at the most per iteration, eight halvings at the most; two steps per call, Crank-Nicolson and Euler.
mgx_newton_steps (a host clock around the one call, from mgx_set_guess to mgx_get_solution) next to the host composition on
the same handle from the same start: the two passes in numpy (tests/newton_steps_ref.py), mgx_set_reaction,
mgx_build_galerkin_transfer, mgx_set_rhs, a zero guess, mgx_solve, mgx_get_solution, the trial in numpy and its norm
through mgx_residual_norm - copies included.  Before this entry point that composition was the only way to take such a
step, so it is also the parent's time.  The time levels are the same bits, so the iteration counts are."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
STEP = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else ""
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "newton_steps_summary.md")
LK = 10 if QUICK else 12
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--levels") + 1].split(",")) if "--levels" in sys.argv else (9,) if QUICK else (11, 12)
STEP_LIMIT = 400                                        # seconds, each child
NSTEPS = 2
MARK = "<!-- notes -->"
ALLEN_CAHN = (-1.0, 0.0, 1.0)


def kernels(pkg, np, eb, dname):
    n = (1 << LK) - 1
    h2 = 1.0 / float(1 << LK) ** 2
    dtype, tname, es = (pkg.DTYPE_F64, "double", 8) if dname == "f64" else (pkg.DTYPE_F32, "float", 4)
    dt = np.float64 if dname == "f64" else np.float32
    med = lambda f: (f(), statistics.median(f() for _ in range(5)))[1]
    lib = pkg.lib()
    print(f"\n| {1 << LK}^2 finest level, {tname} | operator | words per point | ms per launch | TB/s (of 8) | over k_residual_var | 0.8x target |")
    print("|---|---|---|---|---|---|---|")
    for what, _, setter, transfer, nq in eb.problems(pkg, np, LK):
        with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, dtype=dtype) as mg:
            setter(mg)
            mg.build_galerkin(transfer)
            mg.fill_guess_random(7)
            full = lambda v: np.full((n, n), v, dtype=dt)
            mg.newton_steps(1, full(1.0), full(100.0 * h2), p=ALLEN_CAHN, theta=0.5, g=full(h2), lin_tol=1e-2, lin_max_iters=2, tol=0.0,
                            max_newton=1)                     # allocates the workspace

            def residual_ms():
                mg.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    lib.mgx_residual(mg._h, LK)
                return (time.perf_counter() - t0) / 20 * 1e3
            t0 = med(residual_ms)
            rate0 = (nq + 3) * es * n * n / (t0 * 1e-3)
            rows = [(f"`k_residual_var<{tname}, {nq}, 0, 1>` (host clock, one synchronisation per pass)", nq + 3, t0),
                    (f"`k_newton_step_rhs<{tname}, {nq}, false>` (events)", nq + 5, med(lambda: mg.time_newton_step_pass(0, 0.5, 20))),
                    (f"`k_newton_step_rhs<{tname}, 5, true>` (events)", 4, med(lambda: mg.time_newton_step_pass(0, 1.0, 20))),
                    (f"`k_newton_pass<{tname}, {nq}, false, true>` + `k_reduce_partials` (events)", nq + 6, med(lambda: mg.time_newton_step_pass(1, 0.5, 20))),
                    (f"`k_newton_pass<{tname}, {nq}, true, true>` + `k_reduce_partials` (events)", nq + 8, med(lambda: mg.time_newton_step_pass(2, 0.5, 20)))]
            for i, (name, words, t) in enumerate(rows):
                rate = words * es * n * n / (t * 1e-3)
                verdict = "" if i == 0 else "hit" if rate >= 0.8 * rate0 else "missed"
                print(f"| {name} | {what} | {words} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate0:.2f} | {verdict} |", flush=True)


def steps(pkg, np, eb, L):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import galerkin_ref as gr
    import newton_steps_ref as nsr
    n = (1 << L) - 1
    h2 = 1.0 / float(1 << L) ** 2
    print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), contrast 10, Allen-Cahn, kappa = 100 h^2, dt = 1e-4, {NSTEPS} steps | Newton iterations per step | "
          "cycles per step | ms per step, mgx_newton_steps | ms per step, host composition (= the parent's only way) | ratio |")
    print("|---|---|---|---|---|---|")
    what, _, setter, transfer, _ = next(eb.problems(pkg, np, L))
    u0 = np.random.default_rng(5).uniform(-1.0, 1.0, (n, n))
    kap = np.full((n, n), 100.0 * h2)
    zero = np.zeros((n, n))
    opts = dict(lin_tol=1e-6, lin_max_iters=30, tol=1e-8, max_newton=10, max_backtracks=8)
    with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
        setter(mg)
        mg.build_galerkin(transfer)
        A0 = gr.nine([mg.get_stencil(L, q) for q in range(5)])

        def lin(S9, b, d, k):
            mg.set_reaction(d)
            mg.build_galerkin(transfer)
            mg.set_rhs(b)
            mg.set_guess(zero)
            st, _ = mg.solve(tol=opts["lin_tol"], max_cycles=opts["lin_max_iters"])
            return mg.get_solution(), (st.cycles,)

        def norm(b):
            mg.set_rhs(b)
            mg.set_guess(zero)
            return mg.residual_norm()

        for name, theta in (("Crank-Nicolson", 0.5), ("implicit Euler", 1.0)):
            dm = np.full((n, n), h2 / (theta * 1e-4))
            for rep in range(2):                              # the second of two device runs: workspaces and graphs exist
                mg.synchronize()
                t0 = time.perf_counter()
                mg.set_guess(u0)
                done, stats, hists = mg.newton_steps(NSTEPS, dm, kap, p=ALLEN_CAHN, theta=theta, solver="solve", **opts)
                u_dev = mg.get_solution()
                t_dev = time.perf_counter() - t0
            t0 = time.perf_counter()
            o = nsr.steps(A0, kap, dm, None, ALLEN_CAHN, u0, theta, NSTEPS, lin, opts["tol"], opts["max_newton"], opts["max_backtracks"], norm=norm)
            t_host = time.perf_counter() - t0
            same = "" if done == len(o) and np.array_equal(o[-1]["u"], u_dev) and all(np.array_equal(a["hist"], h) for a, h in zip(o, hists)) \
                else " (the time levels DIFFER)"
            note = "" if done == NSTEPS and all(s.converged for s in stats) else f" ({done} steps, the last not converged)"
            print(f"| {name}, {what} | {[s.iterations for s in stats]}{note} | {[s.linear_iterations for s in stats]} | {t_dev * 1e3 / max(done, 1):.1f} | "
                  f"{t_host * 1e3 / max(len(o), 1):.1f}{same} | {t_host / t_dev:.2f} |", flush=True)


def run_step(name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import __graft_entry__ as ge
    import eig_bench as eb
    pkg = ge.load_package()
    kind, arg = name.split(":")
    if kind == "kernels":
        kernels(pkg, np, eb, arg)
    else:
        steps(pkg, np, eb, int(arg))


HEAD = """# mgx_newton_steps: the passes and the time of a time step

Written by `tools/newton_steps_bench.py` on one MI355X (HIP events and host clocks as the rows say; no profiler run, no
counters).  Bytes per point are the algorithm's; 8 TB/s is the HBM figure the other summaries use.  Target: 0.8 of
`k_residual_var`'s rate for every instance, stated per row.
"""


if __name__ == "__main__":
    if STEP:
        run_step(STEP)
        sys.exit(0)
    todo = ([f"kernels:{d}" for d in ("f64", "f32")] if ONLY in ("", "kernels") else []) + ([f"steps:{L}" for L in SIZES] if ONLY in ("", "steps") else [])
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
