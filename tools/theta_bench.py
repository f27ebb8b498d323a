#!/usr/bin/env python3
"""mgx_theta_steps (implicit time stepping on S = A0 + diag(d)): the right-hand-side pass next to
k_residual_var, and the time per step next to the host composition.  Writes profiles/theta_kernel_trace_summary.md
(--out PATH: elsewhere); what follows the line `<!-- notes -->` in an existing file is kept.

    python tools/theta_bench.py [--quick] [--only kernels|steps] [--levels 11,12] [--out PATH]

The tool itself never opens the GPU: every step is a child process of this file (--step NAME) under its own time limit, one
after the other, and the first step that fails or runs out of time ends the run with its exit status.

Kernels (one step per dtype): at a 4096^2 finest level (--quick: 1024^2), GALERKIN handles with the contrast-10 operator
(five-point) and the rotated anisotropy (nine-point), d = 1: mgx_time_theta_rhs - HIP events around 20 launches, median of 5
- for theta = 0.5 (k_theta_rhs<T, NQ, false>, NQ + 3 words in, 1 out) and theta = 1 (k_theta_rhs<T, 5, true>, 3 in, 1 out).
Two yardsticks in the same run: k_residual_var<T, NQ, 0, 1> through mgx_residual (NQ + 2 words in, 1 out: the pass reads d
on top of that; a host clock around 20 calls, one host synchronisation per pass, as tools/galerkin_bench.py times it - the
synchronisation is in its time), and
k_apply_var_multi<T, NQ, 1> through mgx_time_eig_pass (NQ + 2 words, HIP events like the pass).  Bytes are the algorithm's;
no counter run is made.  Target, reported and not gated: 0.8 of k_residual_var's bytes/s.

Steps (one step per size, 2047^2 and 4095^2; --quick: 511^2): GALERKIN, levels L..5, fp64, Jacobi V(2,2), contrast 10
(operator-dependent P), d = h^2 / (theta dt) with dt = 1e-3, g = h^2, a seeded random start, tol = 1e-8, 30 iterations per
step at the most, five steps.  mgx_theta_steps (a host clock around the one call) next to the host composition on the same
handle, from the same start: S u = -mgx_residual(u, 0) for theta < 1 (U and a zero B up, R down), or mgx_get_solution
for theta = 1; the pass in numpy; mgx_set_rhs; the same solver - copies included.  The iterates are the same bits, so
the iteration counts are; the difference is the host round trip."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
STEP = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else ""
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "theta_kernel_trace_summary.md")
LK = 10 if QUICK else 12
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--levels") + 1].split(",")) if "--levels" in sys.argv else (9,) if QUICK else (11, 12)
STEP_LIMIT = 400                                        # seconds, each child
MARK = "<!-- notes -->"
NSTEPS = 5


def kernels(pkg, np, eb, dname):
    n = (1 << LK) - 1
    dtype, tname, es = (pkg.DTYPE_F64, "double", 8) if dname == "f64" else (pkg.DTYPE_F32, "float", 4)
    dt = np.float64 if dname == "f64" else np.float32
    med = lambda f: (f(), statistics.median(f() for _ in range(5)))[1]
    lib = pkg.lib()
    print(f"\n| {1 << LK}^2 finest level, {tname} | operator | words per point | ms per launch | TB/s (of 8) | over k_residual_var |")
    print("|---|---|---|---|---|---|")
    for what, _, setter, transfer, nq in eb.problems(pkg, np, LK):
        with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, dtype=dtype) as mg:
            setter(mg)
            mg.set_reaction(np.ones((n, n), dtype=dt))
            mg.build_galerkin(transfer)
            mg.fill_guess_random(7)
            mg.fill_rhs()
            mg.eigs(1, tol=0.0, max_iters=1)                                 # allocates the column of the second yardstick

            def residual_ms():
                mg.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    lib.mgx_residual(mg._h, LK)
                return (time.perf_counter() - t0) / 20 * 1e3
            t0 = med(residual_ms)
            rate0 = (nq + 3) * es * n * n / (t0 * 1e-3)
            rows = [(f"`k_residual_var<{tname}, {nq}, 0, 1>` (host clock, one synchronisation per pass)", nq + 3, t0),
                    (f"`k_apply_var_multi<{tname}, {nq}, 1>` (events)", nq + 2, med(lambda: mg.time_eig_pass(pkg.EIG_PASS_APPLY, 1, 20))),
                    (f"`k_theta_rhs<{tname}, {nq}, false>`, theta = 0.5 (events)", nq + 4, med(lambda: mg.time_theta_rhs(0.5, 20))),
                    (f"`k_theta_rhs<{tname}, 5, true>`, theta = 1 (events)", 4, med(lambda: mg.time_theta_rhs(1.0, 20)))]
            for name, words, t in rows:
                rate = words * es * n * n / (t * 1e-3)
                print(f"| {name} | {what} | {words} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate0:.2f} |", flush=True)


def steps(pkg, np, eb, L):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import theta_ref as tr
    n = (1 << L) - 1
    h2 = 1.0 / float(1 << L) ** 2
    print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), contrast 10, dt 1e-3, tol 1e-8, {NSTEPS} steps | theta | solver | iterations per step | "
          "ms per step, mgx_theta_steps | ms per step, host composition | ratio |")
    print("|---|---|---|---|---|---|---|")
    what, _, setter, transfer, _ = next(eb.problems(pkg, np, L))
    u0 = np.random.default_rng(5).uniform(-1.0, 1.0, (n, n))
    g = np.full((n, n), h2)
    zero = np.zeros((n, n))
    for theta in (0.5, 1.0):
        d = np.full((n, n), h2 / (theta * 1e-3))
        with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            setter(mg)
            mg.set_reaction(d)
            mg.build_galerkin(transfer)
            for solver, run in (("solve", lambda: mg.solve(tol=1e-8, max_cycles=30)), ("refine_gcr", lambda: mg.solve_refine_gcr(tol=1e-8, max_iters=30, restart=4))):
                t_dev = t_host = 0.0
                for rep in range(2):                           # the second of two: workspaces, graphs and the float copy exist
                    mg.set_guess(u0)
                    mg.synchronize()
                    t0 = time.perf_counter()
                    done, stats, hists = mg.theta_steps(NSTEPS, theta=theta, g=g, solver=solver, tol=1e-8, max_iters=30, restart=4)
                    t_dev = (time.perf_counter() - t0) / max(done, 1)
                    u_dev = mg.get_solution()
                    mg.set_guess(u0)
                    mg.synchronize()
                    t0 = time.perf_counter()
                    u = u0
                    for _ in range(done):
                        Su = None if theta == 1.0 else -mg.residual(L, u, zero)
                        mg.set_rhs(tr.rhs_pass(Su, u, d, g, theta))
                        run()
                        u = mg.get_solution()
                    t_host = (time.perf_counter() - t0) / max(done, 1)
                same = "" if np.array_equal(u, u_dev) else " (the iterates DIFFER)"
                its = [st.cycles for st in stats]
                print(f"| {what} | {theta} | `{solver}` | {its}{'' if done == NSTEPS else ' (ended early)'} | {t_dev * 1e3:.2f} | {t_host * 1e3:.2f}{same} | "
                      f"{t_host / t_dev:.2f} |", flush=True)


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


HEAD = """# mgx_theta_steps: the right-hand-side pass and the time per step

Written by `tools/theta_bench.py` on one MI355X (HIP events and host clocks as the rows say; no profiler run, no counters).
Bytes per point are the algorithm's; 8 TB/s is the HBM figure the other summaries use.  Target, reported and not gated:
0.8 of `k_residual_var`'s rate for `k_theta_rhs<T, 5 | 9, false>`.
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
