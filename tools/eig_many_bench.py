#!/usr/bin/env python3
"""mgx_eigs_many (deflated LOBPCG around the block cycle): the two passes of its projection next to
k_pcg_update, and the time to 8 and 16 eigenpairs next to mgx_eigs with four.  Writes profiles/eig_many_kernel_trace_summary.md
(--out PATH: elsewhere); what follows the line `<!-- notes -->` in an existing file is kept.

    python tools/eig_many_bench.py [--quick] [--only kernels|solves] [--levels 11,12] [--out PATH]

The tool itself never opens the GPU: every step is a child process of this file (--step NAME) under its own time limit, one
after the other, and the first step that fails or runs out of time ends the run with its exit status.

Kernels (one step per dtype): at a 4096^2 finest level (--quick: 1024^2), a GALERKIN handle with the contrast-10 operator:
mgx_time_eig_project - HIP events around 20 launches, median of 5 - for m = 4, 8, 12 locked vectors and k = 1 .. 4 columns,
next to mgx_time_gcr_pass(UPDATE) = k_pcg_update (6 sizeof(T) per point) in the same run.  Bytes are the algorithm's: DOTS
m + k ceil(m / 8) words per point (every locked vector once, the columns once per chunk of eight; the reductions included in the
time), SUB m + 2 k.  No counter run is made.  Target, reported and not gated: 0.8 of k_pcg_update's bytes/s.

Solves (one step per size, 2047^2 and 4095^2; --quick: 511^2): GALERKIN, levels L..5, fp64, Jacobi V(2,2); the Poisson operator
(bilinear P), contrast 10 (operator-dependent P), rotated anisotropy 45 degrees eps = 0.5 (bilinear P).  tol = 1e-8, 200
iterations per block at the most, the binding's seeded guesses; eigs(4), eigs_many(8), eigs_many(16) on the same handle, the
second call of two each.  Seconds are stats.seconds (the whole C call, the host copies of the vectors in and out included),
also per pair; |X^T X - I| over all returned vectors in float64 on the host."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
STEP = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else ""
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "eig_many_kernel_trace_summary.md")
LK = 10 if QUICK else 12
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--levels") + 1].split(",")) if "--levels" in sys.argv else (9,) if QUICK else (11, 12)
STEP_LIMIT = 400                                        # seconds, each child
MARK = "<!-- notes -->"


def kernels(pkg, np, eb, dname):
    n = (1 << LK) - 1
    dtype, tname, es = (pkg.DTYPE_F64, "double", 8) if dname == "f64" else (pkg.DTYPE_F32, "float", 4)
    med = lambda f: (f(), statistics.median(f() for _ in range(5)))[1]
    what, _, setter, transfer, _ = next(eb.problems(pkg, np, LK))
    print(f"\n| {1 << LK}^2 finest level, {tname}, {what} | m | k | words per point | ms per launch | TB/s (of 8) | over k_pcg_update |")
    print("|---|---|---|---|---|---|---|")
    with eb.new_handle(pkg, LK, setter, transfer, dtype) as mg:
        mg.fill_rhs()
        mg.solve_gcr(tol=0.0, max_iters=1, restart=1)                        # allocates the Krylov workspace of the yardstick
        mg.eigs_many(pkg.EIGS_MAX, tol=0.0, max_iters=1)                     # allocates sixteen slots and four columns; ends after block 0
        t0 = med(lambda: mg.time_gcr_pass(0, 0, 20))
        rate0 = 6 * es * n * n / (t0 * 1e-3)
        print(f"| `k_pcg_update<{tname}>` | | | 6 | {t0:.4f} | {rate0 / 1e12:.2f} ({rate0 / 8e12:.2f}) | 1.00 |", flush=True)
        for which, name, words in ((pkg.EIG_PROJECT_DOTS, "k_eig_project_dots<{t}, {c}, {k}>", lambda m, k: m + k * ((m + 7) // 8)),
                                   (pkg.EIG_PROJECT_SUB, "k_eig_project_sub<{t}, {k}>", lambda m, k: m + 2 * k)):
            for m in (4, 8, 12):
                for k in (1, 2, 3, 4):
                    t = med(lambda: mg.time_eig_project(which, m, k, 20))
                    rate = words(m, k) * es * n * n / (t * 1e-3)
                    chunks = "8 + 4" if m == 12 else str(m)
                    print(f"| `{name.format(t=tname, c=chunks, k=k)}` | {m} | {k} | {words(m, k)} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | "
                          f"{rate / rate0:.2f} |", flush=True)


def solves(pkg, np, eb, L):
    n = (1 << L) - 1
    print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), tol 1e-8, 200 iterations per block | P | call | iteration counts of the blocks (distinct) | converged | "
          "seconds (whole call) | seconds per pair | over eigs(4) per pair | X^T X - I |")
    print("|---|---|---|---|---|---|---|---|---|")
    for what, tname, setter, transfer, _ in eb.problems(pkg, np, L, poisson=True):
        with eb.new_handle(pkg, L, setter, transfer) as mg:
            base = None
            for nev in (4, 8, 16):
                call = mg.eigs if nev == 4 else mg.eigs_many
                for _ in range(2):
                    theta, X, stats, hists = call(nev, tol=1e-8, max_iters=200)
                V = X.reshape(nev, -1).astype(np.float64)
                defect = float(np.max(np.abs(V @ V.T - np.eye(nev))))
                # the pairs are sorted across the blocks: a block's iteration count is the history length its pairs share
                its = sorted({len(h) - 1 for h in hists})
                per = stats[0].seconds / nev
                base = per if base is None else base
                print(f"| {what} | {tname} | `{'mgx_eigs' if nev == 4 else 'mgx_eigs_many'}`, nev {nev} | {its} | {sum(st.converged for st in stats)} of {nev} | "
                      f"{stats[0].seconds:.3f} | {per:.3f} | {per / base:.2f} | {defect:.2e} |", flush=True)
                del X, V


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
        solves(pkg, np, eb, int(arg))


HEAD = """# mgx_eigs_many: the projection passes and the time to 8 and 16 eigenpairs

Written by `tools/eig_many_bench.py` on one MI355X (HIP events; no profiler run, no counters).  Bytes per point are the
algorithm's; 8 TB/s is the HBM figure the other summaries use.  Target, reported and not gated: 0.8 of `k_pcg_update`'s rate.
"""


if __name__ == "__main__":
    if STEP:
        run_step(STEP)
        sys.exit(0)
    steps = ([f"kernels:{d}" for d in ("f64", "f32")] if ONLY in ("", "kernels") else []) + ([f"solves:{L}" for L in SIZES] if ONLY in ("", "solves") else [])
    notes = ""
    if os.path.exists(OUT) and MARK in open(OUT).read():
        notes = open(OUT).read().split(MARK, 1)[1]
    text, rc = HEAD, 0
    for step in steps:
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
