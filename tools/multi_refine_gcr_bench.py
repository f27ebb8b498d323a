#!/usr/bin/env python3
"""mgx_solve_multi_refine_gcr (fp64 restarted GCR around the float block cycle on up to four right-hand sides)
next to four mgx_solve_refine_gcr rounds and one mgx_solve_multi_gcr call on the same handle, and its K-column direction
pass next to its K = 1 instance (the tables of profiles/multi_refine_gcr_kernel_trace_summary.md).

    python tools/multi_refine_gcr_bench.py [--quick] [--only kernels|solves] [--levels 11,12]

The tool itself never opens the GPU: every step is a child process of this file (--step NAME) under its own time limit, one
after the other, and the first step that fails or runs out of time ends the run with its exit status.

Kernels (one step): at a 4096^2 finest level (--quick: 1024^2), GALERKIN fp64 handles with a five-point (contrast 10) and a
nine-point (rotated anisotropy) finest operator: mgx_time_multi_refine_direction - HIP events around 20 launches, median of
5 - for nrhs = 1 (k_refine_direction<NQ, 1> on a workspace column, the yardstick of the same run) and nrhs = 2, 3, 4
(k_refine_direction<NQ, K>).  Bytes are the algorithm's: 8 NQ + 20 K per point; no counter run is made.
Target: the K-column instances move their bytes at 0.8 of the K = 1 instance's bytes/s.

Solves (one step per size): time to 1e-10 at 2047^2 and 4095^2 (--quick: 511^2; --levels: the finest levels named), GALERKIN,
levels L..5, fp64, Jacobi V(2,2), GCR(4), four columns b_j = default_rng(3 + j).uniform(-1, 1) from zero guesses; contrast 10
with the operator-dependent P and rotated anisotropy (45 degrees, eps = 0.5, 0.1, 0.01) with the bilinear P.  One
solve_multi_refine_gcr call against four set_rhs / set_guess / solve_refine_gcr / get_solution rounds and against one
solve_multi_gcr call on ONE handle, in turn, median of 3 each after a round that captures the graphs and allocates the
workspaces; all on the host clock around everything the caller waits for (the copies of b and u in, the solves, the
copies of u out)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
STEP = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else ""
LK = 10 if QUICK else 12
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--levels") + 1].split(",")) if "--levels" in sys.argv else (9,) if QUICK else (11, 12)
TOL, RESTART = 1e-10, 4
STEP_LIMIT = 400                                        # seconds, each child


def problems(pkg, L, eps_list):
    import nine_ref
    from pcg_ref import contrast_coefficient
    yield "contrast 10", "OPERATOR", (lambda mg: mg.set_coefficient(contrast_coefficient(L, 10.0))), pkg.TRANSFER_OPERATOR, 5
    for eps in eps_list:
        yield (f"rotated anisotropy 45 degrees, eps = {eps:g}", "BILINEAR",
               (lambda mg, eps=eps: mg.set_tensor(*nine_ref.rotated_tensor(L, 45.0, eps))), pkg.TRANSFER_BILINEAR, 9)


def kernels(pkg, np):
    n = (1 << LK) - 1
    print(f"\n| {1 << LK}^2 finest level, fp64 | nrhs | B per point | ms per launch | TB/s (of 8) | over nrhs = 1 | "
          "ms per column, over nrhs = 1 | byte model, over nrhs = 1 |")
    print("|---|---|---|---|---|---|---|---|")
    for what, _, setter, transfer, nq in problems(pkg, LK, (0.5,)):
        with pkg.Multigrid(finest_level=LK, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            setter(mg)
            mg.build_galerkin(transfer)
            b = np.random.default_rng(3).uniform(-1, 1, (4, n, n))
            mg.solve_multi_refine_gcr(b, tol=0.0, max_iters=1, restart=1)   # allocates the columns and slot 0, every kernel has run once
            del b
            rate1 = t1 = None
            for nrhs in (1, 2, 3, 4):
                mg.time_multi_refine_direction(nrhs, 20)
                t = statistics.median(mg.time_multi_refine_direction(nrhs, 20) for _ in range(5))
                nbytes = 8 * nq + 20 * nrhs
                rate = nbytes * n * n / (t * 1e-3)
                if nrhs == 1:
                    rate1, t1 = rate, t
                kernel = f"`k_refine_direction<{nq}, {nrhs}>`"
                print(f"| {kernel} | {nrhs} | {nbytes} | {t:.4f} | {rate / 1e12:.2f} ({rate / 8e12:.2f}) | {rate / rate1:.2f} | "
                      f"{t / nrhs:.4f}, {t / nrhs / t1:.2f} | {nbytes / nrhs / (8 * nq + 20):.2f} |", flush=True)


def solves(pkg, np, L):
    n = (1 << L) - 1
    b = np.stack([np.random.default_rng(3 + j).uniform(-1, 1, (n, n)) for j in range(4)])
    zero = np.zeros((n, n))
    print(f"\n| {n}^2, levels {L}..5, fp64, Jacobi V(2,2), GCR({RESTART}), to {TOL:g} | P | iterations per column | four solve_refine_gcr rounds, ms | "
          "one solve_multi_refine_gcr call, ms | block / four | same bits | one solve_multi_gcr call: iterations, ms | block / solve_multi_gcr |")
    print("|---|---|---|---|---|---|---|---|---|")
    for what, tname, setter, transfer, _ in problems(pkg, L, (0.5, 0.1, 0.01)):
        with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            setter(mg)
            mg.build_galerkin(transfer)
            ts, tm, tg = [], [], []
            for rep in range(4):                            # the first round captures the graphs and allocates: not timed
                mg.synchronize()
                t0 = time.perf_counter()
                seq = []
                for j in range(4):
                    mg.set_rhs(b[j])
                    mg.set_guess(zero)
                    st, hist = mg.solve_refine_gcr(tol=TOL, max_iters=100, restart=RESTART)
                    seq.append((st, hist, mg.get_solution()))
                t1 = time.perf_counter()
                stats, hists, u = mg.solve_multi_refine_gcr(b, tol=TOL, max_iters=100, restart=RESTART)
                t2 = time.perf_counter()
                gst, _, _ = mg.solve_multi_gcr(b, tol=TOL, max_iters=100, restart=RESTART)
                t3 = time.perf_counter()
                if rep:
                    ts.append((t1 - t0) * 1e3)
                    tm.append((t2 - t1) * 1e3)
                    tg.append((t3 - t2) * 1e3)
            same = all(np.array_equal(u[j], seq[j][2]) and np.array_equal(hists[j], seq[j][1]) for j in range(4))
            ms_s, ms_m, ms_g = statistics.median(ts), statistics.median(tm), statistics.median(tg)
            conv = "" if all(st.converged for st in stats) else " (NOT all converged)"
            gcr = f"{[st.cycles for st in gst]}, {ms_g:.2f}" + ("" if all(st.converged for st in gst) else " (NOT all converged)")
            print(f"| {what} | {tname} | {[st.cycles for st in stats]}{conv} | {ms_s:.2f} (min {min(ts):.2f}, max {max(ts):.2f}) | "
                  f"{ms_m:.2f} (min {min(tm):.2f}, max {max(tm):.2f}) | {ms_m / ms_s:.2f} | {'yes' if same else 'NO'} | {gcr} | {ms_m / ms_g:.2f} |",
                  flush=True)
            # the device's share: stats.seconds of the calls (host copies of the columns excluded for solve_refine_gcr)
            print(f"|   of which in the solve loops: four solve_refine_gcr {sum(s[0].seconds for s in seq) * 1e3:.2f} ms, solve_multi_refine_gcr "
                  f"{stats[0].seconds * 1e3:.2f} ms, solve_multi_gcr {gst[0].seconds * 1e3:.2f} ms (the block calls' copies included) | | | | | | | | |",
                  flush=True)


def run_step(name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    kind, arg = name.split(":")
    if kind == "kernels":
        kernels(pkg, np)
    else:
        solves(pkg, np, int(arg))


if __name__ == "__main__":
    if STEP:
        run_step(STEP)
        sys.exit(0)
    steps = (["kernels:f64"] if ONLY in ("", "kernels") else []) + ([f"solves:{L}" for L in SIZES] if ONLY in ("", "solves") else [])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", step] + (["--quick"] if QUICK else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
