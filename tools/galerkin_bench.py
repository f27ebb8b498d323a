#!/usr/bin/env python3
"""Measurements of the Galerkin hierarchy (op = MGX_OPERATOR_GALERKIN, csrc/mgx_galerkin.hpp) on one MI355X; prints the
markdown kept as profiles/galerkin_kernel_trace_summary.md:
  - k_jacobi_var<T, 9> / k_residual_var<T, 9, 0> at 4096^2 (level 12 of a 13..5 hierarchy): achieved bytes/s over their
    12 sizeof(T) per point, next to the five-point instances <T, 5> (8 sizeof(T)) on a STENCIL5 handle at the same grid;
  - set-up: mgx_build_galerkin at 8192^2 levels 13..5 next to mgx_set_coefficient on a STENCIL5 handle;
  - time to 1e-8 (sine right-hand side as tools/pcg_bench.py): mgx_solve and mgx_solve_pcg at 2047^2 contrast 10 and
    511^2 contrast 100.
Wall times around calls that end in a device synchronise (40 sweeps or 20 residuals per timed call).
    python tools/galerkin_bench.py [--quick]
--transfer: instead, the tables of profiles/opdep_kernel_trace_summary.md - BILINEAR against OPERATOR prolongation
(mgx_build_galerkin_transfer, csrc/mgx_opdep.hpp): mgx_restrict / mgx_prolong_add on the finest level and the one below,
the build, and time and cycles to 1e-8 (constant right-hand side; 2047^2: the random one of seed 3).
--transfer --trace-only: the builds and five calls of each transfer only, for a rocprofv3 --kernel-trace --stats run.
--smoother {jacobi,chebyshev}: instead, the tables of profiles/cheby_kernel_trace_summary.md.  chebyshev: k_cheby_var<T, 5 | 9, FIRST>
(csrc/mgx_cheby.hpp, 10 / 14 sizeof(T) per point and step, one word less on a block's first step) next to
k_jacobi_var<T, 5 | 9> at 4096^2 in the same process, then cycles and time to 1e-8 of mgx_solve and mgx_solve_pcg
with the Chebyshev V(2,2) and V(2,1) cycles (V(2,1): the degrees whose bytes per cycle, 41 words per finest point, are
closest to Jacobi V(2,2)'s 48; V(2,2) moves 56) for both transfers, median of 5.  jacobi: the same solves with the Jacobi
V(2,2) cycle.  --smoother chebyshev --trace-only: five blocks of degree 4 per level and type only, for a
rocprofv3 --kernel-trace --stats run.
--cycle {v,w,f}: instead, the table of profiles/wcycle_kernel_trace_summary.md: the solves of --smoother jacobi (2047^2
contrast 10, 511^2 contrast 100 and 1000, both transfers, Jacobi V(2,2) sweeps) with the cycle index set by
mgx_set_cycle: cycles and median-of-5 time to 1e-8 of mgx_solve and mgx_solve_pcg.  MGX_SMALL_VISIT=0 in the environment:
the W- and F-cycles through the per-level launches only.  --cycle w --trace-only: one solve of that kind at 511^2
contrast 1000 (OPERATOR) only, for a rocprofv3 --kernel-trace --stats run.
--smoother {line_x,line_y,line_alt}: instead, the tables of profiles/line_kernel_trace_summary.md.  The zebra line
kernels k_line_x / k_line_y<T, 5 | 9> (csrc/mgx_line.hpp) at 4096^2 next to k_jacobi_var<T, 5 | 9> in the same process:
ms per colour launch (a sweep is two) and bytes/s over the algorithmic bytes stated in mgx_line.hpp (11 / 15 sizeof(T)
per updated point on five- / nine-point levels, 15 / 19 for k_line_y on a level cut into chunks; a colour launch updates
half the level); k_line_y both with the launcher's chunks and with MGX_LINE_CHUNK set to the whole column.  Then, with
--aniso EPS[,layers] (default 1e-2: the x-strong problem c = 2(1 + EPS), w = e = -1, n = s = -EPS; ",layers": x-strong in
the upper half, y-strong in the lower half), cycles and median-of-5 time to 1e-8 at 2047^2, levels 11..5, right-hand side
default_rng(3).uniform(-1, 1): the line smoother's V(1,1) against Jacobi V(2,2), mgx_solve and mgx_solve_pcg each.
--smoother line_x --trace-only: five sweeps per level and type only, for a rocprofv3 --kernel-trace --stats run.
--smoother {color_gs,color_sgs}: instead, the tables of profiles/colour_gs_kernel_trace_summary.md.  The multicolour
Gauss-Seidel kernels (csrc/mgx_colour.hpp) at 4096^2 next to k_jacobi_var<T, 5 | 9> in the same process, ms per SWEEP:
k_gs_colour<T, 5> (two launches; a handle created under MGX_GS_FUSED=0), k_gs_rb<T> (one launch) and k_gs_colour<T, 9>
(four launches), with the bytes/s over the algorithmic bytes of mgx_colour.hpp (16 / 8 / 24 sizeof(T) per point and
sweep).  Then cycles and median-of-5 time to 1e-8 at 2047^2, levels 11..5, right-hand side default_rng(3).uniform(-1, 1),
of mgx_solve with the smoother's V(1,1) and V(2,2) against Jacobi V(2,2) and Chebyshev V(2,2), on Poisson, contrast 10
with the operator-dependent P, and the rotated anisotropy (45 degrees, eps = 0.5; nine-point finest level).
--smoother color_gs --trace-only: five sweeps per level, type and kernel form only, for a rocprofv3 --kernel-trace
--stats run."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from pcg_ref import contrast_coefficient  # noqa: E402

pkg = ge.load_package()
QUICK = "--quick" in sys.argv
TRACE_ONLY = "--trace-only" in sys.argv
LF = 9 if QUICK else 13          # finest level of the kernel / set-up handles; the timed nine-point level is LF - 1
LK = LF - 1


def wall(f, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def kname(prefix, tag, name, mode=""):
    """the template spelling of a kernel: tag "var" = the five-point instance, "var9" the nine-point one"""
    return f"{prefix}var<{name}, {9 if tag == 'var9' else 5}{mode}>"


def kernels():
    n = (1 << LK) - 1
    x = np.linspace(0.0, 1.0, (1 << LF) + 1)
    a = 1.0 + 0.8 * np.sin(3 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    rng = np.random.default_rng(0)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    print(f"| kernel | grid | dtype | ms per pass | bytes per point | achieved GB/s | fraction of the 8 TB/s HBM peak |")
    print("|---|---|---|---|---|---|---|")
    rate = {}
    for dtype, name, es in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        for op, tag, words, finest in ((pkg.OPERATOR_STENCIL5, "var", 8, LK), (pkg.OP_GALERKIN, "var9", 12, LF)):
            with pkg.Multigrid(finest_level=finest, coarsest_level=5, mu1=2, mu2=2, schedule=pkg.SCHEDULE_V, op=op, dtype=dtype, omega=0.8) as mg:
                if op == pkg.OP_GALERKIN:
                    mg.set_coefficient(a)
                    t0 = time.perf_counter()
                    mg.build_galerkin()
                    rate[("build", name)] = (time.perf_counter() - t0) * 1e3
                else:
                    mg.set_coefficient(a[::2, ::2])
                mg.set_level(LK, pkg.VEC_U, u)
                mg.set_level(LK, pkg.VEC_B, b)
                mg.smooth(LK, 4)
                sweeps = 40
                ms = wall(lambda: mg.smooth(LK, sweeps)) / sweeps
                gbs = words * es * n * n / (ms * 1e-3) / 1e9
                rate[(tag, name)] = gbs
                print(f"| {kname('k_jacobi_', tag, name)} | {1 << LK}^2 | {name} | {ms:.4f} | {words * es} | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
                mg.residual(LK, u, b)
                lib, h = pkg.lib(), mg._h

                def res20():
                    for _ in range(20):
                        lib.mgx_residual(h, LK)
                ms = wall(res20) / 20
                gbs = words * es * n * n / (ms * 1e-3) / 1e9
                print(f"| {kname('k_residual_', tag, name, ', 0')} (one host synchronise per pass) | {1 << LK}^2 | {name} | {ms:.4f} | {words * es} | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
    for name in ("f64", "f32"):
        print(f"\nk_jacobi_var<T, 9> / k_jacobi_var<T, 5> bytes/s, {name}: {rate[('var9', name)] / rate[('var', name)]:.3f} (accepted: >= 0.9)")
    return rate


def setup(rate):
    N = 1 << LF
    a = contrast_coefficient(LF, 10.0)
    print(f"\n| set-up at {N}^2, levels {LF}..5, f64 | ms (wall, one call, after a warm-up call) |\n|---|---|")
    with pkg.Multigrid(finest_level=LF, coarsest_level=5, schedule=0, op=pkg.OP_GALERKIN) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        print(f"| mgx_build_galerkin (R A P on {LF - 5} levels, all splittings, dense inverse of the 31^2 level) | {wall(mg.build_galerkin):.1f} |")
        print(f"| mgx_set_coefficient on the GALERKIN handle (finest level only; includes the host-to-device copy of the nodal coefficient) | {wall(lambda: mg.set_coefficient(a)):.1f} |")
    with pkg.Multigrid(finest_level=LF, coarsest_level=5, schedule=0, op=pkg.OPERATOR_STENCIL5) as mg:
        mg.set_coefficient(a)
        print(f"| mgx_set_coefficient on a STENCIL5 handle (re-discretises every level, splittings, dense inverse; includes the same copy) | {wall(lambda: mg.set_coefficient(a)):.1f} |", flush=True)


def solves():
    print("\n| problem, V(2,2), levels L..5, f64, sine right-hand side | GALERKIN mgx_solve | GALERKIN mgx_solve_pcg |\n|---|---|---|")
    for L, contrast in ((9, 10.0), (9, 100.0)) if QUICK else ((11, 10.0), (9, 100.0)):
        with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            mg.set_coefficient(contrast_coefficient(L, contrast))
            mg.build_galerkin()
            mg.fill_rhs(1)
            cells = []
            for f in (lambda: mg.solve(tol=1e-8, max_cycles=100), lambda: mg.solve_pcg(tol=1e-8, max_iters=200)):
                ts = []
                for rep in range(6):                    # the first run captures the graphs: not timed
                    mg.set_guess(np.zeros((mg.n(), mg.n())))
                    st, h = f()
                    if rep:
                        ts.append(st.seconds * 1e3)
                cells.append(f"{st.cycles} {'it' if len(cells) else 'cycles'}, {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}), converged {st.converged}")
            print(f"| {(1 << L) - 1}^2 contrast {contrast:g} | {cells[0]} | {cells[1]} |", flush=True)


def transfers():
    """words per fine point moved by the algorithm (OPERATOR): fused restriction U, B, A (5 or 9 grids), B_c (1/4), weights
    (2); prolongation U in and out, e (1/4), weights (2).  BILINEAR runs the restriction as two kernels (residual, then
    k_restrict) and its times are the pair's"""
    x = np.linspace(0.0, 1.0, (1 << LF) + 1)
    a = 1.0 + 0.8 * np.sin(3 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    rng = np.random.default_rng(0)
    print("| call | fine grid | transfer | ms per call (one host synchronise each) | words per fine point | achieved GB/s | fraction of 8 TB/s |")
    print("|---|---|---|---|---|---|---|")
    with pkg.Multigrid(finest_level=LF, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN, omega=0.8) as mg:
        mg.set_coefficient(a)
        lib, h = pkg.lib(), mg._h
        for lv in (LK, LF):
            n = (1 << lv) - 1
            mg.set_level(lv, pkg.VEC_U, rng.uniform(-1, 1, (n, n)))
            mg.set_level(lv, pkg.VEC_B, rng.uniform(-1, 1, (n, n)))
        for transfer, tname in ((pkg.TRANSFER_BILINEAR, "BILINEAR"), (pkg.TRANSFER_OPERATOR, "OPERATOR")):
            mg.build_galerkin(transfer)
            build_ms = wall(lambda: mg.build_galerkin(transfer))
            if TRACE_ONLY:                              # under rocprofv3 --kernel-trace --stats: five launches of each kernel
                for lv in (LK, LF):
                    for fn in (lib.mgx_restrict, lib.mgx_prolong_add):
                        for _ in range(5):
                            fn(h, lv)
                continue
            for lv in (LK, LF):
                n = (1 << lv) - 1
                agrids = 9 if lv < LF else 5
                extra = 2.0 if transfer == pkg.TRANSFER_OPERATOR else 0.0
                for fn, label, words in ((lib.mgx_restrict, "mgx_restrict (residual fused in)", 2 + agrids + 0.25 + extra),
                                         (lib.mgx_prolong_add, "mgx_prolong_add", 2 + 0.25 + extra)):
                    fn(h, lv)

                    def rep20():
                        for _ in range(20):
                            fn(h, lv)
                    ms = wall(rep20) / 20
                    gbs = words * 8 * n * n / (ms * 1e-3) / 1e9
                    print(f"| {label} | {1 << lv}^2 | {tname} | {ms:.4f} | {words:g} | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
            print(f"| mgx_build_galerkin_transfer, levels {LF}..5 | {1 << LF}^2 | {tname} | {build_ms:.1f} | | | |", flush=True)
    if TRACE_ONLY:
        return
    print("\n| problem, V(2,2), levels L..5, f64 | transfer | mgx_solve | mgx_solve_pcg |\n|---|---|---|---|")
    for L, contrast in ((9, 10.0), (9, 100.0), (9, 1000.0)) if QUICK else ((11, 10.0), (9, 100.0), (9, 1000.0)):
        n = (1 << L) - 1
        b = np.random.default_rng(3).standard_normal((n, n)) if L == 11 else None
        with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
            mg.set_coefficient(contrast_coefficient(L, contrast))
            for transfer, tname in ((pkg.TRANSFER_BILINEAR, "BILINEAR"), (pkg.TRANSFER_OPERATOR, "OPERATOR")):
                mg.build_galerkin(transfer)
                if b is None:
                    mg.fill_rhs(0)
                else:
                    mg.set_rhs(b)
                cells = []
                for f in (lambda: mg.solve(tol=1e-8, max_cycles=150), lambda: mg.solve_pcg(tol=1e-8, max_iters=200)):
                    ts = []
                    for rep in range(6):                    # the first run captures the graphs: not timed
                        mg.set_guess(np.zeros((n, n)))
                        st, hist = f()
                        if rep:
                            ts.append(st.seconds * 1e3)
                    cells.append(f"{st.cycles} {'it' if len(cells) else 'cycles'}, {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}), converged {st.converged}")
                print(f"| {n}^2 contrast {contrast:g} | {tname} | {cells[0]} | {cells[1]} |", flush=True)


def smoother_kernels():
    n = (1 << LK) - 1
    x = np.linspace(0.0, 1.0, (1 << LF) + 1)
    a = 1.0 + 0.8 * np.sin(3 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    rng = np.random.default_rng(0)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    if not TRACE_ONLY:
        print("| kernel | grid | dtype | ms per step | bytes per point | achieved GB/s | fraction of the 8 TB/s HBM peak |")
        print("|---|---|---|---|---|---|---|")
    rate = {}
    steps = 40
    for dtype, name, es in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        for op, tag, finest in ((pkg.OPERATOR_STENCIL5, "var", LK), (pkg.OP_GALERKIN, "var9", LF)):
            for sm, prefix, words in ((pkg.SMOOTHER_JACOBI, "k_jacobi_", 8 if tag == "var" else 12),
                                     (pkg.SMOOTHER_CHEBYSHEV, "k_cheby_", 10 if tag == "var" else 14)):
                with pkg.Multigrid(finest_level=finest, coarsest_level=5, mu1=2, mu2=2, schedule=pkg.SCHEDULE_V, op=op, dtype=dtype, omega=0.8,
                                   smoother=sm) as mg:
                    if op == pkg.OP_GALERKIN:
                        mg.set_coefficient(a)
                        mg.build_galerkin()
                    else:
                        mg.set_coefficient(a[::2, ::2])
                    mg.set_level(LK, pkg.VEC_U, u)
                    mg.set_level(LK, pkg.VEC_B, b)
                    mg.smooth(LK, 4)
                    if TRACE_ONLY:
                        for _ in range(5):
                            mg.smooth(LK, 4)
                        continue
                    ms = wall(lambda: mg.smooth(LK, steps), reps=5) / steps
                    # a Chebyshev block's first step does not read d: one word less in `steps` steps
                    per_step = words - (1.0 / steps if sm == pkg.SMOOTHER_CHEBYSHEV else 0.0)
                    gbs = per_step * es * n * n / (ms * 1e-3) / 1e9
                    rate[(prefix, tag, name)] = gbs
                    print(f"| {kname(prefix, tag, name)} | {1 << LK}^2 | {name} | {ms:.4f} | {per_step * es:.1f} | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
    if TRACE_ONLY:
        return
    print()
    for name in ("f64", "f32"):
        for tag in ("var", "var9"):
            r = rate[("k_cheby_", tag, name)] / rate[("k_jacobi_", tag, name)]
            print(f"{kname('k_cheby_', tag, 'T')} / {kname('k_jacobi_', tag, 'T')} bytes/s, {name}: {r:.3f} (accepted: >= 0.9{'' if r >= 0.9 else ': NOT MET'})")


LINE = {"line_x": pkg.SMOOTHER_LINE_X, "line_y": pkg.SMOOTHER_LINE_Y, "line_alt": pkg.SMOOTHER_LINE_ALT}


def line_kernels(which):
    """which: line_x, line_y or line_alt (both kernels)"""
    n = (1 << LK) - 1
    x = np.linspace(0.0, 1.0, (1 << LF) + 1)
    a = 1.0 + 0.8 * np.sin(3 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    rng = np.random.default_rng(0)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    chunked = (1 << LK) > 64                               # the launcher cuts the columns of this level (line_chunk_rows)
    if not TRACE_ONLY:
        print("| kernel | grid | dtype | ms per launch | bytes per updated point | points per launch | achieved GB/s | fraction of the 8 TB/s HBM peak |")
        print("|---|---|---|---|---|---|---|---|")
    rate = {}
    sweeps = 20
    runs = [("k_jacobi_", pkg.SMOOTHER_JACOBI, None)]
    if which in ("line_x", "line_alt"):
        runs.append(("k_line_x", pkg.SMOOTHER_LINE_X, None))
    if which in ("line_y", "line_alt"):
        runs += [("k_line_y", pkg.SMOOTHER_LINE_Y, None), ("k_line_y", pkg.SMOOTHER_LINE_Y, str(1 << LF))]
    for dtype, name, es in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        for op, tag, finest in ((pkg.OPERATOR_STENCIL5, "var", LK), (pkg.OP_GALERKIN, "var9", LF)):
            nq = 9 if tag == "var9" else 5
            for prefix, sm, chunk in runs:
                if chunk is None:
                    os.environ.pop("MGX_LINE_CHUNK", None)
                else:
                    os.environ["MGX_LINE_CHUNK"] = chunk      # read at mgx_create: the whole column as one chunk
                with pkg.Multigrid(finest_level=finest, coarsest_level=5, mu1=2, mu2=2, schedule=pkg.SCHEDULE_V, op=op, dtype=dtype, omega=0.8,
                                   smoother=sm) as mg:
                    os.environ.pop("MGX_LINE_CHUNK", None)
                    if op == pkg.OP_GALERKIN:
                        mg.set_coefficient(a)
                        mg.build_galerkin()
                    else:
                        mg.set_coefficient(a[::2, ::2])
                    mg.set_level(LK, pkg.VEC_U, u)
                    mg.set_level(LK, pkg.VEC_B, b)
                    mg.smooth(LK, 2)
                    if TRACE_ONLY:
                        mg.smooth(LK, 5)
                        continue
                    ms = wall(lambda: mg.smooth(LK, sweeps), reps=5) / sweeps
                    if sm == pkg.SMOOTHER_JACOBI:
                        words, launches, label = (8 if nq == 5 else 12), 1, kname(prefix, tag, name)
                    else:
                        cut = prefix == "k_line_y" and chunked and chunk is None
                        words, launches = (11 if nq == 5 else 15) + (4 if cut else 0), 2
                        label = f"{prefix}<{name}, {nq}>" + ("" if prefix == "k_line_x" else " (launcher's chunks)" if cut else " (one chunk per column)")
                    ms /= launches
                    gbs = words * es * (n * n / launches) / (ms * 1e-3) / 1e9
                    rate[(label, tag, name)] = gbs
                    print(f"| {label} | {1 << LK}^2 | {name} | {ms:.4f} | {words * es} | 1/{launches} of the level | {gbs:.0f} | {gbs / 8000:.3f} |", flush=True)
    if TRACE_ONLY:
        return
    print()
    for (label, tag, name), gbs in rate.items():
        if label.startswith("k_jacobi_"):
            continue
        r = gbs / rate[(kname("k_jacobi_", tag, name), tag, name)]
        print(f"{label} / {kname('k_jacobi_', tag, name)} bytes/s: {r:.3f}{'' if r >= 0.5 else ' (BELOW HALF: open item)'}")


def aniso_solves(which, eps, layers):
    import line_ref
    L = 9 if QUICK else 11
    n = (1 << L) - 1
    st5 = line_ref.aniso_stencil(L, eps, "layers" if layers else "x")
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    what = f"layers, eps = {eps:g}" if layers else f"x-strong, eps = {eps:g}"
    print(f"\n| {n}^2, {what}, levels {L}..5, f64, BILINEAR | mgx_solve (cap 100 cycles) | mgx_solve_pcg (cap 300 iterations) |\n|---|---|---|")
    for label, sm, mu in ((f"{which} V(1,1)", LINE[which], 1), ("Jacobi V(2,2), omega = 2/3", pkg.SMOOTHER_JACOBI, 2)):
        with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=mu, mu2=mu, schedule=0, op=pkg.OP_GALERKIN, smoother=sm) as mg:
            mg.set_stencil(L, *st5)
            mg.build_galerkin()
            mg.set_rhs(b)
            cells = []
            for f in (lambda: mg.solve(tol=1e-8, max_cycles=100), lambda: mg.solve_pcg(tol=1e-8, max_iters=300)):
                ts = []
                for rep in range(6):                    # the first run captures the graphs: not timed
                    mg.set_guess(np.zeros((n, n)))
                    st, hist = f()
                    if rep:
                        ts.append(st.seconds * 1e3)
                cells.append(f"{st.cycles} {'it' if len(cells) else 'cycles'}, {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}), "
                             f"converged {st.converged}, residual ratio {hist[-1] / hist[0]:.1e}")
            print(f"| {label} | {cells[0]} | {cells[1]} |", flush=True)


COLOUR = {"color_gs": pkg.SMOOTHER_COLOR_GS, "color_sgs": pkg.SMOOTHER_COLOR_SGS}


def colour_kernels(which):
    n = (1 << LK) - 1
    x = np.linspace(0.0, 1.0, (1 << LF) + 1)
    a = 1.0 + 0.8 * np.sin(3 * np.pi * x)[None, :] * np.cos(2 * np.pi * x)[:, None]
    rng = np.random.default_rng(0)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    if not TRACE_ONLY:
        print("| kernel | grid | dtype | launches per sweep | ms per sweep | bytes per point and sweep | achieved GB/s | fraction of the 8 TB/s HBM peak | sweep time / Jacobi sweep time |")
        print("|---|---|---|---|---|---|---|---|---|")
    sweeps = 20
    for dtype, name, es in ((pkg.DTYPE_F64, "f64", 8), (pkg.DTYPE_F32, "f32", 4)):
        for op, tag, finest in ((pkg.OPERATOR_STENCIL5, "var", LK), (pkg.OP_GALERKIN, "var9", LF)):
            nq = 9 if tag == "var9" else 5
            runs = [(kname("k_jacobi_", tag, name), pkg.SMOOTHER_JACOBI, None, 1, nq + 3)]
            if nq == 5:
                runs += [(f"k_gs_colour<{name}, 5>", COLOUR[which], "0", 2, 16), (f"k_gs_rb<{name}>", COLOUR[which], None, 1, 8)]
            else:
                runs += [(f"k_gs_colour<{name}, 9>", COLOUR[which], None, 4, 24)]
            jacobi_ms = None
            for label, sm, fused, launches, words in runs:
                if fused is None:
                    os.environ.pop("MGX_GS_FUSED", None)
                else:
                    os.environ["MGX_GS_FUSED"] = fused          # read at mgx_create
                with pkg.Multigrid(finest_level=finest, coarsest_level=5, mu1=2, mu2=2, schedule=pkg.SCHEDULE_V, op=op, dtype=dtype, omega=0.8,
                                   smoother=sm) as mg:
                    os.environ.pop("MGX_GS_FUSED", None)
                    if op == pkg.OP_GALERKIN:
                        mg.set_coefficient(a)
                        mg.build_galerkin()
                    else:
                        mg.set_coefficient(a[::2, ::2])
                    mg.set_level(LK, pkg.VEC_U, u)
                    mg.set_level(LK, pkg.VEC_B, b)
                    mg.smooth(LK, 2)
                    if TRACE_ONLY:
                        mg.smooth(LK, 5)
                        continue
                    ms = wall(lambda: mg.smooth(LK, sweeps), reps=5) / sweeps
                    if jacobi_ms is None:
                        jacobi_ms = ms
                    gbs = words * es * n * n / (ms * 1e-3) / 1e9
                    print(f"| {label} | {1 << LK}^2 | {name} | {launches} | {ms:.4f} | {words * es} | {gbs:.0f} | {gbs / 8000:.3f} | {ms / jacobi_ms:.3f} |", flush=True)


def colour_solves(which):
    import nine_ref
    L = 9 if QUICK else 11
    n = (1 << L) - 1
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    one = np.ones((n, n))
    problems = (("Poisson", "BILINEAR", lambda mg: mg.set_stencil(L, 4 * one, -one, -one, -one, -one), None),
                ("contrast 10", "OPERATOR", lambda mg: mg.set_coefficient(contrast_coefficient(L, 10.0)), pkg.TRANSFER_OPERATOR),
                ("rotated anisotropy 45 degrees, eps = 0.5", "BILINEAR", lambda mg: mg.set_tensor(*nine_ref.rotated_tensor(L, 45.0, 0.5)), None))
    cycles = ((f"{which} V(1,1)", COLOUR[which], 1), (f"{which} V(2,2)", COLOUR[which], 2), ("Jacobi V(2,2), omega = 2/3", pkg.SMOOTHER_JACOBI, 2),
              ("Chebyshev V(2,2)", pkg.SMOOTHER_CHEBYSHEV, 2))
    print(f"\n| {n}^2, levels {L}..5, f64, mgx_solve to 1e-8 (cap 100 cycles) | transfer | " + " | ".join(c[0] for c in cycles) + " |")
    print("|---|---|" + "---|" * len(cycles))
    for pname, tname, setter, transfer in problems:
        cells = []
        for label, sm, mu in cycles:
            with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=mu, mu2=mu, schedule=0, op=pkg.OP_GALERKIN, smoother=sm) as mg:
                setter(mg)
                mg.build_galerkin(transfer)
                mg.set_rhs(b)
                ts = []
                for rep in range(6):                    # the first run captures the graphs: not timed
                    mg.set_guess(np.zeros((n, n)))
                    st, hist = mg.solve(tol=1e-8, max_cycles=100)
                    if rep:
                        ts.append(st.seconds * 1e3)
                cells.append(f"{st.cycles} cycles, {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}), converged {st.converged}")
        print(f"| {pname} | {tname} | " + " | ".join(cells) + " |", flush=True)


CYCLES = {"v": pkg.CYCLE_V, "w": pkg.CYCLE_W, "f": pkg.CYCLE_F}


def trace_one_solve(cycle):
    L = 9
    with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=pkg.OP_GALERKIN) as mg:
        mg.set_coefficient(contrast_coefficient(L, 1000.0))
        mg.build_galerkin(pkg.TRANSFER_OPERATOR)
        if cycle != "v":
            mg.set_cycle(CYCLES[cycle])
        mg.fill_rhs(0)
        st, hist = mg.solve(tol=1e-8, max_cycles=150)
        print(f"one {cycle.upper()} solve at 511^2 contrast 1000, OPERATOR: {st.cycles} cycles, converged {st.converged}")


def smoother_solves(which, cycle=None):
    """cycle: None (the tables of --smoother) or the kind of --cycle"""
    sm = pkg.SMOOTHER_CHEBYSHEV if which == "chebyshev" else pkg.SMOOTHER_JACOBI
    kind = (cycle or "v").upper()
    print(f"\n| problem, levels L..5, f64, smoother {which} | cycle | transfer | mgx_solve | mgx_solve_pcg |\n|---|---|---|---|---|")
    for L, contrast in ((9, 10.0), (9, 100.0), (9, 1000.0)) if QUICK else ((11, 10.0), (9, 100.0), (9, 1000.0)):
        n = (1 << L) - 1
        b = np.random.default_rng(3).standard_normal((n, n)) if L == 11 else None
        for mu1, mu2 in ((2, 2), (2, 1)) if which == "chebyshev" else ((2, 2),):
            with pkg.Multigrid(finest_level=L, coarsest_level=5, mu1=mu1, mu2=mu2, schedule=0, op=pkg.OP_GALERKIN, smoother=sm) as mg:
                mg.set_coefficient(contrast_coefficient(L, contrast))
                if cycle not in (None, "v"):                # (v: the handle's default, no call)
                    mg.set_cycle(CYCLES[cycle])
                for transfer, tname in ((pkg.TRANSFER_BILINEAR, "BILINEAR"), (pkg.TRANSFER_OPERATOR, "OPERATOR")):
                    mg.build_galerkin(transfer)
                    if b is None:
                        mg.fill_rhs(0)
                    else:
                        mg.set_rhs(b)
                    cells = []
                    for f in (lambda: mg.solve(tol=1e-8, max_cycles=150), lambda: mg.solve_pcg(tol=1e-8, max_iters=200)):
                        ts = []
                        for rep in range(6):                    # the first run captures the graphs: not timed
                            mg.set_guess(np.zeros((n, n)))
                            st, hist = f()
                            if rep:
                                ts.append(st.seconds * 1e3)
                        cells.append(f"{st.cycles} {'it' if len(cells) else 'cycles'}, {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}), converged {st.converged}")
                    print(f"| {n}^2 contrast {contrast:g} | {kind}({mu1},{mu2}) | {tname} | {cells[0]} | {cells[1]} |", flush=True)


if __name__ == "__main__":
    if "--cycle" in sys.argv:
        kind = sys.argv[sys.argv.index("--cycle") + 1]
        if kind not in CYCLES:
            sys.exit("--cycle v, w or f")
        if TRACE_ONLY:
            trace_one_solve(kind)
        else:
            smoother_solves("jacobi", kind)
    elif "--smoother" in sys.argv:
        which = sys.argv[sys.argv.index("--smoother") + 1]
        if which in LINE:
            if "--aniso" in sys.argv:
                spec = sys.argv[sys.argv.index("--aniso") + 1].split(",")
                aniso_solves(which, float(spec[0]), "layers" in spec[1:])
            else:
                line_kernels(which)
                if not TRACE_ONLY:
                    aniso_solves(which, 1e-2, which == "line_alt")
            sys.exit(0)
        if which in COLOUR:
            colour_kernels(which)
            if not TRACE_ONLY:
                colour_solves(which)
            sys.exit(0)
        if which not in ("jacobi", "chebyshev"):
            sys.exit("--smoother jacobi, chebyshev, line_x, line_y, line_alt, color_gs or color_sgs")
        if which == "chebyshev":
            smoother_kernels()
        if not TRACE_ONLY:
            smoother_solves(which)
    elif "--transfer" in sys.argv:
        transfers()
    else:
        r = kernels()
        setup(r)
        solves()
