#!/usr/bin/env python3
"""Time to a relative residual of 1e-8: mgx_solve_pcg (CG preconditioned by one V-cycle per iteration) against
mgx_solve (plain V-cycles) on the same handle configuration, right-hand side (sine, mgx_fill_rhs kind 1) and
zero guess.  One JSON line per configuration: iterations / cycles, wall time (stats.seconds: device-synchronised,
graph replay on) as median, min and max over --repeats runs after a warm-up of each, and ms per iteration.

    python tools/pcg_bench.py [--repeats 5] [--only NAME[,NAME]]

The split between the V-cycle and the k_pcg_* Krylov passes comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/pcg_bench.py --only ... --repeats 1` run
(summary: profiles/pcg_kernel_trace_summary.md)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
from pcg_ref import contrast_coefficient  # noqa: E402

CONFIGS = {
    "8192_fma_V10_10": dict(finest_level=13, coarsest_level=7, mu1=10, mu2=10, arith=1),
    "4096_V21": dict(finest_level=12, coarsest_level=7, mu1=2, mu2=1, arith=1),
    "8192_rbgs_V21": dict(finest_level=13, coarsest_level=7, mu1=2, mu2=1, smoother=1),
    "2047_stencil5_c10_V22": dict(finest_level=11, coarsest_level=5, mu1=2, mu2=2, op=1, contrast=10.0),
}


def timed(mg, L, fn, repeats):
    out = []
    for _ in range(repeats):
        mg.zero_level(L, 0)
        st, h = fn()
        out.append((st.seconds, st.cycles, bool(st.converged), float(h[-1] / h[0])))
    secs = [o[0] for o in out]
    its = out[-1][1]
    return {"iters": its, "converged": out[-1][2], "rel_residual": out[-1][3],
            "s_median": statistics.median(secs), "s_min": min(secs), "s_max": max(secs),
            "ms_per_iter": 1e3 * statistics.median(secs) / max(its, 1), "runs": len(secs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--max-cycles", type=int, default=60)
    a = ap.parse_args()
    pkg = ge.load_package()
    names = [n for n in CONFIGS if not a.only or n in a.only.split(",")]
    for name in names:
        c = dict(CONFIGS[name])
        contrast = c.pop("contrast", None)
        L = c["finest_level"]
        cfg = dict(mu0=0, schedule=pkg.SCHEDULE_V, profile=0, **c)
        with pkg.Multigrid(**cfg) as mg:
            if contrast is not None:
                mg.set_coefficient(contrast_coefficient(L, contrast))
            mg.fill_rhs(1)
            pcg = lambda: mg.solve_pcg(tol=1e-8, max_iters=200)                    # noqa: E731
            vc = lambda: mg.solve(tol=1e-8, max_cycles=a.max_cycles)              # noqa: E731
            timed(mg, L, pcg, 1)                                                  # warm-up: graphs captured
            timed(mg, L, vc, 1)
            rp = timed(mg, L, pcg, a.repeats)
            rv = timed(mg, L, vc, a.repeats)
        rec = {"config": name, "n": (1 << L) - 1, "cfg": c, "contrast": contrast, "tol": 1e-8, "pcg": rp, "vcycles": rv,
               "pcg_time_over_vcycles": (rp["s_median"] / rv["s_median"]) if rv["converged"] else None}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
