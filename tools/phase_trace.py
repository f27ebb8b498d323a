"""Where does the time go inside the latency-bound kernels of the V-cycle's tail?  Needs the debug build
(make -C multigrid_nikhil_c-_amd/csrc trace -> libmgx_trace.so): wave 0 of every workgroup of k_dst_pair and
k_tile_wide stamps the 100 MHz wall clock at its phase boundaries (csrc/mgx_phase_trace.hpp).  Runs a few V(10,10)
cycles of the bench hierarchy (finest level given, coarsest 7) and prints, per kernel instantiation, the median over
workgroups of every phase in us, and of a launch's span (first entry to last exit) as a markdown table.

    MGX_LIBMGX_PATH=$PWD/multigrid_nikhil_c-_amd/libmgx_trace.so python tools/phase_trace.py 13
"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 13
KMAX, CAP = 24, 1 << 14


class PT(C.Structure):
    _fields_ = [("kind", C.c_int), ("tag", C.c_int), ("block", C.c_int), ("n", C.c_int), ("t", C.c_longlong * KMAX)]


with pkg.Multigrid(finest_level=L, coarsest_level=7, mu0=0, mu1=10, mu2=10, schedule=0, profile=1, arith=pkg.ARITH_FMA) as mg:
    mg.fill_rhs(1, 0.0)
    mg.fill_guess_random(1)
    mg.solve(tol=0.0, max_cycles=4)
    mg.synchronize()
    lib = pkg.binding.lib()
    buf = (PT * CAP)()
    lib.mgx_debug_phase_trace.restype = C.c_int
    n = lib.mgx_debug_phase_trace(C.byref(buf), CAP)
if n <= 0:
    sys.exit(f"no phase records ({n}): is MGX_LIBMGX_PATH the trace build?")
rec = np.frombuffer(buf, dtype=np.dtype([("kind", "i4"), ("tag", "i4"), ("block", "i4"), ("n", "i4"), ("t", "i8", (KMAX,))]))[:n]


def names(kind, tag, nst):
    if kind == 0:       # k_dst_pair: entry, [batch landed]*, sum 1, barrier, [batch landed]*, sum 2, exit
        nb = (nst - 5) // 2
        return [f"p1 batch {q} landed" for q in range(nb)] + ["p1 sum done", "barrier"] + \
               [f"p2 batch {q} landed" for q in range(nb)] + ["p2 sum done", "store + exit"]
    post = (tag >> 20) & 15
    lv = nst - 6 - (1 if post else 0)
    return ["geometry", "rhs band landed", "band landed + correction"] + [f"level {q + 1}" for q in range(lv)] + ["store"] + \
           (["residual"] if post else []) + ["POST stage + exit"]


def label(kind, tag):
    if kind == 0:
        return f"k_dst_pair<{'FIRST' if tag >> 16 else 'second'}> n={tag & 0xffff}"
    return f"k_tile_wide N={tag & 0xffff} PRE={(tag >> 16) & 15} POST={(tag >> 20) & 15} RW={tag >> 24}"


print(f"phase trace, finest level {L}: {n} workgroup records (100 MHz clock: 0.01 us resolution)\n")
for kind, tag in sorted({(int(r["kind"]), int(r["tag"])) for r in rec}):
    g = rec[(rec["kind"] == kind) & (rec["tag"] == tag)]
    nst = int(np.median(g["n"]))
    g = g[g["n"] == nst]
    t = g["t"][:, :nst].astype(np.float64) / 100.0
    d = np.diff(t, axis=1)
    # launches: the records' entry times cluster per launch (a cycle is > 1 ms, a launch < 0.1 ms)
    order = np.argsort(t[:, 0])
    cuts = np.nonzero(np.diff(t[order, 0]) > 50.0)[0] + 1
    spans = [t[idx, -1].max() - t[idx, 0].min() for idx in np.split(order, cuts)]
    wgs = int(np.median([len(idx) for idx in np.split(order, cuts)]))
    print(f"### {label(kind, tag)}: {wgs} workgroups x {len(spans)} launches; launch span median {np.median(spans):.2f} us; "
          f"workgroup entry to exit median {np.median(t[:, -1] - t[:, 0]):.2f} us\n")
    print("| phase | median us | p90 us | cumulative us |")
    print("|---|---|---|---|")
    cum = 0.0
    for q, nm in enumerate(names(kind, tag, nst)):
        m = float(np.median(d[:, q]))
        cum += m
        print(f"| {nm} | {m:.2f} | {np.percentile(d[:, q], 90):.2f} | {cum:.2f} |")
    print()
