"""Every configuration whose timings the project publishes (tools/run_configs.py ROWS), built as bench.py builds it
(tests/bench_cfg.py: profile = 2, V-cycles, the row's rounding mode), against the CPU oracle at its own size.

These sizes select code paths the small parity tests never reach: the float 10-level passes with launcher-sized
chunks and the paired geometry, the float "norm apart" post-smoothing pass, the shallow passes in 48- and 96-row
chunks, k_update_residual and fold_kmax_big at full size.  Per row and rounding mode:
  * inputs generated on the device as bench.py does (fill_rhs(1), fill_guess_random(12345)), read back for the oracle;
  * one warm-up cycle, the guess filled again, then the measured solve - bench.py's order, so the cycles checked are
    replays of the captured graph where the configuration has one;
  * residual history against the oracle (1e-10 per cycle plus the floor of test_gpu_solve.hist_close); the iterate
    bit-exact in fp32 (every float operator and the sine-transform bottom solve follow the oracle's operations),
    to 1e-12 of its maximum in f64 and mixed (the f64 bottom solves are two different exact methods);
  * the same solve with profile = 0 (mgx_solve's default: the whole cycle as one graph replay): the same bits;
  * the first history entry against ||b - A u0|| evaluated here in numpy (tests/np_ref.py), independently of both.
Float and mixed rows run in both rounding modes: their pass plans differ by mode."""
import os

import numpy as np
import pytest

import bench_cfg
import np_ref
from test_gpu_solve import hist_close, oracle_cfg

pytestmark = pytest.mark.gpu

# (row flags, rounding mode) whose oracle run another test already makes on the same grid with the same configuration
# (there: inputs set from the host, profile 0).  Here those pairs keep the device-only checks - profile 2 against
# profile 0 and the independent first residual - which tie the benchmarked path to that test's oracle comparison.
HELD = {
    ("--level 13 --mu1 10 --mu2 10", "fma"): "test_gpu_fma.py::test_full_size_fma_cycles_against_the_oracle[bench]",
    ("--level 12 --coarsest 7 --mu1 2 --mu2 1", "fma"): "test_gpu_fma.py::test_full_size_fma_cycles_against_the_oracle[config2]",
    # red-black Gauss-Seidel has no rounding modes
    ("--level 13 --smoother rbgs --mu1 2 --mu2 1", "fma"): "test_gpu_solve.py::test_full_size_cycles_against_the_oracle[config3]",
}
MEM_L14_GIB = 32          # the oracle peaks at 13.3 GB at 16384^2, the read-back arrays add about 6 GB


def _cases():
    out = []
    for name, flags in bench_cfg.rows():
        a = bench_cfg.parse(flags)
        modes = [a.arith] if "--arith" in flags.split() else (["fma", "separate"] if a.dtype != "f64" else ["fma"])
        for mode in modes:
            tag = f"L{a.level}-{a.coarsest}-{a.smoother}-{a.dtype}-V{a.mu1},{a.mu2}-{mode}"
            out.append(pytest.param(name, flags, mode, id=tag))
    return out


def _mem_available_gib():
    with open("/proc/meminfo") as fh:
        for line in fh:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / (1 << 20)
    return 0.0


def _residual_norm(u, b, rows=512):
    """||b - A u||_2 in float64 (np_ref's statement of A), squares summed in long double; row blocks with one halo
    row on each side keep the temporaries small on the largest grids"""
    n = u.shape[0]
    acc = np.longdouble(0.0)
    for i0 in range(0, n, rows):
        i1 = min(i0 + rows, n)
        lo, hi = max(i0 - 1, 0), min(i1 + 1, n)
        r = np_ref.residual(u[lo:hi].astype(np.float64), b[lo:hi].astype(np.float64))[i0 - lo:i1 - lo]
        acc += np.sum(np.square(r.astype(np.longdouble)))
    return float(np.sqrt(acc))


def _bench_solve(pkg, cfg, cycles, inputs):
    """bench.py's sequence on one handle; returns (history, iterate, b, u0) - b and u0 only when `inputs`"""
    L = cfg["finest_level"]
    b = u0 = None
    with pkg.Multigrid(**cfg) as mg:
        mg.fill_rhs(1, 0.0)
        mg.fill_guess_random(12345)
        if inputs:
            b = mg.get_level(L, pkg.VEC_B)
            u0 = mg.get_solution()
        mg.solve(tol=0.0, max_cycles=1)
        mg.fill_guess_random(12345)
        st, h = mg.solve(tol=0.0, max_cycles=cycles)
        u = mg.get_solution()
    assert st.cycles == cycles and len(h) == cycles + 1
    return h, u, b, u0


@pytest.mark.parametrize("name,flags,mode", _cases())
def test_benchmarked_configuration_matches_the_oracle(pkg, po, name, flags, mode):
    cfg = bench_cfg.config(pkg, flags, arith=mode)
    L = cfg["finest_level"]
    if L >= 14 and _mem_available_gib() < MEM_L14_GIB:
        pytest.skip(f"{name}: the oracle at 16384^2 needs about {MEM_L14_GIB} GiB of host memory, "
                    f"{_mem_available_gib():.1f} GiB available")
    cycles = 1 if L >= 14 else 2
    f32 = cfg["dtype"] == pkg.DTYPE_F32

    h, u, b, u0 = _bench_solve(pkg, cfg, cycles, inputs=True)
    # the first entry, independently of the oracle: the norm kernel on 16 M - 268 M points
    r0 = _residual_norm(u0, b)
    assert abs(h[0] - r0) <= (1e-5 if f32 else 1e-12) * r0, (h[0], r0)

    # profile = 0: the graph-replay default of mgx_solve, the same bits
    h0, u_p0, _, _ = _bench_solve(pkg, dict(cfg, profile=0), cycles, inputs=False)
    assert np.array_equal(u, u_p0), "profile 2 and profile 0 iterates differ"
    assert np.allclose(h, h0, rtol=1e-13, atol=0), (h, h0)
    del u_p0

    if (flags, mode) in HELD:
        return                 # this configuration's oracle run: the test named in HELD
    ocfg = oracle_cfg(po, {k: v for k, v in cfg.items() if k != "profile"})
    orc = po.Solver(**ocfg)
    u_ref, h_ref = orc.solve(b.astype(np.float64, copy=False), u0.astype(np.float64, copy=False), tol=0.0, max_cycles=cycles)
    orc.close()
    del b, u0
    assert hist_close(h, h_ref), (h, h_ref)
    if f32:
        assert np.array_equal(u.astype(np.float64), u_ref), \
            f"fp32 iterate differs from the oracle at {np.count_nonzero(u.astype(np.float64) != u_ref)} points"
    else:
        scale = float(np.max(np.abs(u_ref)))
        assert float(np.max(np.abs(u - u_ref))) <= 1e-12 * scale
