"""k_tile_wide (the wide register tiles of the small levels, MGX_TILE_WIDE=2) against k_tile_smooth (MGX_TILE_WIDE=0)
through the slab C-ABI: every (PRE, POST) stage pair, Jacobi in both rounding modes and red-black GS, fp64 and fp32,
zero_in, whole grids and an interior row window, N = 128 .. 2048 (tiles of 56 x 104 / 40 x 104 / 40 x 232 nodes: the
last tile row and column are partial at every size).  The iterate, the restricted coarse residual and the zeroed coarse
guess must be the same bits; the norm (a sum over differently shaped tiles) agrees to rounding.  Then the bench's V(10,10)
at 8192^2 with the levels up to 1024^2 on k_tile_wide, against the oracle and bit for bit against k_tile_smooth."""
import ctypes as C

import numpy as np
import pytest

import hipmem as hm
from test_gpu_slabs import grid_from_interior
from test_gpu_solve import hist_close, run_gpu

pytestmark = pytest.mark.gpu

STAGES = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]


def _slab_cycle(pkg, level, dt, arith, kind, mu, pre, post, zero_in, window, wide, monkeypatch, seed=5):
    monkeypatch.setenv("MGX_TILE_WIDE", "2" if wide else "0")      # 2: fp32 levels too
    monkeypatch.setenv("MGX_SLAB_TILE_POINTS", str(1 << 24))      # every range here on the register tiles
    L = pkg.lib()
    N, NC = 1 << level, 1 << (level - 1)
    code = pkg.DTYPE_F64 if dt == np.float64 else pkg.DTYPE_F32
    rng = np.random.default_rng(seed + level)
    v = rng.uniform(-1, 1, (N - 1, N - 1)).astype(dt)
    f = rng.uniform(-1, 1, (N - 1, N - 1)).astype(dt)
    e = rng.uniform(-1, 1, (NC - 1, NC - 1)).astype(dt)
    u = grid_from_interior(pkg, v, level, dt)
    b = grid_from_interior(pkg, f, level, dt)
    ce = grid_from_interior(pkg, e, level - 1, dt)
    cb = grid_from_interior(pkg, np.full((NC - 1, NC - 1), 7, dt), level - 1, dt)
    tmp = hm.zeros_like(u)
    fs = pkg.Slab(level=level, dtype=code, rows=N + 1, row0=0, arith=arith)
    cs = pkg.Slab(level=level - 1, dtype=code, rows=NC + 1, row0=0, arith=arith)
    scratch = hm.zeros(int(L.mgx_slab_scratch_doubles(C.byref(fs))), np.float64)
    out = hm.zeros(1, np.float64)
    # whole grid, or the rows [N/4 + 1, N/2 + 1) (an odd first row, as the folded restriction wants)
    rl, rh = (1, N) if not window else (N // 4 + 1, N // 2 + 1)
    crl, crh = (1, NC) if not window else (N // 8 + 1, N // 4 + 1)
    flag = C.c_int()
    st = L.mgx_slab_cycle(C.byref(fs), u.data_ptr(), b.data_ptr(), tmp.data_ptr(), rl, rh, mu, 2.0 / 3.0, kind,
                          C.byref(cs), ce.data_ptr() if pre else None, cb.data_ptr() if post == 1 else None, crl, crh, 0,
                          zero_in, scratch.data_ptr() if post == 2 else None, out.data_ptr() if post == 2 else None,
                          C.byref(flag), None)
    hm.synchronize()
    assert st == 0
    return (tmp if flag.value else u).cpu().numpy(), cb.cpu().numpy(), float(out.item())


@pytest.mark.parametrize("level", [7, 8, 9, 10, 11])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("smoother", ["jacobi", "jacobi_fma", "rbgs"])
def test_wide_tiles_equal_the_narrow_tiles_bit_for_bit(pkg, monkeypatch, level, dt, smoother):
    kind = pkg.SMOOTHER_RBGS if smoother == "rbgs" else pkg.SMOOTHER_JACOBI
    arith = 1 if smoother == "jacobi_fma" else 0
    per = 2 if smoother == "rbgs" else 1
    # one launch of 10 levels, and a block of three launches (mu beyond MGX_TILE_K's 10 levels, whole grids only)
    for pre, post in STAGES:
        for mu, window in ((10 // per, False), (10 // per, True), (25 // per, False)):
            for zero_in in ((0, 1) if not pre else (0,)):
                args = (pkg, level, dt, arith, kind, mu, pre, post, zero_in, window)
                u0, c0, n0 = _slab_cycle(*args, False, monkeypatch)
                u1, c1, n1 = _slab_cycle(*args, True, monkeypatch)
                what = (pre, post, mu, window, zero_in)
                assert np.array_equal(u0, u1), what
                assert np.array_equal(c0, c1), what
                assert n1 == pytest.approx(n0, rel=1e-12), what


def test_bench_cycles_with_wide_tiles_against_the_oracle(pkg, po, monkeypatch):
    """the bench's workload (8192^2, levels 13..7, V(10,10)): levels 7..10 on k_tile_wide by default"""
    cfg = dict(finest_level=13, coarsest_level=7, mu1=10, mu2=10, schedule=0)
    n = (1 << 13) - 1
    b = po.rhs_sine(13)
    u0 = po.fill_uniform((n, n), 12345)
    for k in ("MGX_TILE_WIDE", "MGX_TILE_MAX_N", "MGX_TILE_SHORT_N", "MGX_TILE_K"):
        monkeypatch.delenv(k, raising=False)
    _, h, u = run_gpu(pkg, cfg, b, u0, tol=0.0, max_cycles=2)
    u_ref, h_ref = po.Solver(**cfg).solve(b, u0, tol=0.0, max_cycles=2)
    assert hist_close(h, h_ref), (h, h_ref)
    assert np.max(np.abs(u - u_ref)) <= 1e-12 * np.max(np.abs(u_ref))
    # k_tile_smooth on the same levels (the parent's path): the same bits
    monkeypatch.setenv("MGX_TILE_WIDE", "0")
    _, h0, u_narrow = run_gpu(pkg, cfg, b, u0, tol=0.0, max_cycles=2)
    assert np.array_equal(u, u_narrow)
    assert np.allclose(h, h0, rtol=1e-13, atol=0)
