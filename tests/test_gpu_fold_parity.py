"""The deep folded passes know the parity of every row step at compile time: a chunk whose cone starts on the
other parity marches from one row earlier (csrc/mgx_kernels.hpp, cycle_y0).  mgx_slab_cycle on row ranges whose
first row has each parity - with the slab's halo exactly the cone, and with odd chunk heights that mix both parities
in one launch - must give what the unfolded operators give, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import hipmem as hm      # device buffers on the HIP runtime libmgx is linked against (see hipmem.py)

pytestmark = pytest.mark.gpu


def grid_from_interior(pkg, a, level, dt):
    N = 1 << level
    pitch = pkg.lib().mgx_level_pitch(level, pkg.DTYPE_F64 if dt == np.float64 else pkg.DTYPE_F32)
    g = np.zeros((N + 1, pitch), dtype=dt)
    g[1:N, 1:N] = a
    return hm.from_numpy(g)


# geometry: "march" = the marching passes with the launcher's chunk heights; "odd_chunks" = one-round paired
# heights with an odd short chunk, so that the chunks of one launch start on rows of both parities
@pytest.mark.parametrize("geometry", ["march", "odd_chunks"])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_folded_slab_cycle_on_both_row_parities(pkg, po, dt, first, geometry, monkeypatch):
    for k in ("MGX_SLAB_TILE_POINTS", "MGX_PAIR_MIN_ROWS", "MGX_MIN_CHUNK", "MGX_FUSE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MGX_SLAB_TILE_POINTS", "0")
    if geometry == "odd_chunks":
        monkeypatch.setenv("MGX_PAIR_MIN_ROWS", "8")
        monkeypatch.setenv("MGX_MIN_CHUNK", "9")
    L = pkg.lib()
    mu = 10
    level = 11 if geometry == "odd_chunks" else 9
    N, NC = 1 << level, 1 << (level - 1)
    code = pkg.DTYPE_F64 if dt == np.float64 else pkg.DTYPE_F32
    rng = np.random.default_rng(31 + first)
    v = rng.uniform(-1, 1, (N - 1, N - 1)).astype(dt)
    f = rng.uniform(-1, 1, (N - 1, N - 1)).astype(dt)
    e = rng.uniform(-1, 1, (NC - 1, NC - 1)).astype(dt)
    own_lo, own_hi = N // 4 + first, N // 2 + first      # first row even (first = 0) or odd (first = 1)
    halo = mu + 1                                         # exactly the cone of the norm stage
    lo, hi = own_lo - halo, own_hi + halo
    clo, chi = lo // 2 - 1, hi // 2 + 2
    U, B = grid_from_interior(pkg, v, level, dt), grid_from_interior(pkg, f, level, dt)
    E = grid_from_interior(pkg, e, level - 1, dt)
    fs = pkg.Slab(level=level, dtype=code, rows=hi - lo, row0=lo)
    cs = pkg.Slab(level=level - 1, dtype=code, rows=chi - clo, row0=clo)
    scratch = hm.zeros(int(L.mgx_slab_scratch_doubles(C.byref(fs))), np.float64)

    def folded(pre, post):
        u, b, tmp = U[lo:hi].clone(), B[lo:hi].clone(), hm.zeros_like(U[lo:hi])
        ce = E[clo:chi].clone()
        out = hm.zeros(1, np.float64)
        flag = C.c_int()
        st = L.mgx_slab_cycle(C.byref(fs), u.data_ptr(), b.data_ptr(), tmp.data_ptr(), own_lo - lo, own_hi - lo, mu, 2.0 / 3.0,
                              pkg.SMOOTHER_JACOBI, C.byref(cs), ce.data_ptr() if pre else None, None, 0, 0, 0, 0,
                              scratch.data_ptr() if post == 2 else None, out.data_ptr() if post == 2 else None,
                              C.byref(flag), None)
        hm.synchronize()
        assert st == 0
        return (tmp if flag.value else u).cpu().numpy()[own_lo - lo:own_hi - lo, 1:N], float(out.item())

    def unfolded(pre):
        # the same rows through the separate operators: prolongation + add on the whole slab, then the slab smoother
        u, b, tmp = U[lo:hi].clone(), B[lo:hi].clone(), hm.zeros_like(U[lo:hi])
        if pre:
            assert L.mgx_slab_prolong(C.byref(fs), u.data_ptr(), C.byref(cs), E[clo:chi].clone().data_ptr(), 0, hi - lo, 1, None) == 0
        flag = C.c_int()
        assert L.mgx_slab_jacobi(C.byref(fs), u.data_ptr(), b.data_ptr(), tmp.data_ptr(), own_lo - lo, own_hi - lo, mu, 2.0 / 3.0, 1,
                                 C.byref(flag), None) == 0
        hm.synchronize()
        return (tmp if flag.value else u).cpu().numpy()[own_lo - lo:own_hi - lo, 1:N]

    ref_pre, ref_plain = unfolded(True), unfolded(False)
    assert np.array_equal(ref_pre, po.jacobi(po.prolong_add(v, e), f, mu)[own_lo - 1:own_hi - 1])
    got, _ = folded(True, 0)
    assert np.array_equal(got, ref_pre)
    got, sq = folded(True, 2)
    assert np.array_equal(got, ref_pre)
    r = po.residual(po.jacobi(po.prolong_add(v, e), f, mu), f)[own_lo - 1:own_hi - 1].astype(np.float64)
    assert abs(sq - float(np.sum(r * r))) <= 1e-12 * float(np.sum(r * r))
    got, _ = folded(False, 0)
    assert np.array_equal(got, ref_plain)
    got, _ = folded(False, 2)
    assert np.array_equal(got, ref_plain)
