"""GPU tests of nine-point finest operators on GALERKIN handles (mgx_set_stencil9, mgx_set_tensor; include/mgx.h)
against the numpy statement of tests/nine_ref.py, which tests/test_tensor_cpu.py pins against mathematics.

Bit for bit: the tensor discretisation, the hierarchy (both transfers, both restriction modes) from caller-given
nine-point operators - also with junk in the ring-pointing coefficients -, the Jacobi sweep, the residual, Chebyshev
blocks and the line factors on a nine-point finest level.  Line sweeps by the tolerance rule of tests/test_gpu_line.py,
solve histories to 1e-10 relative in double and 1e-6 in float (tests/test_gpu_galerkin.py), Krylov histories to
RTOL64 = 1e-9 / RTOL32 = 1e-3 (tests/test_gpu_pcg.py).

Shapes: a wave covers 62 output lanes, 124 columns in double and 248 in float.  (9, 5) and (8, 3): the first product has
more than one strip in double ((9, 5) in float too); (10, 4): a middle strip with neighbour strips on both sides in
float; (6, 2); (4, 4): no coarse level, the dense inverse of a nine-point finest operator.  Level 3 (n = 7): every point
touches the ring."""
import ctypes as C

import numpy as np
import pytest

import gcr_ref
import galerkin_ref as gr
import line_ref as lr
import nine_ref as nr
import pcg_ref
import wcycle_ref as wr
from test_gpu_galerkin import assert_hierarchy, assert_same, handle, np_dtype
from test_gpu_line import check_sweeps
from test_gpu_opdep import assert_weights
from test_gpu_pcg import RTOL32, RTOL64, assert_hist
from test_gpu_solve import hist_close

pytestmark = pytest.mark.gpu

BILINEAR, OPERATOR = 0, 1
INVALID, STATE = 1, 5                     # MGX_ERR_INVALID, MGX_ERR_STATE
PROF_SMOOTH_FINE = 0                      # MGX_PROF_SMOOTH_FINE

TENSORS = {
    "const": lambda L: nr.rotated_tensor(L, 30.0, 0.2),
    "rot45": lambda L: nr.rotated_tensor(L, 45.0, 0.5),
    "smooth": nr.smooth_tensor,
    "jump": nr.jump_tensor,
}


def ptrs(arrays):
    return [C.c_void_p(a.ctypes.data) for a in arrays]


def raw_set9(pkg, mg, level, st, count=None):
    return pkg.lib().mgx_set_stencil9(mg._h, level, *ptrs(st), st[0].size if count is None else count)


def rand(level, seed, dt):
    n = (1 << level) - 1
    return np.random.default_rng(seed).uniform(-1, 1, (n, n)).astype(dt)


_refs = {}


def reference(po, key, make):
    """one reference hierarchy per configuration for the whole module (its dense inverse is built once); mu1, mu2 and
    the cycle kind are attributes the callers set per use"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def tensor_ref(po, kind, L, Lc, dtype, transfer=BILINEAR, cls=None, **kw):
    cls = cls or (nr.OpdepHierarchy if transfer == OPERATOR else nr.Hierarchy)
    key = (kind, L, Lc, dtype, cls.__name__, tuple(sorted(kw.items())))
    ref = reference(po, key, lambda: cls(po, nr.tensor9(*TENSORS[kind](L), dtype=np_dtype(dtype)), L, Lc, np_dtype(dtype), **kw))
    ref.mu1, ref.mu2, ref.cycle = kw.get("mu1", 2), kw.get("mu2", 2), wr.V
    return ref


def tensor_handle(pkg, kind, L, Lc, transfer=BILINEAR, **kw):
    mg = handle(pkg, L, Lc, **kw)
    mg.set_tensor(*TENSORS[kind](L))
    mg.build_galerkin(transfer)
    return mg


# ---- 1. entry and state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_entry_points_and_the_state_model(pkg, po, dtype):
    dt = np_dtype(dtype)
    L, Lc = 4, 3
    n, N = (1 << L) - 1, 1 << L
    st = [x.astype(dt) for x in nr.random_stencil9(L, 1)]
    nodes = [np.ones((N + 1, N + 1)), np.full((N + 1, N + 1), 0.25), np.ones((N + 1, N + 1))]
    lib = pkg.lib()
    # handles whose op is not GALERKIN: MGX_ERR_STATE, the message names GALERKIN
    for op in (pkg.OPERATOR_STENCIL5, pkg.OPERATOR_POISSON):
        with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=op, dtype=dtype, schedule=0) as mg:
            assert raw_set9(pkg, mg, L, st) == STATE
            assert "GALERKIN" in lib.mgx_last_error(mg._h).decode()
            assert lib.mgx_set_tensor(mg._h, *ptrs(nodes), nodes[0].size) == STATE
            assert "GALERKIN" in lib.mgx_last_error(mg._h).decode()
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        c = [x.astype(dt) for x in nr.random_stencil9(Lc, 2)]
        assert raw_set9(pkg, mg, Lc, c) == STATE                         # a coarse level is not the caller's
        assert raw_set9(pkg, mg, L + 1, st) == INVALID                   # no such level
        assert raw_set9(pkg, mg, L, st, count=n * n - 1) == INVALID
        for k in range(9):
            p = ptrs(st)
            p[k] = C.c_void_p()
            assert lib.mgx_set_stencil9(mg._h, L, *p, st[0].size) == INVALID, k
        assert lib.mgx_set_tensor(mg._h, *ptrs(nodes), nodes[0].size - 1) == INVALID
        for k in range(3):
            p = ptrs(nodes)
            p[k] = C.c_void_p()
            assert lib.mgx_set_tensor(mg._h, *p, nodes[0].size) == INVALID, k
        # none of the refused calls gave the handle an operator
        with pytest.raises(pkg.MgxError, match="finest operator not set"):
            mg.build_galerkin()
        for setter in (lambda: mg.set_stencil9(L, *st), lambda: mg.set_tensor(*nodes)):
            setter()
            # between the set and the build: schedules and read-backs are MGX_ERR_STATE
            for call in (mg.vcycle, mg.vcycle_zero, lambda: mg.solve(1e-8, 3), lambda: mg.solve_pcg(1e-8, 3), lambda: mg.solve_gcr(1e-8, 3, 2),
                         lambda: mg.get_stencil9(L, 0), lambda: mg.smooth(L, 1)):
                with pytest.raises(pkg.MgxError, match="invalid state.*not built"):
                    call()
            mg.build_galerkin()
            with pytest.raises(pkg.MgxError, match="invalid state.*mgx_get_stencil9"):
                mg.get_stencil(L, 0)
            mg.set_rhs(rand(L, 3, dt))
            stt, h = mg.solve(tol=0.0, max_cycles=2)
            assert np.isfinite(h).all() and h[-1] < h[0]
        # back to five-point: mgx_get_stencil answers again, the corners read back as zeros
        mg.set_stencil(L, *st[:5])
        mg.build_galerkin()
        assert np.array_equal(mg.get_stencil(L, 0), st[0])
        for q in range(5, 9):
            assert not mg.get_stencil9(L, q).any() and not mg.get_stencil9(L, 9 + q).any()


@pytest.mark.parametrize("dtype", [1, 0])
def test_ring_pointing_values_read_back_as_given(pkg, po, dtype):
    """the rule mgx.h states: the finest operator is stored as the caller gave it, ring-pointing places included (as
    mgx_set_stencil does); R_omega there is computed from them; the coarse operators hold zeros there"""
    dt = np_dtype(dtype)
    L = 5
    st = [x.astype(dt) for x in nr.with_ring_values9(nr.random_stencil9(L, 5), 6)]
    ref = nr.Hierarchy(po, st, L, 3, dt)
    with handle(pkg, L, 3, dtype=dtype) as mg:
        mg.set_stencil9(L, *st)
        mg.build_galerkin()
        for q in range(9):
            assert_same(mg.get_stencil9(L, q), st[q], ("finest slot", gr.SLOTS[q]))
        assert abs(mg.get_stencil9(L, 5)[0, 0]) >= 1.0                  # junk, not a zero
        assert_hierarchy(mg, ref, range(L, 2, -1))
        for lv in (4, 3):
            got = [mg.get_stencil9(lv, q) for q in range(9)]
            for a, b in zip(got, nr.zero_ring(got)):
                assert np.array_equal(a, b)


# ---- 2. mgx_set_tensor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("kind", ["const", "smooth", "jump"])
@pytest.mark.parametrize("L", [3, 8])
def test_set_tensor_is_tensor9_bit_for_bit(pkg, po, L, kind, dtype):
    dt = np_dtype(dtype)
    want = nr.tensor9(*TENSORS[kind](L), dtype=dt)
    with handle(pkg, L, 3 if L > 3 else 2, dtype=dtype) as mg:
        mg.set_tensor(*TENSORS[kind](L))
        mg.build_galerkin()
        for q in range(9):
            assert_same(mg.get_stencil9(L, q), want[q], (kind, L, "slot", gr.SLOTS[q]))
    assert np.abs(want[5]).max() > 0.01


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
def test_isotropic_tensor_equals_set_coefficient_on_every_level(pkg, po, transfer, dtype):
    """axy = 0, axx = ayy = a: operators, splittings and bounds of every level, and ten cycles of mgx_solve, equal those
    of a handle given mgx_set_coefficient(a) - the nine-point path tied to the five-point path the oracle pins"""
    L, Lc = 7, 3
    x, y = nr.grid_nodes(L)
    a = 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    b = rand(L, 7, np_dtype(dtype))
    out = []
    for nine in (True, False):
        with handle(pkg, L, Lc, dtype=dtype) as mg:
            if nine:
                mg.set_tensor(a, np.zeros_like(a), a)
            else:
                mg.set_coefficient(a)
            mg.build_galerkin(transfer)
            ops = {(lv, q): mg.get_stencil9(lv, q) for lv in range(Lc, L + 1) for q in range(18)}
            lam = [mg.lambda_max(lv) for lv in range(Lc, L + 1)]
            mg.set_rhs(b)
            st, h = mg.solve(tol=0.0, max_cycles=10)
            out.append((ops, lam, h, mg.get_solution()))
    (ops9, lam9, h9, u9), (ops5, lam5, h5, u5) = out
    for key in ops5:
        assert_same(ops9[key], ops5[key], ("level", key[0], "array", key[1]))
    assert lam9 == lam5
    assert np.array_equal(h9, h5), (h9, h5)
    assert_same(u9, u5, "U after ten cycles")


# ---- 3. hierarchies from caller-given nine-point operators -----------------------------------------------------------
SHAPES = [(9, 5), (8, 3), (10, 4), (6, 2), (4, 4)]
HIER = [(f, c, transfer, mode, dtype) for f, c in SHAPES for transfer in (BILINEAR, OPERATOR) for mode in (gr.CONSISTENT, gr.FW16)
        for dtype in (1, 0)]


@pytest.mark.parametrize("finest,coarsest,transfer,mode,dtype", HIER, ids=["-".join(map(str, c)) for c in HIER])
def test_hierarchy_from_a_nine_point_operator_is_bit_identical(pkg, po, finest, coarsest, transfer, mode, dtype):
    dt = np_dtype(dtype)
    omega = 0.8
    base = nr.random_stencil9(finest, 100 + finest)
    junk = [x.astype(dt) for x in nr.with_ring_values9(base, 200 + finest)]
    zeroed = [x.astype(dt) for x in nr.zero_ring(base)]
    cls = nr.OpdepHierarchy if transfer == OPERATOR else nr.Hierarchy
    ref = cls(po, junk, finest, coarsest, dt, mode, omega)
    assert np.max(np.abs(zeroed[4][:, :-1] - zeroed[3][:, 1:])) > 0.1 and np.max(np.abs(zeroed[8][:-1, :-1] - zeroed[5][1:, 1:])) > 0.1    # not symmetric
    seen = []
    f = rand(coarsest, 9, dt)
    for st in (junk, zeroed):
        with handle(pkg, finest, coarsest, dtype=dtype, restrict_mode=mode, omega=omega) as mg:
            mg.set_stencil9(finest, *st)
            mg.build_galerkin(transfer)
            if st is junk:
                assert_hierarchy(mg, ref, range(finest, coarsest - 1, -1))
                if transfer == OPERATOR:
                    assert_weights(mg, ref)
            below = {(lv, q): mg.get_stencil9(lv, q) for lv in range(coarsest, finest) for q in range(18)}
            wts = {(lv, k): mg.get_prolongation(lv, k) for lv in range(finest, coarsest, -1) for k in range(8)} if transfer == OPERATOR else {}
            seen.append((below, wts, [mg.lambda_max(lv) for lv in range(coarsest, finest + 1)], mg.bottom_solve(f)))
    (b0, w0, l0, x0), (b1, w1, l1, x1) = seen
    for key in b0:
        assert_same(b0[key], b1[key], ("junk against zeros: level", key[0], "array", key[1]))
    for key in w0:
        assert_same(w0[key], w1[key], ("junk against zeros: level", key[0], "weight", key[1]))
    assert l0 == l1
    assert_same(x0, x1, "bottom solve, junk against zeros")
    if coarsest <= 4:
        x_ref = ref.bottom(f)                                          # (4, 4): the dense inverse of the nine-point FINEST operator
        if dtype == 1:
            assert np.max(np.abs(x0 - x_ref)) <= 1e-10 * np.max(np.abs(x_ref))
        else:
            assert np.allclose(x0, x_ref, rtol=1e-6, atol=1e-6 * np.max(np.abs(x_ref)))


# ---- 4. operators on a nine-point finest level -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("L", [9, 3])
def test_sweep_residual_and_norm_on_the_finest_level(pkg, po, L, dtype):
    dt = np_dtype(dtype)
    omega = 2.0 / 3.0
    Lc = 5 if L == 9 else 2
    st = [x.astype(dt) for x in nr.with_ring_values9(nr.random_stencil9(L, 11), 12)]
    jac = gr.build_jacobi9(st, omega)
    u, b = rand(L, 1, dt), rand(L, 2, dt)
    with handle(pkg, L, Lc, dtype=dtype, omega=omega) as mg:
        mg.set_stencil9(L, *st)
        mg.build_galerkin()
        for mu in (1, 2, 5):
            assert_same(mg.jacobirelaxation(L, u, b, mu), gr.jacobi9(u, b, mu, omega, jac), ("level", L, "mu", mu))
        want = gr.residual9(u, b, st)
        assert_same(mg.residual(L, u, b), want, ("level", L, "residual"))
        rn = mg.residual_norm(L)
        assert abs(rn - po.norm2(want)) <= 1e-12 * rn
        assert mg.lambda_max(L) == nr.cr.lambda_bound(st, nine=True)
        ms = mg.time_smoother(4)
        assert ms > 0.0


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
def test_chebyshev_blocks_on_the_finest_level(pkg, po, transfer, dtype):
    dt = np_dtype(dtype)
    for L, Lc in ((8, 4), (3, 2)):
        cls = nr.ChebyOpdepHierarchy if transfer == OPERATOR else nr.ChebyHierarchy
        ref = cls(po, nr.tensor9(*nr.smooth_tensor(L), dtype=dt), L, Lc, dt)
        u, b = rand(L, 3, dt), rand(L, 4, dt)
        with handle(pkg, L, Lc, dtype=dtype, smoother=pkg.SMOOTHER_CHEBYSHEV) as mg:
            mg.set_tensor(*nr.smooth_tensor(L))
            mg.build_galerkin(transfer)
            for lv in range(Lc, L + 1):
                assert mg.lambda_max(lv) == ref.g[lv], lv
            for k in (1, 2, 3, 4):
                assert_same(mg.jacobirelaxation(L, u, b, k), ref.smooth(L, u, b, k), ("level", L, "degree", k))


@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
@pytest.mark.parametrize("smoother", [lr.LINE_X, lr.LINE_Y, lr.LINE_ALT], ids=["x", "y", "alt"])
def test_line_factors_and_sweeps_on_the_finest_level(pkg, po, smoother, dtype):
    """factors bit for bit; sweeps to the bound of tests/test_gpu_line.py (4 x line_ref's own distance to long double, floor
    16 eps; check_sweeps prints the ratios).  Level 8: rows cross a k_line_x tile in double, columns are cut into the
    launcher's chunks; level 3: every coefficient that is guarded is guarded on some point"""
    dt = np_dtype(dtype)
    for L, Lc in ((8, 4), (3, 2)):
        st = nr.tensor9(*nr.rotated_tensor(L, 45.0, 0.1), dtype=dt)
        with handle(pkg, L, Lc, dtype=dtype, smoother=smoother, mu1=1, mu2=1) as mg:
            mg.set_tensor(*nr.rotated_tensor(L, 45.0, 0.1))
            mg.build_galerkin()
            for d, name in ((0, "x"), (1, "y")):
                if name in lr.DIRS[smoother]:
                    m, g, ok = lr.factor_dir(st, name)
                    assert ok
                    assert_same(mg.line_factor(L, d, 0), m, (L, name, "m"))
                    assert_same(mg.line_factor(L, d, 1), g, (L, name, "g"))
            check_sweeps(mg, L, st, True, smoother, dt, "nine-point finest")


# ---- 5. solves ---------------------------------------------------------------------------------------------------------
def assert_solve(dtype, h, h_ref, u, u_ref, what):
    m = min(len(h), len(h_ref))
    print(f"{what}: {len(h) - 1} cycles (reference {len(h_ref) - 1}), max rel. history difference {np.max(np.abs(h[:m] - h_ref[:m]) / h_ref[:m]):.3e}")
    assert len(h) == len(h_ref), (what, h, h_ref)
    if dtype == 1:
        assert hist_close(h, h_ref), (what, h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref)), what
    else:
        assert np.allclose(h, h_ref, rtol=1e-6, atol=0), (what, h, h_ref)


def tolerance(dtype):
    return (1e-8, 40) if dtype == 1 else (1e-4, 40)         # float cannot reach 1e-8; 1e-4 is above its rounding floor


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("L,Lc", [(7, 3), (8, 4)])
@pytest.mark.parametrize("kind", ["rot45", "smooth"])
def test_v22_solves_take_the_reference_s_cycles(pkg, po, kind, L, Lc, dtype):
    dt = np_dtype(dtype)
    tol, cap = tolerance(dtype)
    b = np.random.default_rng(3).uniform(-1, 1, ((1 << L) - 1,) * 2).astype(dt)
    ref = tensor_ref(po, kind, L, Lc, dtype)
    u_ref, h_ref = ref.solve(b, tol=tol, max_cycles=cap)
    assert h_ref[-1] <= tol * h_ref[0], "the reference itself did not converge"
    with tensor_handle(pkg, kind, L, Lc, dtype=dtype) as mg:
        mg.set_rhs(b)
        st, h = mg.solve(tol=tol, max_cycles=cap)
        assert st.converged and mg.graphs_cached() >= 1
        assert_solve(dtype, h, h_ref, mg.get_solution(), u_ref, (kind, L, Lc, dtype))


VARIANTS = {
    "fmg": dict(schedule=gr.FMG),
    "bottom_smooth": dict(bottom=gr.SMOOTH),
    "opdep": dict(transfer=OPERATOR),
    "opdep_fmg_fw16": dict(transfer=OPERATOR, schedule=gr.FMG, mode=gr.FW16),
    "profile1": dict(profile=1),
    "profile2": dict(profile=2),
}


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_other_schedules_and_paths(pkg, po, name, dtype):
    v = dict(VARIANTS[name])
    dt = np_dtype(dtype)
    L, Lc = 7, 3
    tol, cap = tolerance(dtype)
    transfer, schedule, profile = v.pop("transfer", BILINEAR), v.pop("schedule", gr.V), v.pop("profile", 0)
    b = rand(L, 3, dt)
    ref = tensor_ref(po, "smooth", L, Lc, dtype, transfer, **v)
    u_ref, h_ref = ref.solve(b, tol=tol, max_cycles=cap, schedule=schedule)
    dev = dict(dtype=dtype, schedule=schedule, profile=profile, mu0=0)
    if "mode" in v:
        dev["restrict_mode"] = v["mode"]
    if "bottom" in v:
        dev["bottom"] = v["bottom"]
    with tensor_handle(pkg, "smooth", L, Lc, transfer, **dev) as mg:
        mg.set_rhs(b)
        st, h = mg.solve(tol=tol, max_cycles=cap)
        assert_solve(dtype, h, h_ref, mg.get_solution(), u_ref, (name, dtype))
        if profile:
            p = mg.profile()
            assert p["launches"][PROF_SMOOTH_FINE] > 0 and p["ms"][PROF_SMOOTH_FINE] > 0.0


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
@pytest.mark.parametrize("cycle", [wr.W, wr.F], ids=["W", "F"])
def test_w_and_f_cycles_keep_the_finest_level_s_launches(pkg, po, monkeypatch, cycle, transfer, dtype):
    """levels 6..3: the finest level has N = 64 and is nine-point - it must not become a one-workgroup visit (levels 5 and
    4 do): MGX_SMALL_VISIT=0 and the default give the same bits, and both follow the reference"""
    dt = np_dtype(dtype)
    L, Lc = 6, 3
    tol, cap = tolerance(dtype)
    b = rand(L, 3, dt)
    ref = tensor_ref(po, "smooth", L, Lc, dtype, transfer)
    ref.cycle = cycle
    u_ref, h_ref = ref.solve(b, tol=tol, max_cycles=cap)
    runs = {}
    for small in ("1", "0"):
        monkeypatch.setenv("MGX_SMALL_VISIT", small)
        with tensor_handle(pkg, "smooth", L, Lc, transfer, dtype=dtype) as mg:
            mg.set_cycle(cycle)
            mg.set_rhs(b)
            u0 = rand(L, 4, dt)
            mg.set_guess(u0)
            mg.vcycle()
            one = mg.get_solution()
            mg.set_guess(np.zeros_like(b))
            st, h = mg.solve(tol=tol, max_cycles=cap)
            runs[small] = (one, h, mg.get_solution())
    assert_same(runs["1"][0], runs["0"][0], "U after one cycle")
    assert np.array_equal(runs["1"][1], runs["0"][1])
    assert_same(runs["1"][2], runs["0"][2], "U after the solve")
    assert_solve(dtype, runs["1"][1], h_ref, runs["1"][2], u_ref, (wr.NAMES[cycle], transfer, dtype))


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_vcycle_zero_equals_zero_guess_then_vcycle(pkg, po, monkeypatch, graph, dtype):
    monkeypatch.setenv("MGX_GRAPH", graph)
    dt = np_dtype(dtype)
    L, Lc = 7, 3
    b = rand(L, 5, dt)
    ref = tensor_ref(po, "rot45", L, Lc, dtype)
    want = ref.vcycle(L, np.zeros_like(b), b)
    with tensor_handle(pkg, "rot45", L, Lc, dtype=dtype) as mg:
        mg.set_rhs(b)
        mg.set_guess(rand(L, 6, dt))                      # must not matter
        mg.vcycle_zero()
        a = mg.get_solution()
        mg.vcycle_zero()                                  # again: the replayed graph
        a2 = mg.get_solution()
        mg.set_guess(np.zeros_like(b))
        mg.vcycle()
        c = mg.get_solution()
    assert_same(a, c, "vcycle_zero against zero guess + vcycle")
    assert_same(a2, a, "second vcycle_zero")
    scale = np.max(np.abs(want))
    assert np.max(np.abs(a - want)) <= (1e-10 if dtype == 1 else 1e-5) * scale


# ---- 6. Krylov ---------------------------------------------------------------------------------------------------------
def krylov_ref(po, method, st, ref, b, x0, tol, cap, restart=None):
    A = nr.Operator9(st, ref.dt)
    M = gcr_ref.cycle_preconditioner(ref)
    if method == "pcg":
        return pcg_ref.pcg(A, M, b, x0, tol=tol, max_iters=cap)
    return gcr_ref.gcr(A, M, b, x0, tol=tol, max_iters=cap, restart=restart)


def run_krylov(pkg, mg, L, method, b, x0, tol, cap, restart=None):
    mg.set_rhs(b)
    mg.set_guess(x0)
    st, h = mg.solve_pcg(tol=tol, max_iters=cap) if method == "pcg" else mg.solve_gcr(tol=tol, max_iters=cap, restart=restart)
    return st, h, mg.get_solution(), mg.get_level(L, pkg.VEC_B)


KRYLOV = [("pcg", None), ("gcr", 1), ("gcr", 3), ("gcr", 8)]


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("method,restart", KRYLOV, ids=[m + (str(r) if r else "") for m, r in KRYLOV])
@pytest.mark.parametrize("L,Lc", [(8, 4), (3, 2)])
def test_krylov_histories_on_the_tensor_operator(pkg, po, monkeypatch, L, Lc, method, restart, dtype):
    """the symmetric tensor operator (theta = 45, eps = 0.1), V(2,2) Jacobi cycle; B restored, two runs and MGX_GRAPH=0
    give the same bits.  Level 8 in double is the smallest finest level whose Krylov launch (make_launch(N, W, N - 1, 0)
    as krylov_direction is called: strips = ceil(N / W / 62), chunks = ceil((N - 1) / R), R = 4) has three strips (128
    vectors of two doubles: 62 + 62 + 4) and 64 row chunks: the corner neighbours cross strip seams and chunk seams"""
    dt = np_dtype(dtype)
    tol, cap = (1e-8, 30) if dtype == 1 else (1e-4, 30)
    nodes = nr.rotated_tensor(L, 45.0, 0.1)
    st = nr.tensor9(*nodes, dtype=dt)
    ref = reference(po, ("kry", L, Lc, dtype), lambda: nr.Hierarchy(po, st, L, Lc, dt))
    b, x0 = rand(L, 21, dt), rand(L, 22, dt)
    x_ref, h_ref, conv, brk = krylov_ref(po, method, st, ref, b, x0, tol, cap, restart)
    assert conv and not brk
    runs = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("MGX_GRAPH", graph)
        with handle(pkg, L, Lc, dtype=dtype) as mg:
            mg.set_tensor(*nodes)
            mg.build_galerkin()
            for _ in range(2 if len(runs) == 0 else 1):          # the first handle runs twice
                stt, h, x, b_after = run_krylov(pkg, mg, L, method, b, x0, tol, cap, restart)
                assert_same(b_after, b, "B after the solve")
                runs.append((h, x))
            if len(runs) == 2 and method == "gcr":
                assert mg.time_gcr_pass(3, 0, repeats=2) > 0.0     # MGX_GCR_PASS_DIRECTION on a nine-point finest level
    print(f"{method}{restart or ''} level {L} dtype {dtype}: {len(runs[0][0]) - 1} iterations (reference {len(h_ref) - 1})")
    assert stt.converged
    assert_hist(runs[0][0], h_ref, RTOL64 if dtype == 1 else RTOL32)
    for h, x in runs[1:]:
        assert np.array_equal(h, runs[0][0])
        assert_same(x, runs[0][1], "the iterate of a repeated / eager run")
    assert np.max(np.abs(runs[0][1] - x_ref)) <= (1e-8 if dtype == 1 else 1e-3) * np.max(np.abs(x_ref))


def test_krylov_seams_in_float(pkg, po):
    """float: three strips need N / 4 > 124, level 9 (128 vectors of four floats: 62 + 62 + 4; 128 row chunks)"""
    L, Lc, dt = 9, 4, np.float32
    nodes = nr.smooth_tensor(L)
    st = nr.tensor9(*nodes, dtype=dt)
    ref = nr.Hierarchy(po, st, L, Lc, dt)
    b, x0 = rand(L, 31, dt), np.zeros(((1 << L) - 1,) * 2, dt)
    x_ref, h_ref, conv, brk = krylov_ref(po, "gcr", st, ref, b, x0, 1e-4, 20, 3)
    assert conv and not brk
    with handle(pkg, L, Lc, dtype=0) as mg:
        mg.set_tensor(*nodes)
        mg.build_galerkin()
        stt, h, x, b_after = run_krylov(pkg, mg, L, "gcr", b, x0, 1e-4, 20, 3)
    assert_same(b_after, b, "B after the solve")
    assert_hist(h, h_ref, RTOL32)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("restart", [1, 3, 8])
def test_gcr_on_a_non_symmetric_nine_point_operator(pkg, po, restart, dtype):
    dt = np_dtype(dtype)
    L, Lc = 7, 3
    tol, cap = (1e-8, 30) if dtype == 1 else (1e-4, 30)
    st = [x.astype(dt) for x in nr.with_ring_values9(nr.random_stencil9(L, 41), 42)]
    ref = reference(po, ("nonsym", L, Lc, dtype), lambda: nr.Hierarchy(po, st, L, Lc, dt))
    b, x0 = rand(L, 43, dt), rand(L, 44, dt)
    x_ref, h_ref, conv, brk = krylov_ref(po, "gcr", st, ref, b, x0, tol, cap, restart)
    assert conv and not brk
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        mg.set_stencil9(L, *st)
        mg.build_galerkin()
        stt, h, x, b_after = run_krylov(pkg, mg, L, "gcr", b, x0, tol, cap, restart)
    assert_same(b_after, b, "B after the solve")
    assert stt.converged
    assert_hist(h, h_ref, RTOL64 if dtype == 1 else RTOL32)


# ---- 7. back and forth on one handle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
def test_tensor_coefficient_tensor_on_one_handle_equals_fresh_handles(pkg, po, transfer, dtype):
    dt = np_dtype(dtype)
    L, Lc = 7, 3
    x, y = nr.grid_nodes(L)
    a = 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    b = rand(L, 51, dt)
    legs = ["tensor", "coefficient", "tensor"]

    def leg(mg, what):
        if what == "tensor":
            mg.set_tensor(*nr.smooth_tensor(L))
        else:
            mg.set_coefficient(a)
        assert mg.graphs_cached() == 0                       # the setter dropped the graphs
        mg.build_galerkin(transfer)
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st, h = mg.solve(tol=0.0, max_cycles=6)
        assert mg.graphs_cached() >= 1                       # ... and the solve captured anew
        ops = [mg.get_stencil9(lv, q) for lv in range(Lc, L + 1) for q in range(18)]
        return h, mg.get_solution(), ops

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        long_lived = [leg(mg, w) for w in legs]
        with pytest.raises(pkg.MgxError, match="mgx_get_stencil9"):
            mg.get_stencil(L, 0)
    fresh = {}
    for w in set(legs):
        with handle(pkg, L, Lc, dtype=dtype) as mg:
            fresh[w] = leg(mg, w)
            if w == "coefficient":
                assert np.array_equal(mg.get_stencil(L, 0), fresh[w][2][(L - Lc) * 18])
    for w, (h, u, ops) in zip(legs, long_lived):
        hf, uf, of = fresh[w]
        assert np.array_equal(h, hf), (w, h, hf)
        assert_same(u, uf, (w, "U"))
        for k, (p, q) in enumerate(zip(ops, of)):
            assert_same(p, q, (w, "level", Lc + k // 18, "array", k % 18))
    assert not np.array_equal(fresh["tensor"][0], fresh["coefficient"][0])
