"""GPU tests of the zebra line smoothers (cfg.smoother = MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT, csrc/mgx_line.hpp)
against the numpy statement of tests/line_ref.py (whose properties tests/test_line_cpu.py checks).

The factors are compared bit for bit.  Sweeps and histories follow THE TOLERANCE RULE of tests/test_line_cpu.py: the
device joins the segments of a line in another order than the sequential recurrence, so the bound of a case is 4 x the
largest difference, relative to max |x|, between line_ref in the working type and line_ref in np.longdouble, with a
floor of 16 eps (histories: relative to the largest entry, floor 1e-12).  It is never taken from the device's output; the device is held to it against both
the working-type and the long-double statement.

Shapes: levels 5 and 6 (lines of 31 and 63 points in one tile and one chunk); N = 64 with MGX_LINE_CHUNK = 8 and 16
(k_line_y's carries through LDS: 8 and 4 chunks, the last one short); level 7 (the launcher's own chunking: 64 + 63
rows); k_line_x marches in tiles of 64 lanes x 16 bytes = 128 doubles or 256 floats, so a row crosses a tile boundary
from level 8 in double and from level 9 in float: levels 9, 8, 7 of a (9, 5) double hierarchy and 10, 9 of a (10, 5)
float hierarchy; every line has 2^L - 1 points, no multiple of a tile or a chunk."""
import functools

import numpy as np
import pytest

import galerkin_ref as gr
import line_ref as lr
import pcg_ref
import wcycle_ref as wr
from test_galerkin_cpu import with_ring_values
from test_gpu_galerkin import np_dtype
from test_line_cpu import CAP, SEED_STABLE, TABLE_STABLE, TOL, as_type, operator5, rule_bound

pytestmark = pytest.mark.gpu

SMOOTHERS = (lr.LINE_X, lr.LINE_Y, lr.LINE_ALT)
NAMES = {lr.LINE_X: "x", lr.LINE_Y: "y", lr.LINE_ALT: "alt"}
KINDS = ("x1e-3", "layers", "contrast")


def handle(pkg, finest, coarsest, smoother, **kw):
    cfg = dict(finest_level=finest, coarsest_level=coarsest, op=pkg.OP_GALERKIN, smoother=smoother, mu1=1, mu2=1, schedule=0)
    cfg.update(kw)
    return pkg.Multigrid(**cfg)


@functools.lru_cache(maxsize=None)
def galerkin_ops(kind, finest, coarsest, dtype):
    """the operators of a GALERKIN hierarchy whose finest level carries `kind`, in the working type (bit for bit the
    device's: tests/test_gpu_galerkin.py)"""
    from oracle import pyoracle as po
    st = {finest: gr.nine(operator5(po, finest, kind, np_dtype(dtype)))}
    for lv in range(finest, coarsest, -1):
        st[lv - 1] = gr.rap(st[lv], 1 << lv)
    return st


def check_sweeps(mg, lv, st9, nine, smoother, dt, what, mus=(1, 3)):
    """mu sweeps on a level from a random v and b against line_ref, by the tolerance rule"""
    n = (1 << lv) - 1
    rng = np.random.default_rng(1000 + lv)
    v, b = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
    ref = lr.LevelSmoother(st9, nine, smoother)
    exact = lr.LevelSmoother(as_type(st9, np.longdouble), nine, smoother)
    for mu in mus:
        want, far = ref.sweep(v, b, mu), exact.sweep(v.astype(np.longdouble), b.astype(np.longdouble), mu)
        bound, err = rule_bound(want, far)
        got = mg.jacobirelaxation(lv, v, b, mu)
        assert got.dtype == dt and np.isfinite(got).all(), (what, mu)
        scale = float(np.max(np.abs(far)))
        d_t = float(np.max(np.abs(got.astype(np.longdouble) - want.astype(np.longdouble)))) / scale
        d_x = float(np.max(np.abs(got.astype(np.longdouble) - far))) / scale
        eps = float(np.finfo(dt).eps)
        msg = (f"{what} level {lv} {NAMES[smoother]} mu {mu}: device - line_ref {d_t / eps:.1f} eps, device - long double {d_x / eps:.1f} eps, "
               f"line_ref - long double {err / eps:.1f} eps, bound {bound / eps:.1f} eps; ratio to the bound {max(d_t, d_x) / bound:.2f}")
        print(msg)
        assert max(d_t, d_x) <= bound, msg


# ---- 1. factors, bit for bit -----------------------------------------------------------------------------------------
def assert_factors(mg, lv, st9, what):
    for d, name in ((0, "x"), (1, "y")):
        m, g, ok = lr.factor_dir(st9, name)
        assert ok
        assert np.array_equal(mg.line_factor(lv, d, 0), m), (what, lv, name, "m")
        assert np.array_equal(mg.line_factor(lv, d, 1), g), (what, lv, name, "g")


@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_factors_are_bit_identical_to_the_reference(pkg, po, kind, dtype):
    """five-point: STENCIL5 levels 5 and 6 and the finest GALERKIN level 6; nine-point: the built levels 5 (of a
    hierarchy 6..4) and 6 (of 7..5)"""
    dt = np_dtype(dtype)
    with pkg.Multigrid(finest_level=6, coarsest_level=5, op=pkg.OPERATOR_STENCIL5, smoother=lr.LINE_ALT, dtype=dtype) as mg:
        for lv in (5, 6):
            st5 = operator5(po, lv, kind, dt)
            mg.set_stencil(lv, *st5)
            assert_factors(mg, lv, gr.nine(st5), "STENCIL5")
    for finest, coarsest, levels in ((6, 4, (6, 5)), (7, 5, (6,))):
        st = galerkin_ops(kind, finest, coarsest, dtype)
        with handle(pkg, finest, coarsest, lr.LINE_ALT, dtype=dtype) as mg:
            mg.set_stencil(finest, *st[finest][:5])
            mg.build_galerkin()
            for lv in levels:
                assert_factors(mg, lv, st[lv], ("GALERKIN", finest))


# ---- 2. one sweep and mgx_smooth(level, 3) ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
@pytest.mark.parametrize("smoother", SMOOTHERS, ids=[NAMES[s] for s in SMOOTHERS])
@pytest.mark.parametrize("kind", KINDS)
def test_sweeps_follow_the_reference(pkg, po, kind, smoother, dtype):
    dt = np_dtype(dtype)
    with pkg.Multigrid(finest_level=6, coarsest_level=5, op=pkg.OPERATOR_STENCIL5, smoother=smoother, dtype=dtype) as mg:
        for lv in (5, 6):
            st5 = operator5(po, lv, kind, dt)
            mg.set_stencil(lv, *st5)
        for lv in (5, 6):
            check_sweeps(mg, lv, gr.nine(operator5(po, lv, kind, dt)), False, smoother, dt, ("STENCIL5", kind))
    for finest, coarsest, levels in ((6, 4, (6, 5)), (7, 5, (6,))):
        st = galerkin_ops(kind, finest, coarsest, dtype)
        with handle(pkg, finest, coarsest, smoother, dtype=dtype) as mg:
            mg.set_stencil(finest, *st[finest][:5])
            mg.build_galerkin()
            for lv in levels:
                check_sweeps(mg, lv, st[lv], lv != finest, smoother, dt, ("GALERKIN", finest, kind))


def test_coefficients_that_point_at_the_ring_are_never_read(pkg, po):
    """values up to 1e30 of mixed sign there change no bit of the factors or of a sweep"""
    L = 6
    st5 = operator5(po, L, "contrast")
    junk = with_ring_values(st5, 5)
    n = (1 << L) - 1
    rng = np.random.default_rng(6)
    v, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    out = []
    for op in (st5, junk):
        with pkg.Multigrid(finest_level=L, coarsest_level=5, op=pkg.OPERATOR_STENCIL5, smoother=lr.LINE_ALT) as mg:
            mg.set_stencil(5, *operator5(po, 5, "contrast"))
            mg.set_stencil(L, *op)
            out.append([mg.line_factor(L, d, w) for d in (0, 1) for w in (0, 1)] + [mg.jacobirelaxation(L, v, b, 2)])
    for a, c in zip(*out):
        assert np.array_equal(a, c)


# ---- 3. every carry path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
@pytest.mark.parametrize("chunk", ["8", "16"])
@pytest.mark.parametrize("smoother", [lr.LINE_Y, lr.LINE_ALT], ids=["y", "alt"])
def test_chunked_columns_at_n_64(pkg, po, monkeypatch, smoother, chunk, dtype):
    """MGX_LINE_CHUNK (read at mgx_create): 63 rows in chunks of 8 (7 full, one of 7) and 16 (3 full, one of 15); the
    five-point level 6 and the nine-point level 6 of a (7, 5) hierarchy"""
    dt = np_dtype(dtype)
    monkeypatch.setenv("MGX_LINE_CHUNK", chunk)
    for kind in ("layers", "contrast"):
        st = galerkin_ops(kind, 7, 5, dtype)
        with handle(pkg, 7, 5, smoother, dtype=dtype) as mg:
            mg.set_stencil(7, *st[7][:5])
            mg.build_galerkin()
            # the override took effect on this handle (and is floored at 16 chunks: level 9 has 511 rows)
            assert mg.line_chunks(6) == (int(chunk), -(-63 // int(chunk))) and mg.line_chunks(7) == (int(chunk), -(-127 // int(chunk)))
            assert_factors_dir_y(mg, 6, st[6])
            check_sweeps(mg, 6, st[6], True, smoother, dt, ("chunk", chunk, kind))
        st5 = operator5(po, 6, kind, dt)
        with pkg.Multigrid(finest_level=6, coarsest_level=5, op=pkg.OPERATOR_STENCIL5, smoother=smoother, dtype=dtype) as mg:
            mg.set_stencil(5, *operator5(po, 5, kind, dt))
            mg.set_stencil(6, *st5)
            check_sweeps(mg, 6, gr.nine(st5), False, smoother, dt, ("chunk", chunk, kind, "five-point"))


def assert_factors_dir_y(mg, lv, st9):
    m, g, ok = lr.factor_dir(st9, "y")
    assert ok and np.array_equal(mg.line_factor(lv, 1, 0), m) and np.array_equal(mg.line_factor(lv, 1, 1), g)


@pytest.mark.parametrize("dtype,finest,levels", [(1, 9, (9, 8, 7)), (0, 10, (10, 9))], ids=["f64", "f32"])
@pytest.mark.parametrize("smoother", SMOOTHERS, ids=[NAMES[s] for s in SMOOTHERS])
def test_rows_longer_than_a_tile_and_columns_in_the_launcher_s_chunks(pkg, po, smoother, dtype, finest, levels):
    """the smallest levels at which k_line_x crosses a tile boundary (8 in double, 9 in float: nine-point there, five-point
    one level up) and k_line_y takes more than one chunk on its own (7: 64 + 63 rows)"""
    dt = np_dtype(dtype)
    st = galerkin_ops("layers", finest, 5, dtype)
    with handle(pkg, finest, 5, smoother, dtype=dtype) as mg:
        mg.set_stencil(finest, *st[finest][:5])
        mg.build_galerkin()
        if smoother != lr.LINE_X:
            # the launcher's own chunks: 64 rows, at most 16 chunks; one chunk up to N = 64
            assert [mg.line_chunks(lv) for lv in (6, 7, 9)] == [(64, 1), (64, 2), (64, 8)]
            assert mg.line_chunks(finest) == ((64, 8) if finest == 9 else (64, 16))
        for lv in levels:
            check_sweeps(mg, lv, st[lv], lv != finest, smoother, dt, ("tiles", finest), mus=(1,))


# ---- 4, 5. solves ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_solve(cls, kind, smoother, finest, coarsest, dtype, tol, cap, schedule=gr.V, **kw):
    """(history in the working type, history in long double) of one reference solve; stencil5: every level carries the
    constant stencil of `kind`"""
    from oracle import pyoracle as po
    n = (1 << finest) - 1
    b = np.random.default_rng(SEED_STABLE).uniform(-1, 1, (n, n))
    out = []
    for ops, dt in ((po, np_dtype(dtype)), (lr.NumpyOps, np.longdouble)):
        if cls is lr.Stencil5:
            op = {lv: as_type(operator5(po, lv, kind, np_dtype(dtype)), dt) for lv in range(coarsest, finest + 1)}
        else:
            op = as_type(operator5(po, finest, kind, np_dtype(dtype)), dt)
        h = cls(smoother, ops, op, finest, coarsest, dt, mu1=1, mu2=1, **kw)
        out.append(np.asarray(h.solve(b.astype(np_dtype(dtype)), tol=tol, max_cycles=cap, schedule=schedule)[1], dtype=np.float64))
    return b, out[0], out[1]


def history_bound(h_t, h_x):
    """the tolerance rule on a history: the largest difference between the reference's histories in the working type and
    in long double, relative to the largest entry (as a sweep's is to max |x|), times 4, floor 1e-12"""
    m = min(len(h_t), len(h_x))
    return max(4.0 * float(np.max(np.abs(h_t[:m] - h_x[:m])) / np.max(h_x)), 1e-12)


def assert_history(h, h_t, h_x, what):
    assert len(h) == len(h_t), (what, len(h) - 1, len(h_t) - 1, h, h_t)
    bound = history_bound(h_t, h_x)
    d = float(np.max(np.abs(h - h_t)) / np.max(h_t))
    # (entry by entry the last residuals of a converged solve are rounding noise of b - A u: printed, not asserted)
    msg = (f"{what}: {len(h) - 1} cycles, largest history difference {d:.3e} of the largest entry, bound {bound:.3e}, ratio {d / bound:.2f}; "
           f"entry by entry {float(np.max(np.abs(h - h_t) / h_t)):.3e}")
    print(msg)
    assert d <= bound, msg


def device_solve(pkg, kind, smoother, finest, coarsest, dtype, b, tol, cap, op="galerkin", transfer=None, cycle=None, **kw):
    from oracle import pyoracle as po
    dt = np_dtype(dtype)
    if op == "stencil5":
        kw["op"] = pkg.OPERATOR_STENCIL5
    with handle(pkg, finest, coarsest, smoother, dtype=dtype, **kw) as mg:
        if op == "stencil5":
            for lv in range(coarsest, finest + 1):
                mg.set_stencil(lv, *operator5(po, lv, kind, dt))
        else:
            mg.set_stencil(finest, *operator5(po, finest, kind, dt))
            mg.build_galerkin(transfer)
        if cycle is not None:
            mg.set_cycle(cycle)
        mg.set_rhs(b.astype(dt))
        st, h = mg.solve(tol=tol, max_cycles=cap)
        return st, h, mg.get_solution()


@pytest.mark.parametrize("smoother", SMOOTHERS, ids=[NAMES[s] for s in SMOOTHERS])
@pytest.mark.parametrize("kind", ["iso", "x1e-2", "y1e-2", "x1e-3", "layers"])
def test_solves_take_the_reference_s_cycles(pkg, po, kind, smoother):
    """GALERKIN 6..3, V(1,1), double, to 1e-8 within 60 cycles: the counts of tests/test_line_cpu.py (TABLE_STABLE); the
    combinations that do not converge stop at the cap on the device as well.  The x-strong 1e-2 problem with x-lines
    in 7 cycles is the solve no earlier version of the library could run: the handle could not be created"""
    b, h_t, h_x = reference_solve(lr.Hierarchy, kind, smoother, 6, 3, 1, TOL, CAP)
    want = TABLE_STABLE[6][kind][SMOOTHERS.index(smoother)]
    st, h, _ = device_solve(pkg, kind, smoother, 6, 3, 1, b, TOL, CAP)
    n = 63
    assert st.fine_updates == st.cycles * 2 * (2 if smoother == lr.LINE_ALT else 1) * n * n
    if not isinstance(want, int):
        assert len(h_t) - 1 == CAP and st.cycles == CAP and st.converged == 0 and h[-1] > 1e-3 * h[0], (kind, smoother, st.cycles, h[-1] / h[0])
    else:
        assert len(h_t) - 1 == want and st.cycles == want and st.converged == 1, (kind, smoother, want, st.cycles, h)
    assert_history(h, h_t, h_x, (kind, NAMES[smoother]))


VARIANTS = {
    "stencil5": dict(cls=lr.Stencil5, kind="x1e-2", smoother=lr.LINE_X, dtype=1, ref={}, dev=dict(op="stencil5")),
    "f32": dict(cls=lr.Hierarchy, kind="x1e-2", smoother=lr.LINE_X, dtype=0, ref={}, dev={}, tol=1e-4),
    "operator-W": dict(cls=lr.OpdepHierarchy, kind="layers", smoother=lr.LINE_ALT, dtype=1, ref=dict(cycle=wr.W), dev=dict(transfer=1, cycle=1), tol=1e-9),
    "fmg": dict(cls=lr.Hierarchy, kind="layers", smoother=lr.LINE_ALT, dtype=1, ref=dict(schedule=gr.FMG), dev=dict(schedule=1, mu0=0), tol=1e-9),
    "bottom-smooth": dict(cls=lr.Hierarchy, kind="y1e-2", smoother=lr.LINE_Y, dtype=1, ref=dict(bottom=gr.SMOOTH), dev=dict(bottom=1)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_one_solve_each_through_the_other_paths(pkg, po, name):
    """levels 6..3: STENCIL5 with the same constant anisotropic stencil on every level; float (to 1e-4: float does not
    reach 1e-8); operator-dependent transfers with the W-cycle and schedule FMG (to 1e-9: at 1e-8 the reference ends within
    [0.5, 2] tol); bottom = SMOOTH"""
    v = VARIANTS[name]
    tol = v.get("tol", TOL)
    b, h_t, h_x = reference_solve(v["cls"], v["kind"], v["smoother"], 6, 3, v["dtype"], tol, CAP, **v["ref"])
    st, h, _ = device_solve(pkg, v["kind"], v["smoother"], 6, 3, v["dtype"], b, tol, CAP, **v["dev"])
    assert h_t[-1] < 0.5 * tol * h_t[0] and len(h_t) - 1 < 20, ("the reference itself", h_t)
    assert st.converged == 1 and st.cycles == len(h_t) - 1, (name, st.cycles, len(h_t) - 1, h, h_t)
    assert_history(h, h_t, h_x, name)


def test_pcg_with_the_alternating_cycle_on_the_layers_problem(pkg, po):
    """flexible PCG needs no symmetric preconditioner: converged, in no more iterations than mgx_solve takes cycles"""
    b, h_t, _ = reference_solve(lr.Hierarchy, "layers", lr.LINE_ALT, 6, 3, 1, TOL, CAP)
    with handle(pkg, 6, 3, lr.LINE_ALT) as mg:
        mg.set_stencil(6, *operator5(po, 6, "layers"))
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=TOL, max_cycles=CAP)
        mg.set_guess(np.zeros_like(b))
        sp, hp = mg.solve_pcg(tol=TOL, max_iters=CAP)
    print(f"mgx_solve {st.cycles} cycles, mgx_solve_pcg {sp.cycles} iterations")
    assert st.converged == 1 and sp.converged == 1 and sp.cycles <= st.cycles, (st.cycles, sp.cycles, hp)


def test_two_solves_and_graph_replay_against_eager_launches_give_the_same_bits(pkg, po, monkeypatch):
    L = 7
    n = (1 << L) - 1
    b = np.random.default_rng(4).uniform(-1, 1, (n, n))

    def solves(**kw):
        with handle(pkg, L, 4, lr.LINE_ALT, **kw) as mg:
            mg.set_stencil(L, *operator5(po, L, "layers"))
            mg.build_galerkin()
            runs = []
            for _ in range(2):
                mg.set_rhs(b)
                mg.set_guess(np.zeros_like(b))
                st, h = mg.solve(tol=1e-9, max_cycles=12)
                runs.append((h, mg.get_solution()))
            return runs, mg.graphs_cached()

    replay, cached = solves()
    assert cached >= 1
    assert np.array_equal(replay[0][0], replay[1][0]) and np.array_equal(replay[0][1], replay[1][1])
    eager_profile, _ = solves(profile=1)
    monkeypatch.setenv("MGX_GRAPH", "0")
    eager, cached = solves()
    assert cached <= 0
    for runs in (eager, eager_profile):
        for h, u in runs:
            assert np.array_equal(h, replay[0][0]) and np.array_equal(u, replay[0][1])


# ---- 6. a rebuilt handle equals a fresh one --------------------------------------------------------------------------
def test_a_rebuilt_handle_equals_a_fresh_one(pkg, po):
    """a second operator on a handle that has solved: new factors, and no cycle graph of the first problem"""
    L, Lc = 6, 3
    n = (1 << L) - 1
    b = np.random.default_rng(2).uniform(-1, 1, (n, n))
    op1, op2 = operator5(po, L, "x1e-2"), operator5(po, L, "layers")

    def state(mg):
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        h = mg.solve(tol=TOL, max_cycles=20)[1]
        return [mg.line_factor(lv, d, w) for lv in range(Lc, L + 1) for d in (0, 1) for w in (0, 1)] + [h, mg.get_solution()]

    with handle(pkg, L, Lc, lr.LINE_ALT) as fresh:
        fresh.set_stencil(L, *op2)
        fresh.build_galerkin()
        want = state(fresh)
    with handle(pkg, L, Lc, lr.LINE_ALT) as mg:
        mg.set_stencil(L, *op1)
        mg.build_galerkin()
        first = state(mg)
        assert mg.graphs_cached() >= 1
        mg.set_stencil(L, *op2)
        mg.build_galerkin()
        got = state(mg)
    assert not np.array_equal(first[0], want[0]) and len(first[-2]) != len(want[-2])
    for a, c in zip(got, want):
        assert np.array_equal(a, c)


# ---- 7. refusals and state -------------------------------------------------------------------------------------------
def test_refusals_name_the_smoother_and_leave_a_jacobi_handle_usable(pkg, po):
    import hipmem as hm
    from test_gpu_solve import hist_close

    L, Lc = 6, 4
    a = pcg_ref.contrast_coefficient(L, 10.0)
    b = po.rhs_sine(L)
    h_ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, Lc).solve(b, tol=1e-9, max_cycles=4)[1]

    def jacobi_still_solves():
        with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OP_GALERKIN, mu1=2, mu2=2, schedule=0) as mg:
            mg.set_coefficient(a)
            mg.build_galerkin()
            mg.set_rhs(b)
            assert hist_close(mg.solve(tol=1e-9, max_cycles=4)[1], h_ref)

    refused = [dict(op=pkg.OPERATOR_POISSON), dict(op=pkg.OPERATOR_POISSON, n_gpus=2), dict(op=pkg.OP_GALERKIN, n_gpus=2),
               dict(op=pkg.OPERATOR_STENCIL5, n_gpus=2), dict(op=pkg.OP_GALERKIN, dtype=pkg.DTYPE_MIXED),
               dict(op=pkg.OPERATOR_STENCIL5, dtype=pkg.DTYPE_MIXED), dict(op=pkg.OP_GALERKIN, arith=pkg.ARITH_FMA),
               dict(op=pkg.OPERATOR_STENCIL5, arith=pkg.ARITH_FMA)]
    for smoother in SMOOTHERS:
        for bad in refused:
            with pytest.raises(pkg.MgxError, match="invalid argument.*LINE"):
                pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=smoother, **bad)
        with pytest.raises(pkg.MgxError, match="invalid argument.*LINE"):
            pkg.Multigrid.rank(0, 2, finest_level=L, coarsest_level=Lc, smoother=smoother)
        with pytest.raises(pkg.MgxError, match="LINE"):
            pkg.Plan(2, 0, finest_level=9, coarsest_level=5, smoother=smoother)
        n_rows = (1 << L) + 1
        pitch = pkg.lib().mgx_level_pitch(L, pkg.DTYPE_F64)
        slab = pkg.Slab(L, pkg.DTYPE_F64, n_rows, 0, 0)
        u, f, t = (hm.zeros((n_rows, pitch), np.float64) for _ in range(3))
        rc = pkg.lib().mgx_slab_cycle(slab, u.data_ptr(), f.data_ptr(), t.data_ptr(), 1, n_rows - 1, 2, 2.0 / 3.0, smoother, None, None, None,
                                      0, 0, 0, 0, None, None, None, None)
        assert rc == 1                                   # MGX_ERR_INVALID
    for value in (3, 7):
        with pytest.raises(pkg.MgxError):
            pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=value, op=pkg.OP_GALERKIN)
    jacobi_still_solves()


def test_a_zero_pivot_is_refused_and_the_handle_solves_after_a_good_operator(pkg, po):
    """c = 1, w = e = -1 (tests/test_line_cpu.py): the second pivot of every x-line is zero"""
    L, Lc = 5, 4
    n = (1 << L) - 1
    one = np.ones((n, n))
    good = operator5(po, L, "x1e-2")
    b = np.random.default_rng(1).uniform(-1, 1, (n, n))
    with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OPERATOR_STENCIL5, smoother=lr.LINE_X, mu1=1, mu2=1, schedule=0) as mg:
        mg.set_stencil(Lc, *operator5(po, Lc, "x1e-2"))
        with pytest.raises(pkg.MgxError, match="invalid argument.*LINE.*level 5.*direction x"):
            mg.set_stencil(L, one, -one, -one, -one, -one)
        with pytest.raises(pkg.MgxError, match="not set"):
            mg.line_factor(L, 0, 0)
        mg.set_stencil(L, *good)
        mg.set_rhs(b)
        st, h = mg.solve(tol=TOL, max_cycles=30)
        assert st.converged == 1
    with handle(pkg, L, Lc, lr.LINE_Y) as mg:
        mg.set_stencil(L, one, -one, -one, -one, -one)               # a GALERKIN handle factors in the build
        with pytest.raises(pkg.MgxError, match="invalid argument.*LINE.*direction y"):
            mg.build_galerkin()
        with pytest.raises(pkg.MgxError, match="not built"):
            mg.line_factor(L, 1, 0)
        mg.set_stencil(L, *operator5(po, L, "y1e-2"))
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=TOL, max_cycles=30)
        assert st.converged == 1


def test_line_factor_states(pkg, po):
    L, Lc = 5, 4
    with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OP_GALERKIN) as mg:
        mg.set_stencil(L, *operator5(po, L, "iso"))
        mg.build_galerkin()
        with pytest.raises(pkg.MgxError, match="invalid state.*line smoother"):
            mg.line_factor(L, 0, 0)
    with pkg.Multigrid(finest_level=L, coarsest_level=Lc) as mg:
        with pytest.raises(pkg.MgxError, match="invalid state.*line smoother"):
            mg.line_factor(L, 0, 0)
    with handle(pkg, L, Lc, lr.LINE_X) as mg:
        mg.set_stencil(L, *operator5(po, L, "iso"))
        with pytest.raises(pkg.MgxError, match="invalid state.*not built"):
            mg.line_factor(L, 0, 0)
        mg.build_galerkin()
        assert mg.line_factor(L, 0, 0).shape == (31, 31)
        with pytest.raises(pkg.MgxError, match="invalid state.*no y-lines"):
            mg.line_factor(L, 1, 0)
        with pytest.raises(pkg.MgxError, match="invalid state.*no y-lines"):
            mg.line_chunks(L)
        with pytest.raises(pkg.MgxError, match="out of range"):
            mg.line_factor(L, 2, 0)
        with pytest.raises(pkg.MgxError, match="out of range"):
            mg.line_factor(Lc - 1, 0, 0)
    with handle(pkg, L, Lc, lr.LINE_Y) as mg:
        mg.set_stencil(L, *operator5(po, L, "iso"))
        mg.build_galerkin()
        with pytest.raises(pkg.MgxError, match="invalid state.*no x-lines"):
            mg.line_factor(L, 0, 1)
    with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OPERATOR_STENCIL5, smoother=lr.LINE_ALT) as mg:
        with pytest.raises(pkg.MgxError, match="invalid state.*not set"):
            mg.line_factor(L, 0, 0)


def test_time_smoother_and_launch_counts(pkg, po):
    """mgx_time_smoother(2) is two sweeps; an alternating sweep is four launches (profile class 0: MGX_PROF_SMOOTH_FINE)"""
    L = 6
    st5 = operator5(po, L, "layers")
    n = (1 << L) - 1
    rng = np.random.default_rng(3)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    for smoother in SMOOTHERS:
        with handle(pkg, L, 4, smoother, profile=1) as mg:
            mg.set_stencil(L, *st5)
            mg.build_galerkin()
            want = mg.jacobirelaxation(L, u, b, 2)
            mg.set_guess(u)
            mg.set_rhs(b)
            assert mg.time_smoother(2) > 0.0
            assert np.array_equal(mg.get_solution(), want)
            mg.profile_reset()
            mg.set_guess(u)
            mg.smooth(L, 3)
            launches = mg.profile()["launches"]
            assert launches[0] == 3 * (4 if smoother == lr.LINE_ALT else 2), (smoother, launches)
