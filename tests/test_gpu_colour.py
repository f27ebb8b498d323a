"""GPU tests of the multicolour Gauss-Seidel smoothers (cfg.smoother = MGX_SMOOTHER_COLOR_GS / COLOR_SGS,
csrc/mgx_colour.hpp) against the numpy statement of tests/colour_ref.py (whose properties tests/test_colour_cpu.py checks).

The project's rule for point kernels: sweeps are compared with np.array_equal; iterates and histories of whole solves to
1e-10 relative in double and 1e-6 in float (the dense coarsest solve is the one step that is not bit for bit), as in
tests/test_gpu_galerkin.py.

Shapes.  A strip is 62 lanes x 16 bytes, 124 doubles or 248 floats: level 7 in double and level 8 in float are the smallest
levels whose rows span two strips; level 2 is a row of one vector.  k_gs_rb takes chunks of 8 rows below N = 1024
(gs_chunk_rows), and a level has 2^L - 1 interior rows, never a multiple of 8: every fused level ends in a short chunk
(7 rows at levels 5, 7, 8 and 9), and level 3 (7 rows) is below a chunk and runs the per-colour form."""
import functools

import numpy as np
import pytest

import colour_ref as cf
import galerkin_ref as gr
import gcr_ref
import nine_ref as nr
import pcg_ref
import wcycle_ref as wr
from test_galerkin_cpu import with_ring_values
from test_gpu_galerkin import np_dtype
from test_line_cpu import operator5

pytestmark = pytest.mark.gpu

SMOOTHERS = (cf.COLOR_GS, cf.COLOR_SGS)
IDS = [cf.NAMES[s] for s in SMOOTHERS]
RTOL = {1: 1e-10, 0: 1e-6}


def chunk_rows(N):
    """gs_chunk_rows of csrc/mgx_colour.hpp"""
    return 16 if N >= 1024 else 8


def handle(pkg, finest, coarsest, smoother, **kw):
    cfg = dict(finest_level=finest, coarsest_level=coarsest, op=pkg.OP_GALERKIN, smoother=smoother, mu1=1, mu2=1, schedule=0)
    cfg.update(kw)
    return pkg.Multigrid(**cfg)


def random5(L, seed, dt=np.float64):
    """an unsymmetric, strictly diagonally dominant five-point operator with values in the ring-pointing places too"""
    n = (1 << L) - 1
    rng = np.random.default_rng(seed)
    off = [-rng.uniform(0.2, 1.0, (n, n)) for _ in range(4)]
    c = sum(np.abs(o) for o in off) + rng.uniform(0.05, 0.5, (n, n))
    return [np.ascontiguousarray(x.astype(dt)) for x in [c] + off]


def five_point(po, L, kind, dt):
    return random5(L, 70 + L, dt) if kind == "random" else operator5(po, L, kind, dt)


def rand(L, seed, dt=np.float64):
    n = (1 << L) - 1
    return np.random.default_rng(seed).uniform(-1, 1, (n, n)).astype(dt)


@functools.lru_cache(maxsize=None)
def galerkin_ops(kind, finest, coarsest, dtype):
    """the operators of a GALERKIN hierarchy whose five-point finest level carries `kind`, in the working type (bit for
    bit the device's: tests/test_gpu_galerkin.py)"""
    from oracle import pyoracle as po
    st = {finest: gr.nine(five_point(po, finest, kind, np_dtype(dtype)))}
    for lv in range(finest, coarsest, -1):
        st[lv - 1] = gr.rap(st[lv], 1 << lv)
    return st


def check_sweeps(mg, lv, st9, nine, dt, what, mus=(1, 3)):
    """mu forward sweeps (mgx_smooth) on a level from a random v and b against colour_ref, bit for bit"""
    v, b = rand(lv, 1000 + lv, dt), rand(lv, 2000 + lv, dt)
    dinv = cf.dinv_of(st9)
    for mu in mus:
        got = mg.jacobirelaxation(lv, v, b, mu)
        assert got.dtype == dt
        assert np.array_equal(got, cf.smooth(st9, dinv, v, b, mu, nine)), (what, lv, mu)


# ---- 1. sweeps, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,finest,levels", [(1, 7, (2, 3, 5, 7)), (0, 8, (8,))], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["contrast", "layers", "random"])
def test_five_point_sweeps_are_bit_identical_to_the_reference(pkg, po, kind, dtype, finest, levels):
    """STENCIL5: level 2 (one vector a row), 3 (below a chunk: per-colour launches), 5, 7 (two strips in double), 8 in float"""
    dt = np_dtype(dtype)
    with pkg.Multigrid(finest_level=finest, coarsest_level=2, op=pkg.OPERATOR_STENCIL5, smoother=cf.COLOR_GS, dtype=dtype) as mg:
        ops = {lv: five_point(po, lv, kind, dt) for lv in range(2, finest + 1)}
        for lv, st5 in ops.items():
            mg.set_stencil(lv, *st5)
        for lv in levels:
            assert np.array_equal(mg.get_stencil(lv, 5), cf.dinv_of(gr.nine(ops[lv])))
            check_sweeps(mg, lv, gr.nine(ops[lv]), False, dt, ("STENCIL5", kind))


@pytest.mark.parametrize("dtype,finest,coarsest,levels", [(1, 8, 3, (3, 5, 7)), (0, 9, 4, (8,))], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["contrast", "layers", "random"])
def test_nine_point_sweeps_are_bit_identical_to_the_reference(pkg, po, kind, dtype, finest, coarsest, levels):
    """the built levels of a GALERKIN hierarchy (and its five-point finest level, fused): 3, 5, 7 in double, 8 in float"""
    dt = np_dtype(dtype)
    st = galerkin_ops(kind, finest, coarsest, dtype)
    with handle(pkg, finest, coarsest, cf.COLOR_SGS, dtype=dtype) as mg:
        mg.set_stencil(finest, *st[finest][:5])
        mg.build_galerkin()
        for lv in levels:
            assert np.array_equal(mg.get_stencil9(lv, 9), cf.dinv_of(st[lv]))
            check_sweeps(mg, lv, st[lv], True, dt, ("GALERKIN", kind))
        check_sweeps(mg, finest, st[finest], False, dt, ("GALERKIN finest", kind), mus=(1,))


@pytest.mark.parametrize("dtype,L", [(1, 7), (1, 4), (0, 8)], ids=["f64-7", "f64-4", "f32-8"])
def test_a_nine_point_finest_level_with_corners(pkg, po, dtype, L):
    """mgx_set_stencil9: unsymmetric, corner coefficients, values in the ring-pointing places"""
    dt = np_dtype(dtype)
    st9 = nr.random_stencil9(L, 5, dt)
    with handle(pkg, L, 3, cf.COLOR_GS, dtype=dtype) as mg:
        mg.set_stencil9(L, *st9)
        mg.build_galerkin()
        check_sweeps(mg, L, st9, True, dt, "stencil9")


# ---- 2. fused equals unfused, forward and reverse ----------------------------------------------------------------------
def one_level_sweeps(pkg, po, L, dtype, monkeypatch, fused, kind="contrast", mus=(1, 2, 3)):
    """{(direction, mu): iterate} of mu = 1, 2, 3 sweeps on the five-point level L, and the launches of three forward
    sweeps.  Forward: mgx_smooth.  Reverse: a COLOR_SGS handle with finest = coarsest = L, bottom = SMOOTH, mu1 = 0: its
    'cycle' is mu2 post-smoothing sweeps"""
    dt = np_dtype(dtype)
    if fused:
        monkeypatch.delenv("MGX_GS_FUSED", raising=False)
    else:
        monkeypatch.setenv("MGX_GS_FUSED", "0")
    st5 = five_point(po, L, kind, dt)
    v, b = rand(L, 31, dt), rand(L, 32, dt)
    out = {}
    for mu in mus:
        with pkg.Multigrid(finest_level=L, coarsest_level=L, op=pkg.OPERATOR_STENCIL5, smoother=cf.COLOR_SGS, dtype=dtype, mu1=0, mu2=mu,
                           bottom=1, schedule=0, profile=1) as mg:
            mg.set_stencil(L, *st5)
            out["forward", mu] = mg.jacobirelaxation(L, v, b, mu)
            out["reverse", mu] = mg.vcyclemultigrid(L, v, b)
            mg.profile_reset()
            mg.smooth(L, 3)
            launches = mg.profile()["launches"][0]
    return out, launches, gr.nine(st5), v, b


@pytest.mark.parametrize("dtype,L", [(1, 5), (1, 7), (1, 9), (0, 8)], ids=["f64-5", "f64-7", "f64-9", "f32-8"])
def test_the_fused_pass_equals_the_per_colour_launches(pkg, po, monkeypatch, dtype, L):
    N = 1 << L
    # the launcher's chunks at these levels: 8 rows, and the last chunk of every strip is short (7 rows)
    assert chunk_rows(N) == 8 and (N - 1) % chunk_rows(N) == 7 and (N - 1) // chunk_rows(N) >= 3
    fused, n_fused, st9, v, b = one_level_sweeps(pkg, po, L, dtype, monkeypatch, True)
    plain, n_plain, _, _, _ = one_level_sweeps(pkg, po, L, dtype, monkeypatch, False)
    assert n_fused == 3 and n_plain == 6, (n_fused, n_plain)           # one launch a sweep against one a colour
    dinv = cf.dinv_of(st9)
    for (direction, mu), got in fused.items():
        assert np.array_equal(got, plain[direction, mu]), (direction, mu)
        assert np.array_equal(got, cf.smooth(st9, dinv, v, b, mu, False, reverse=direction == "reverse")), (direction, mu)
    assert not np.array_equal(fused["forward", 1], fused["reverse", 1])


@pytest.mark.parametrize("kind", ["contrast", "random"])
@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
def test_the_sixteen_row_chunks_of_the_fused_pass(pkg, po, monkeypatch, dtype, kind):
    """from N = 1024 up gs_chunk_rows is 16: a rolling window of 16 rows, and a last chunk of 15.  Level 10 is the smallest
    level that takes this path (level 9: 8 rows, above), so it is the size of this test: one and three sweeps, forward
    and in reverse, against colour_ref and against the per-colour launches, bit for bit"""
    L = 10
    N = 1 << L
    assert chunk_rows(N) == 16 and chunk_rows(N // 2) == 8 and (N - 1) % 16 == 15 and (N - 1) // 16 >= 3
    strip = 62 * 16 // np.dtype(np_dtype(dtype)).itemsize
    assert strip == (124 if dtype == 1 else 248) and -(-(N - 1) // strip) > 1          # more than one strip in either type
    fused, n_fused, st9, v, b = one_level_sweeps(pkg, po, L, dtype, monkeypatch, True, kind, mus=(1, 3))
    plain, n_plain, _, _, _ = one_level_sweeps(pkg, po, L, dtype, monkeypatch, False, kind, mus=(1, 3))
    assert n_fused == 3 and n_plain == 6, (n_fused, n_plain)           # one launch a sweep against one a colour
    dinv = cf.dinv_of(st9)
    assert set(fused) == {(d, mu) for d in ("forward", "reverse") for mu in (1, 3)}
    for (direction, mu), got in fused.items():
        assert got.dtype == np_dtype(dtype)
        want = cf.smooth(st9, dinv, v, b, mu, False, reverse=direction == "reverse")
        assert np.array_equal(got, want), (direction, mu, np.argwhere(got != want)[:4])
        assert np.array_equal(got, plain[direction, mu]), (direction, mu)
    assert not np.array_equal(fused["forward", 1], fused["reverse", 1])


# ---- 3. ring-pointing coefficients --------------------------------------------------------------------------------------
def test_coefficients_that_point_at_the_ring_change_no_bit(pkg, po):
    """values up to 1e30 of mixed sign there multiply the zero ring of the iterate: five-point fused (level 6), five-point
    per colour (MGX_GS_FUSED=0 is not needed: level 3) and a nine-point finest level"""
    for L in (6, 3):
        st5 = five_point(po, L, "contrast", np.float64)
        v, b = rand(L, 6), rand(L, 7)
        out = []
        for op in (st5, with_ring_values(st5, 5)):
            with pkg.Multigrid(finest_level=L, coarsest_level=L, op=pkg.OPERATOR_STENCIL5, smoother=cf.COLOR_GS, bottom=1) as mg:
                mg.set_stencil(L, *op)
                out.append(mg.jacobirelaxation(L, v, b, 2))
        assert np.array_equal(out[0], out[1]), L
    L = 5
    st9 = nr.random_stencil9(L, 8)
    v, b = rand(L, 9), rand(L, 10)
    out = []
    for op in (st9, nr.with_ring_values9(st9, 11)):
        with handle(pkg, L, 3, cf.COLOR_GS) as mg:
            mg.set_stencil9(L, *op)
            mg.build_galerkin()
            out.append(mg.jacobirelaxation(L, v, b, 2))
    assert np.array_equal(out[0], out[1])


# ---- 4. cycles and solves ------------------------------------------------------------------------------------------------
CYCLES = 5

CASES = {
    # name: (reference class, operator kind, finest, coarsest, reference keywords, device keywords, device transfer, cycle)
    "galerkin": (cf.Hierarchy, "contrast", 7, 4, {}, {}, None, None),
    "operator-P": (cf.OpdepHierarchy, "contrast", 7, 4, {}, {}, 1, None),
    "stencil5": (cf.Stencil5, "layers", 6, 4, {}, dict(op="stencil5"), None, None),
    "bottom-smooth": (cf.Hierarchy, "contrast", 5, 3, dict(bottom=gr.SMOOTH), dict(bottom=1), None, None),
    "W": (cf.Hierarchy, "contrast", 7, 4, dict(cycle=wr.W), {}, None, 1),
    "F": (cf.OpdepHierarchy, "contrast", 7, 4, dict(cycle=wr.F), {}, 1, 2),
    "fmg": (cf.Hierarchy, "contrast", 7, 4, {}, dict(schedule=1, mu0=0), None, None),
}


@functools.lru_cache(maxsize=None)
def reference_solve(name, smoother, mu1, mu2, dtype=1):
    from oracle import pyoracle as po
    cls, kind, finest, coarsest, ref_kw, dev_kw, _, _ = CASES[name]
    dt = np_dtype(dtype)
    if cls is cf.Stencil5:
        op = {lv: five_point(po, lv, kind, dt) for lv in range(coarsest, finest + 1)}
    else:
        op = five_point(po, finest, kind, dt)
    b = rand(finest, 77, dt)
    h = cls(smoother, po, op, finest, coarsest, dt, mu1=mu1, mu2=mu2, **ref_kw)
    u, hist = h.solve(b, tol=0.0, max_cycles=CYCLES, schedule=gr.FMG if dev_kw.get("schedule") else gr.V)
    return b, u, np.asarray(hist, dtype=np.float64)


def device_solve(pkg, po, name, smoother, mu1, mu2, dtype=1):
    _, kind, finest, coarsest, _, dev_kw, transfer, cycle = CASES[name]
    dt = np_dtype(dtype)
    kw = dict(dev_kw)
    stencil5 = kw.pop("op", None) == "stencil5"
    if stencil5:
        kw["op"] = pkg.OPERATOR_STENCIL5
    with handle(pkg, finest, coarsest, smoother, dtype=dtype, mu1=mu1, mu2=mu2, **kw) as mg:
        if stencil5:
            for lv in range(coarsest, finest + 1):
                mg.set_stencil(lv, *five_point(po, lv, kind, dt))
        else:
            mg.set_stencil(finest, *five_point(po, finest, kind, dt))
            mg.build_galerkin(transfer)
        if cycle is not None:
            mg.set_cycle(cycle)
        mg.set_rhs(rand(finest, 77, dt))
        st, h = mg.solve(tol=0.0, max_cycles=CYCLES)
        return st, h, mg.get_solution()


def assert_solve(st, h, u, h_ref, u_ref, dtype, n, sweeps, what):
    assert st.cycles == CYCLES and len(h) == len(h_ref) == CYCLES + 1, (what, st.cycles, h, h_ref)
    d_h = float(np.max(np.abs(h - h_ref) / h_ref))
    d_u = float(np.max(np.abs(u - u_ref)) / np.max(np.abs(u_ref)))
    print(f"{what}: history {h_ref[0]:.3e} -> {h_ref[-1]:.3e}; device - reference: history {d_h:.3e} relative, iterate {d_u:.3e} of max|u|")
    assert h_ref[-1] < h_ref[0], ("the reference itself", h_ref)
    assert d_h <= RTOL[dtype] and d_u <= RTOL[dtype], (what, d_h, d_u)
    assert st.fine_updates == st.cycles * sweeps * n * n, (what, st.fine_updates)


@pytest.mark.parametrize("mu1,mu2", [(1, 1), (2, 1)], ids=["V11", "V21"])
@pytest.mark.parametrize("smoother", SMOOTHERS, ids=IDS)
@pytest.mark.parametrize("name", ["galerkin", "operator-P", "stencil5"])
def test_v_cycles_follow_the_reference(pkg, po, name, smoother, mu1, mu2):
    """GALERKIN 7..4 with bilinear and operator-dependent P, STENCIL5 6..4: five V-cycles from zero"""
    b, u_ref, h_ref = reference_solve(name, smoother, mu1, mu2)
    st, h, u = device_solve(pkg, po, name, smoother, mu1, mu2)
    assert_solve(st, h, u, h_ref, u_ref, 1, b.shape[0], mu1 + mu2, (name, cf.NAMES[smoother], mu1, mu2))


@pytest.mark.parametrize("smoother", SMOOTHERS, ids=IDS)
@pytest.mark.parametrize("name", ["bottom-smooth", "W", "F", "fmg"])
def test_the_other_schedules_follow_the_reference(pkg, po, name, smoother):
    """bottom = SMOOTH on 5..3 with V(2,1) (COLOR_SGS: two forward sweeps, then one in reverse, at the bottom); a W- and an
    F-cycle on 7..4 (levels 6 and 5 are small nine-point levels: the one-workgroup visit must be bypassed, and every block
    keeps the direction of its position); the FMG schedule"""
    mu1, mu2 = (2, 1) if name == "bottom-smooth" else (1, 1)
    b, u_ref, h_ref = reference_solve(name, smoother, mu1, mu2)
    st, h, u = device_solve(pkg, po, name, smoother, mu1, mu2)
    n = b.shape[0]
    assert st.cycles == CYCLES and len(h) == len(h_ref)
    d_h = float(np.max(np.abs(h - h_ref) / h_ref))
    d_u = float(np.max(np.abs(u - u_ref)) / np.max(np.abs(u_ref)))
    print(f"{name} {cf.NAMES[smoother]}: history {h_ref[0]:.3e} -> {h_ref[-1]:.3e}; history {d_h:.3e} relative, iterate {d_u:.3e} of max|u|")
    assert h_ref[-1] < h_ref[0] and d_h <= RTOL[1] and d_u <= RTOL[1], (name, d_h, d_u)
    if name == "bottom-smooth" and smoother == cf.COLOR_SGS:
        # the direction at the bottom matters: the forward-only reference is another iteration
        _, u_gs, _ = reference_solve(name, cf.COLOR_GS, mu1, mu2)
        assert np.max(np.abs(u_gs - u_ref)) > 1e-6 * np.max(np.abs(u_ref))


def test_a_float_solve_follows_the_reference(pkg, po):
    b, u_ref, h_ref = reference_solve("galerkin", cf.COLOR_SGS, 1, 1, dtype=0)
    st, h, u = device_solve(pkg, po, "galerkin", cf.COLOR_SGS, 1, 1, dtype=0)
    assert_solve(st, h, u, h_ref, u_ref, 0, b.shape[0], 2, "float")


# ---- 5. Krylov -----------------------------------------------------------------------------------------------------------
def test_pcg_with_the_symmetric_cycle_follows_the_reference(pkg, po):
    """mgx_solve_pcg around the COLOR_SGS V(1,1) cycle on the symmetric contrast-100 operator at 7..4"""
    L, Lc = 7, 4
    st5 = five_point(po, L, "contrast", np.float64)
    b = rand(L, 81)
    ref = cf.Hierarchy(cf.COLOR_SGS, po, st5, L, Lc, np.float64, mu1=1, mu2=1)
    x_ref, h_ref, conv, brk = pcg_ref.pcg(pcg_ref.Operator(st5, np.float64), gcr_ref.cycle_preconditioner(ref), b, np.zeros_like(b), 1e-8, 40)
    assert conv and not brk
    with handle(pkg, L, Lc, cf.COLOR_SGS) as mg:
        mg.set_stencil(L, *st5)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=40)
        x = mg.get_solution()
    d_h = float(np.max(np.abs(h[:len(h_ref)] - h_ref[:len(h)]) / h_ref[:len(h)]))
    d_x = float(np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)))
    print(f"PCG / SGS: {st.cycles} iterations (reference {len(h_ref) - 1}); history {d_h:.3e} relative, iterate {d_x:.3e} of max|x|")
    assert st.converged == 1 and st.cycles == len(h_ref) - 1, (st.cycles, h, h_ref)      # converged: no breakdown either
    assert d_h <= RTOL[1] and d_x <= RTOL[1], (d_h, d_x)


def test_gcr_with_the_forward_cycle_on_an_unsymmetric_nine_point_operator(pkg, po):
    """mgx_solve_gcr(restart = 4) around the COLOR_GS V(1,1) cycle, nine-point finest level 6..3"""
    L, Lc = 6, 3
    st9 = nr.random_stencil9(L, 91)
    b = rand(L, 92)
    ref = cf.NineHierarchy(cf.COLOR_GS, po, st9, L, Lc, np.float64, mu1=1, mu2=1)
    x_ref, h_ref, conv, brk = gcr_ref.gcr(nr.Operator9(st9), gcr_ref.cycle_preconditioner(ref), b, np.zeros_like(b), 1e-8, 40, 4)
    assert conv and not brk
    with handle(pkg, L, Lc, cf.COLOR_GS) as mg:
        mg.set_stencil9(L, *st9)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve_gcr(tol=1e-8, max_iters=40, restart=4)
        x = mg.get_solution()
    d_h = float(np.max(np.abs(h[:len(h_ref)] - h_ref[:len(h)]) / h_ref[:len(h)]))
    d_x = float(np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)))
    print(f"GCR(4) / GS: {st.cycles} iterations (reference {len(h_ref) - 1}); history {d_h:.3e} relative, iterate {d_x:.3e} of max|x|")
    assert st.converged == 1 and st.cycles == len(h_ref) - 1, (st.cycles, h, h_ref)
    assert np.all(np.diff(h) <= 0.0), h
    assert d_h <= RTOL[1] and d_x <= RTOL[1], (d_h, d_x)


# ---- 6. the cycle-count claim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ["poisson", "rotated"])
def test_gs_v11_needs_no_more_cycles_than_jacobi_v22(pkg, po, problem):
    """7..3 to 1e-8 from a random right-hand side: COLOR_GS V(1,1) - half the sweeps - converges in no more cycles than
    Jacobi V(2,2), and in exactly the cycles of colour_ref"""
    L, Lc = 7, 3
    b = rand(L, 61)
    if problem == "poisson":
        op = operator5(po, L, "iso")
        ref = cf.Hierarchy(cf.COLOR_GS, po, op, L, Lc, np.float64, mu1=1, mu2=1)
    else:
        op = nr.tensor9(*nr.rotated_tensor(L, 45.0, 0.5))
        ref = cf.NineHierarchy(cf.COLOR_GS, po, op, L, Lc, np.float64, mu1=1, mu2=1)
    want = len(ref.solve(b, tol=1e-8, max_cycles=40)[1]) - 1
    counts = {}
    for name, kw in (("gs", dict(smoother=cf.COLOR_GS, mu1=1, mu2=1)), ("jacobi", dict(smoother=pkg.SMOOTHER_JACOBI, mu1=2, mu2=2))):
        with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OP_GALERKIN, schedule=0, **kw) as mg:
            if problem == "poisson":
                mg.set_stencil(L, *op)
            else:
                mg.set_stencil9(L, *op)
            mg.build_galerkin()
            mg.set_rhs(b)
            st, h = mg.solve(tol=1e-8, max_cycles=40)
            assert st.converged == 1, (name, h)
            counts[name] = st.cycles
    print(f"{problem}: COLOR_GS V(1,1) {counts['gs']} cycles (colour_ref {want}), Jacobi V(2,2) {counts['jacobi']} cycles")
    assert counts["gs"] == want
    assert counts["gs"] <= counts["jacobi"]


# ---- 7. state and refusals -----------------------------------------------------------------------------------------------
def test_refusals_name_the_smoother(pkg, po):
    import hipmem as hm

    L, Lc = 6, 4
    refused = [dict(op=pkg.OPERATOR_POISSON), dict(op=pkg.OPERATOR_POISSON, n_gpus=2), dict(op=pkg.OP_GALERKIN, n_gpus=2),
               dict(op=pkg.OPERATOR_STENCIL5, n_gpus=2), dict(op=pkg.OP_GALERKIN, dtype=pkg.DTYPE_MIXED),
               dict(op=pkg.OPERATOR_STENCIL5, dtype=pkg.DTYPE_MIXED), dict(op=pkg.OP_GALERKIN, arith=pkg.ARITH_FMA),
               dict(op=pkg.OPERATOR_STENCIL5, arith=pkg.ARITH_FMA)]
    for smoother in SMOOTHERS:
        for bad in refused:
            with pytest.raises(pkg.MgxError, match="invalid argument.*COLOR_GS"):
                pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=smoother, **bad)
        with pytest.raises(pkg.MgxError, match="invalid argument.*COLOR_GS"):
            pkg.Multigrid.rank(0, 2, finest_level=L, coarsest_level=Lc, smoother=smoother)
        with pytest.raises(pkg.MgxError, match="COLOR_GS"):
            pkg.Plan(2, 0, finest_level=9, coarsest_level=5, smoother=smoother)
        n_rows = (1 << L) + 1
        pitch = pkg.lib().mgx_level_pitch(L, pkg.DTYPE_F64)
        slab = pkg.Slab(L, pkg.DTYPE_F64, n_rows, 0, 0)
        u, f, t = (hm.zeros((n_rows, pitch), np.float64) for _ in range(3))
        rc = pkg.lib().mgx_slab_cycle(slab, u.data_ptr(), f.data_ptr(), t.data_ptr(), 1, n_rows - 1, 2, 2.0 / 3.0, smoother, None, None, None,
                                      0, 0, 0, 0, None, None, None, None)
        assert rc == 1                                   # MGX_ERR_INVALID
        # accepted where valid, in both types
        for op in (pkg.OP_GALERKIN, pkg.OPERATOR_STENCIL5):
            for dtype in (pkg.DTYPE_F64, pkg.DTYPE_F32):
                pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=smoother, op=op, dtype=dtype).close()
    for value in (1, 3, 7, 10):                          # RBGS stays refused on general operators; 3, 7 and 10 are no smoothers
        with pytest.raises(pkg.MgxError):
            pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=value, op=pkg.OP_GALERKIN)


def test_graph_replay_and_eager_launches_give_the_same_bits_over_three_solves(pkg, po, monkeypatch):
    L = 7
    b = rand(L, 4)
    st5 = five_point(po, L, "contrast", np.float64)

    def solves(**kw):
        with handle(pkg, L, 4, cf.COLOR_SGS, **kw) as mg:
            mg.set_stencil(L, *st5)
            mg.build_galerkin()
            runs = []
            for _ in range(3):
                mg.set_rhs(b)
                mg.set_guess(np.zeros_like(b))
                st, h = mg.solve(tol=1e-9, max_cycles=12)
                runs.append((h, mg.get_solution()))
            return runs, mg.graphs_cached()

    replay, cached = solves()
    assert cached >= 1
    monkeypatch.setenv("MGX_GRAPH", "0")
    eager, cached = solves()
    assert cached <= 0
    for h, u in replay[1:] + eager:
        assert np.array_equal(h, replay[0][0]) and np.array_equal(u, replay[0][1])


def test_a_long_lived_handle_gives_the_bits_of_fresh_handles(pkg, po):
    """two solves interleaved with mgx_set_stencil -> mgx_build_galerkin: each equals the solve of a fresh handle"""
    L, Lc = 6, 3
    b = rand(L, 2)
    ops = [five_point(po, L, "contrast", np.float64), five_point(po, L, "random", np.float64)]

    def state(mg):
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        h = mg.solve(tol=1e-8, max_cycles=20)[1]
        return h, mg.get_solution()

    want = []
    for op in ops:
        with handle(pkg, L, Lc, cf.COLOR_SGS) as fresh:
            fresh.set_stencil(L, *op)
            fresh.build_galerkin()
            want.append(state(fresh))
    got = []
    with handle(pkg, L, Lc, cf.COLOR_SGS) as mg:
        for op in ops:
            mg.set_stencil(L, *op)
            mg.build_galerkin()
            got.append(state(mg))
        assert mg.graphs_cached() >= 1
    assert not np.array_equal(want[0][1], want[1][1])
    for (h, u), (h_w, u_w) in zip(got, want):
        assert np.array_equal(h, h_w) and np.array_equal(u, u_w)


def test_time_smoother_and_launch_counts(pkg, po):
    """mgx_time_smoother(2) is two forward sweeps under either smoother; launches per sweep: 1 on a fused five-point
    level, 4 on a nine-point one (profile class 0: MGX_PROF_SMOOTH_FINE)"""
    L = 6
    u, b = rand(L, 3), rand(L, 5)
    for nine, per_sweep in ((False, 1), (True, 4)):
        op = nr.random_stencil9(L, 13) if nine else five_point(po, L, "contrast", np.float64)
        for smoother in SMOOTHERS:
            with handle(pkg, L, 4, smoother, profile=1) as mg:
                if nine:
                    mg.set_stencil9(L, *op)
                else:
                    mg.set_stencil(L, *op)
                mg.build_galerkin()
                want = mg.jacobirelaxation(L, u, b, 2)
                mg.set_guess(u)
                mg.set_rhs(b)
                assert mg.time_smoother(2) > 0.0
                assert np.array_equal(mg.get_solution(), want)
                mg.profile_reset()
                mg.set_guess(u)
                mg.smooth(L, 3)
                assert mg.profile()["launches"][0] == 3 * per_sweep
