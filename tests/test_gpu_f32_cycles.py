"""Pure-fp32 POISSON handles against the oracle BIT FOR BIT.  The reference (Poissons_SYCL.cpp) is an fp32
program; a dtype = F32 handle performs the oracle's float operations in the oracle's order, the sine-transform
bottom solve included (oracle_cfg: ORC_BOTTOM_DST), so every iterate is held to np.array_equal - one rounding,
one weight or one operand order off fails - and every residual history (the same float residual summed in
double in a different order) to the project's own 1e-10 per cycle (HIST_TOL).

 a. a seeded fuzz of 48 configurations (levels 6..11, both smoothers, V and FMG, both restriction weights,
    both bottom modes, both rounding modes of the Jacobi update) under three kernel selections;
 b. every one-pass depth of the float folded marching kernels (k_jacobi_cycle<float, K, ...>), around the
    float-only holes of the instantiation set, in the planner's own plan and in one forced split;
 c. the stand-alone schedule entry points (vcyclemultigrid, fullmultigrid, mgx_vcycle_zero) in fp32;
 d. the float operator bits no other test pins: Jacobi at omega != 2/3 in both rounding modes, FW16 transfers.
"""
import numpy as np
import pytest

from test_gpu_solve import HIST_TOL, hist_close, oracle_cfg, run_gpu

pytestmark = pytest.mark.gpu

KNOBS = ("MGX_TILE_MAX_N", "MGX_TILE_WIDE", "MGX_TILE_K", "MGX_TILE_SHORT_N", "MGX_PLAN_MIN_N", "MGX_PLAN_PRE",
         "MGX_PLAN_POST", "MGX_FOLD", "MGX_FUSE", "MGX_GRAPH")


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def assert_bits(u, h, u_ref, h_ref, what):
    assert u.dtype == np.float32, what
    assert len(h) == len(h_ref), (what, h, h_ref)
    assert hist_close(h, h_ref, HIST_TOL), (what, h, h_ref)
    assert np.array_equal(u.astype(np.float64), u_ref), \
        (what, int(np.count_nonzero(u.astype(np.float64) != u_ref)), float(np.max(np.abs(u - u_ref))))


# ---- a. seeded fuzz ------------------------------------------------------------------------------------------
def draw(seed=20261019, cases=48):
    rng = np.random.default_rng(seed)
    out = []
    for case in range(cases):
        finest = int(rng.integers(6, 12))
        coarsest = min(int(rng.integers(max(2, finest - 5), finest + 1)), 8)
        smoother = int(rng.integers(0, 2))
        top = 6 if smoother else 11
        cfg = dict(finest_level=finest, coarsest_level=coarsest, mu0=int(rng.integers(0, 2)),
                   mu1=int(rng.integers(0, top)), mu2=int(rng.integers(0, top)),
                   omega=float(rng.choice([2.0 / 3.0, 0.8, 0.5, 0.4])), smoother=smoother, dtype=0,
                   schedule=int(rng.integers(0, 2)), restrict_mode=int(rng.choice([0, 0, 1])),
                   bottom=int(rng.choice([0, 0, 1])), arith=int(rng.integers(0, 2)) if smoother == 0 else 0)
        if cfg["mu1"] + cfg["mu2"] == 0:
            cfg["mu1"] = 1
        out.append(cfg)
    return out


FUZZ = draw()
# kernel selections: the default (register tiles up to 1024^2, marching above), marching / folded kernels on
# every level with 256 columns or more, and k_tile_wide on the float levels too
SELECTIONS = {"default": {}, "marching": {"MGX_TILE_MAX_N": "0"}, "wide": {"MGX_TILE_WIDE": "2"}}


def fuzz_id(c):
    g = FUZZ[c]
    return (f"c{c:02d}-L{g['finest_level']}.{g['coarsest_level']}-{'gs' if g['smoother'] else 'jac'}"
            f"{g['mu0']}.{g['mu1']}.{g['mu2']}-w{g['omega']:.2f}-{'fmg' if g['schedule'] else 'v'}"
            f"-{'fw16' if g['restrict_mode'] else 'cons'}-{'smooth' if g['bottom'] else 'exact'}"
            f"-{'fma' if g['arith'] else 'sep'}")


_fuzz_ref = {}


def fuzz_problem(po, c):
    """inputs and the oracle's answer of fuzz case c, computed once (the three selections of a case run in turn)"""
    if c not in _fuzz_ref:
        _fuzz_ref.clear()
        cfg = FUZZ[c]
        L = cfg["finest_level"]
        n = (1 << L) - 1
        b = (po.rhs_sine(L) if c % 2 else po.rhs_constant(L)).astype(np.float32)
        u0 = po.fill_uniform((n, n), 3000 + c).astype(np.float32) if c % 3 == 0 and cfg["schedule"] == 0 else None
        u_ref, h_ref = po.Solver(**oracle_cfg(po, cfg)).solve(b, u0, tol=0.0, max_cycles=3)
        for a in (b, u0, u_ref, h_ref):
            if a is not None:
                a.setflags(write=False)
        _fuzz_ref[c] = (b, u0, u_ref, h_ref)
    return _fuzz_ref[c]


@pytest.mark.parametrize("selection", list(SELECTIONS))       # (the upper decorator varies fastest)
@pytest.mark.parametrize("c", range(len(FUZZ)), ids=fuzz_id)
def test_f32_fuzz_is_bit_equal_to_the_oracle(pkg, po, monkeypatch, selection, c):
    b, u0, u_ref, h_ref = fuzz_problem(po, c)
    assert len(h_ref) == 4 and np.all(np.isfinite(u_ref)) and np.any(u_ref != 0) and np.all(h_ref > 0)
    set_knobs(monkeypatch, SELECTIONS[selection])
    _, h, u = run_gpu(pkg, FUZZ[c], b, u0, tol=0.0, max_cycles=3)
    assert_bits(u, h, u_ref, h_ref, (selection, FUZZ[c]))


# ---- b. one-pass depths of the float folded kernels -------------------------------------------------------------
DEPTHS = [(0, k, arith) for k in range(1, 11) for arith in (0, 1)] + [(1, k, 0) for k in range(1, 6)]


@pytest.fixture(scope="module")
def depth_inputs(po):
    b = po.rhs_sine(9).astype(np.float32)
    u0 = po.fill_uniform(b.shape, 909).astype(np.float32)
    b.setflags(write=False)
    u0.setflags(write=False)
    return b, u0


@pytest.mark.parametrize("restrict_mode", [0, 1], ids=["cons", "fw16"])
@pytest.mark.parametrize("smoother,k,arith", DEPTHS,
                         ids=[f"{'gs' if s else 'jac'}{k}-{'fma' if a else 'sep'}" for s, k, a in DEPTHS])
def test_f32_folded_pass_depths_are_bit_equal_to_the_oracle(pkg, po, monkeypatch, depth_inputs, smoother, k, arith,
                                                            restrict_mode):
    """levels 9..7, marching kernels: levels 9 and 8 (512 and 256 columns, the smallest grid the planner folds
    on) run k_jacobi_cycle<float>.  V(k, k): a depth the planner runs in one pass selects K = k; k = 7 and 9
    have no instantiation, k = 8 none for the float pre-smoothing pass with its residual stage, k = 10 in
    SEPARATE mode only for the post-smoothing block - there the planner splits.  Its own plan and one forced
    split (5 + (k - 5) sweeps from k = 6 on) must both give the oracle's bits."""
    b, u0 = depth_inputs
    cfg = dict(finest_level=9, coarsest_level=7, mu1=k, mu2=k, schedule=0, dtype=0, smoother=smoother, arith=arith,
               restrict_mode=restrict_mode, bottom=0)
    u_ref, h_ref = po.Solver(**oracle_cfg(po, cfg)).solve(b, u0, tol=0.0, max_cycles=2)
    assert len(h_ref) == 3 and np.all(np.isfinite(u_ref)) and np.all(h_ref > 0)
    plans = [{"MGX_TILE_MAX_N": "0"}]
    if smoother == 0:
        split = str(k) if k <= 5 else f"5,{k - 5}"
        plans.append({"MGX_TILE_MAX_N": "0", "MGX_PLAN_MIN_N": "256", "MGX_PLAN_PRE": split, "MGX_PLAN_POST": split})
    for env in plans:
        set_knobs(monkeypatch, env)
        _, h, u = run_gpu(pkg, cfg, b, u0, tol=0.0, max_cycles=2)
        assert_bits(u, h, u_ref, h_ref, (cfg, env))


# ---- c. stand-alone schedule entry points -----------------------------------------------------------------------
@pytest.mark.parametrize("tiles", ["tiles", "marching"])
@pytest.mark.parametrize("smoother", [0, 1], ids=["jacobi", "rbgs"])
def test_f32_schedule_entry_points_are_bit_equal_to_the_oracle(pkg, po, monkeypatch, smoother, tiles):
    set_knobs(monkeypatch, {"MGX_TILE_MAX_N": "0"} if tiles == "marching" else {})
    cfg = dict(finest_level=9, coarsest_level=6, mu0=1, mu1=3, mu2=2, dtype=0, smoother=smoother, bottom=0)
    b = po.rhs_sine(9).astype(np.float32)
    u0 = po.fill_uniform(b.shape, 7).astype(np.float32)
    ref = po.Solver(**dict(cfg, bottom=po.BOTTOM_DST))
    n7 = (1 << 7) - 1
    with pkg.Multigrid(**cfg) as mg:
        v = mg.vcyclemultigrid(9, u0, b)                                    # PS:575
        v_ref = ref.vcycle(9, u0, b)
        assert v.dtype == np.float32 and v_ref.dtype == np.float32 and np.any(v_ref != 0)
        assert np.array_equal(v, v_ref)
        # a V-cycle from an intermediate level (PS:617 recursion entry) on the leading 127^2 block
        v7 = mg.vcyclemultigrid(7, u0[:n7, :n7], b[:n7, :n7])
        assert np.array_equal(v7, ref.vcycle(7, u0[:n7, :n7].copy(), b[:n7, :n7].copy()))
        w = mg.fullmultigrid(b)                                             # PS:629
        w_ref = ref.fmg(9, b)
        assert w.dtype == np.float32 and w_ref.dtype == np.float32 and np.any(w_ref != 0)
        assert np.array_equal(w, w_ref)
        # the zero-start cycle: stale data in U that the call must ignore
        mg.set_rhs(b)
        mg.set_guess(u0)
        mg.vcycle_zero()
        assert np.array_equal(mg.get_solution(), ref.vcycle(9, np.zeros_like(b), b))


# ---- d. operator level ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", ["tiles", "marching"])
@pytest.mark.parametrize("arith", [0, 1], ids=["sep", "fma"])
@pytest.mark.parametrize("omega", [0.4, 0.8, 1.0])
def test_f32_jacobi_bits_at_other_omegas_and_both_rounding_modes(pkg, po, monkeypatch, omega, arith, tiles):
    set_knobs(monkeypatch, {"MGX_TILE_MAX_N": "0"} if tiles == "marching" else {})
    with pkg.Multigrid(finest_level=9, coarsest_level=4, dtype=0, omega=omega, arith=arith, bottom=pkg.BOTTOM_SMOOTH) as mg:
        for level in (5, 9):
            n = (1 << level) - 1
            rng = np.random.default_rng(600 + level)
            v = rng.uniform(-1, 1, (n, n)).astype(np.float32)
            f = rng.uniform(-1, 1, (n, n)).astype(np.float32)
            for mu in (1, 4):
                got = mg.jacobirelaxation(level, v, f, mu)
                ref = po.jacobi(v, f, mu, omega, arith=arith)
                assert got.dtype == ref.dtype == np.float32
                assert np.array_equal(got, ref), (level, mu, omega, arith, int(np.count_nonzero(got != ref)))


@pytest.mark.parametrize("tiles", ["tiles", "marching"])
def test_f32_fw16_restrictions_are_bit_equal_to_the_oracle(pkg, po, monkeypatch, tiles):
    set_knobs(monkeypatch, {"MGX_TILE_MAX_N": "0"} if tiles == "marching" else {})
    with pkg.Multigrid(finest_level=9, coarsest_level=4, dtype=0, restrict_mode=pkg.RESTRICT_FW16,
                       bottom=pkg.BOTTOM_SMOOTH) as mg:
        for level in (5, 9):
            n = (1 << level) - 1
            rng = np.random.default_rng(700 + level)
            v = rng.uniform(-1, 1, (n, n)).astype(np.float32)
            f = rng.uniform(-1, 1, (n, n)).astype(np.float32)
            got = mg.restriction2d(level, f)
            ref = po.restrict(f, po.RESTRICT_FW16)
            assert got.dtype == ref.dtype == np.float32 and np.array_equal(got, ref), level
            assert not np.array_equal(ref, po.restrict(f)), level           # the weight really differs
            cb, cu = mg.residual_restriction(level, v, f)
            assert np.array_equal(cb, po.restrict(po.residual(v, f), po.RESTRICT_FW16)), level
            assert np.all(cu == 0)                                          # PS:613
