"""The exact coarsest-level solve (csrc/mgx_bottom.hpp: two launches of k_dst_pair) against the oracle's sine-transform
mode ORC_BOTTOM_DST, which performs the same four products in the same order - every sum over k = 0 .. n-1 with one
accumulator, each product rounded before it is added, in double whatever the level's type.  The header of
mgx_bottom.hpp claims the same bits; this file holds it to that: np.array_equal at every batch shape of the kernel
(n = 3, 7: less than one batch of 32 rows; 31: one short of a batch; 63, 127: whole batches and a tail, one wave pair;
255: the full workgroup), in f64 and f32, for a random right-hand side and for one that is zero except for its four
corners and its last row (sums whose first terms are all zero, and the rows a batch's tail must not skip or repeat).
Then two V(2,2) cycles through the solve on levels 8..7 against the oracle's history."""
import numpy as np
import pytest

from test_gpu_solve import hist_close, oracle_cfg, run_gpu

pytestmark = pytest.mark.gpu

LEVELS = [2, 3, 5, 6, 7, 8]
DT = {"f64": (np.float64, 1), "f32": (np.float32, 0)}


def _rhs(kind, n, level):
    if kind == "random":
        return np.random.default_rng(900 + level).uniform(-1, 1, (n, n))
    f = np.zeros((n, n))
    f[0, 0], f[0, -1], f[-1, 0] = 1.0, -2.0, 3.0
    f[-1, :] = np.random.default_rng(950 + level).uniform(-1, 1, n)
    f[-1, -1] = -4.0
    return f


@pytest.fixture(scope="module")
def oracle_solutions(po):
    """ORC_BOTTOM_DST on every (level, dtype, rhs) of this file, computed once"""
    out = {}
    for level in LEVELS:
        n = (1 << level) - 1
        s = po.Solver(finest_level=level, coarsest_level=level, bottom=po.BOTTOM_DST)
        for name, (dt, _) in DT.items():
            for kind in ("random", "corners"):
                f = _rhs(kind, n, level).astype(dt)             # the float input is rounded to float first
                out[(level, name, kind)] = (f, s.bottom_solve(f.astype(np.float64)).astype(dt))
    return out


@pytest.mark.parametrize("kind", ["random", "corners"])
@pytest.mark.parametrize("name", ["f64", "f32"])
@pytest.mark.parametrize("level", LEVELS)
def test_bottom_solve_has_the_bits_of_the_oracles_sine_transform(pkg, oracle_solutions, level, name, kind):
    f, ref = oracle_solutions[(level, name, kind)]
    with pkg.Multigrid(finest_level=level, coarsest_level=level, dtype=DT[name][1]) as mg:
        x = mg.bottom_solve(f)
    assert x.dtype == ref.dtype and x.shape == ref.shape
    bad = np.argwhere(x != ref)
    print(f"level {level} {name} {kind}: {len(bad)} of {x.size} entries differ, max |x - ref| = {np.max(np.abs(x - ref)):.3e}")
    assert np.array_equal(x, ref), (level, name, kind, bad[:4])


@pytest.mark.parametrize("name", ["f64", "f32"])
def test_two_cycles_through_the_bottom_solve_against_the_oracle(pkg, po, name):
    cfg = dict(finest_level=8, coarsest_level=7, mu1=2, mu2=2, schedule=0, dtype=DT[name][1])
    b = po.rhs_sine(8)
    u0 = po.fill_uniform((255, 255), 12345)
    _, h, _ = run_gpu(pkg, cfg, b, u0, tol=0.0, max_cycles=2)
    _, h_ref = po.Solver(**oracle_cfg(po, cfg)).solve(b, u0, tol=0.0, max_cycles=2)
    print(f"{name}: history {h} oracle {h_ref}")
    assert hist_close(h, h_ref), (h, h_ref)
