"""k_tile_wide against k_tile_smooth on SHORT blocks: mu = 1, 2, 3 levels per launch are the first and last trips of the
kernel's level loop with nothing in between (tests/test_gpu_tile_wide.py runs 10 and 25), so a loop that hands values
from one trip to the next - rows updated around the halo exchange, products kept across levels - is wrong here first.
Levels 7 and 9 (one tile row and several), fp64, every (PRE, POST) stage pair, the whole grid and an interior row
window: the iterate and the restricted coarse residual must be the same bits as the narrow tiles', the norm (a sum over
differently shaped tiles) agrees to 1e-12 relative."""
import numpy as np
import pytest

from test_gpu_tile_wide import STAGES, _slab_cycle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mu", [1, 2, 3])
@pytest.mark.parametrize("smoother", ["jacobi", "jacobi_fma", "rbgs"])
@pytest.mark.parametrize("level", [7, 9])
def test_short_blocks_on_wide_tiles_equal_the_narrow_tiles(pkg, monkeypatch, level, smoother, mu):
    kind = pkg.SMOOTHER_RBGS if smoother == "rbgs" else pkg.SMOOTHER_JACOBI
    arith = 1 if smoother == "jacobi_fma" else 0
    for pre, post in STAGES:
        for window in (False, True):
            args = (pkg, level, np.float64, arith, kind, mu, pre, post, 0, window)
            u0, c0, n0 = _slab_cycle(*args, False, monkeypatch)
            u1, c1, n1 = _slab_cycle(*args, True, monkeypatch)
            what = (pre, post, mu, window)
            assert np.array_equal(u0, u1), what
            assert np.array_equal(c0, c1), what
            assert n1 == pytest.approx(n0, rel=1e-12), what
