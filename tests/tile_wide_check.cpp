// CPU check of the tile map of k_tile_wide (csrc/mgx_geom.hpp, tile_wide_geom): for every level the launcher gives it,
// every band height, element width and halo, on whole grids and row windows, the output tiles cover every unknown
// node of the range exactly once, each output node lies inside its tile's array with at least He nodes of halo on
// every side (the region where all `levels` sweeps are valid), the array's first column and the output columns start
// on whole vectors, and the tile count fits the norm partials' buffer (mgx.hip: ceil(N / 32) x ceil(N / 40) + 8).
// Built and run by tests/test_tile_wide_geom.py.
#include "mgx_geom.hpp"
#include <cstdio>
#include <vector>
using namespace mgx;
int main()
{
    int fails = 0, cases = 0;
    for (int L = 7; L <= 11; ++L)
        for (int W : {2, 4})
            for (int RW : {8, 10})
                for (int He = 1; He <= 12; ++He)
                    for (int win = 0; win < 3; ++win) {
                        const int N = 1 << L;
                        const int row_lo = win == 0 ? 1 : (win == 1 ? N / 4 + 1 : N / 2 - 3);
                        const int row_hi = win == 0 ? N : (win == 1 ? N / 2 + 1 : N / 2 + 5);
                        const TileWideGeom g = tile_wide_geom(N, row_lo, row_hi, He, W, RW);
                        ++cases;
                        auto fail = [&](const char* what) {
                            if (fails++ < 20) printf("FAIL %s: N %d W %d RW %d He %d rows [%d, %d)\n", what, N, W, RW, He, row_lo, row_hi);
                        };
                        if (g.TH < 8 || g.TW < 8) { fail("tile too small"); continue; }
                        if (g.Hx < He || g.Hx % W || g.TW % W) fail("columns not on whole vectors");
                        if (g.TH < 32 || g.TW < 40) fail("tile smaller than the partial buffer assumes");
                        if ((long)g.tiles_y * g.tiles_x > (long)((N + 31) / 32) * ((N + 39) / 40)) fail("more tiles than partials");
                        std::vector<int> hits((size_t)(N + 1) * (N + 1), 0);
                        const int SY = kTileWideWaves * RW, SX = 64 * W;
                        for (int ty = 0; ty < g.tiles_y; ++ty)
                            for (int tx = 0; tx < g.tiles_x; ++tx) {
                                const int gy_a = row_lo + ty * g.TH - He, gx_a = tx * g.TW - g.Hx;   // array row / column 0
                                if (gx_a % W) fail("array column 0 not on a vector boundary");
                                for (int y = 0; y < SY; ++y)
                                    for (int x = 0; x < SX; ++x) {
                                        const int gy = gy_a + y, gx = gx_a + x;
                                        // the kernel's store rule: output rows [He, He + TH) in the range, output columns
                                        // [tx TW, tx TW + TW) below N (column 0 holds the boundary: not an unknown)
                                        const bool out = y >= He && y < He + g.TH && gy >= row_lo && gy < row_hi && gy < N &&
                                                         gx >= tx * g.TW && gx < tx * g.TW + g.TW && gx < N && gx >= 1;
                                        if (!out) continue;
                                        if (y < He || y >= SY - He || x < He || x >= SX - He) fail("output node within He of the array edge");
                                        ++hits[(size_t)gy * (N + 1) + gx];
                                    }
                            }
                        for (int y = row_lo; y < row_hi; ++y)
                            for (int x = 1; x < N; ++x)
                                if (hits[(size_t)y * (N + 1) + x] != 1) { fail("node not covered exactly once"); y = row_hi; break; }
                    }
    printf("%d cases, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
