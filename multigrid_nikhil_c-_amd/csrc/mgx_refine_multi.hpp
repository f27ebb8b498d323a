// mgx_refine_multi.hpp - the one kernel mgx_solve_multi_refine_gcr adds: the direction pass of
// mgx_solve_refine_gcr (k_refine_direction, mgx_refine_gcr.hpp) on K = 2, 3 or 4 columns per operator read.  Every other
// pass of that solve is an existing kernel: the float block cycle is mgx_multi.hpp's on the shadow hierarchy, the
// orthogonalisation, the mixed update and the reductions are the single-column ones on each column's view.
//
// k_refine_direction_multi<NQ, K>: k_refine_direction on K columns with the loading discipline of k_gcr_direction_multi (mgx_multi.hpp):
// Z_j = z_j = scale_j * (double) z32_j, Q_j = A z_j, the NQ grids of A loaded once per row for the K columns:
// 8 NQ + 20 K bytes per point against K (8 NQ + 20) - five-point, K = 4: 120 against 240; nine-point: 152 against 368.
// The same geometry, the same zrow (conversion, scaling, mask_cols, the two edge values from the adjacent lanes), the
// same Rows3, stencil_sum<NQ> with the same centre lambda and mask_cols before the stores: per column the arithmetic
// and its order are k_refine_direction's, so its bits, whatever R is and however the columns are grouped.
// Per row all K columns' loads of row y + 1 are issued first, then the coefficients once, then the K sums; nothing is
// stored before every result of the row exists (the output pointers carry no __restrict__).  The column pointers and
// scales arrive by value and are indexed by unrolled constants only.  No partial sums; a wave without a tile returns
// at once (nothing below synchronises the workgroup).
#pragma once

#include "mgx_refine.hpp"
#include "mgx_multi.hpp"

namespace mgx {

template <int K> struct RefineScales { double s[K]; };

template <int NQ, int K>
__global__ void __launch_bounds__(kBlock)
k_refine_direction_multi(MultiIn<float, K> z32, Op9<double> a, MultiOut<double, K> z, MultiOut<double, K> q, RefineScales<K> scale,
                         int N, long pitch, long epitch, int R, int strips, int chunks)
{
    const Tile t = wave_tile(strips, chunks);
    if (!t.active) return;
    const Cols c = lane_cols<2>(t.strip, N, pitch);
    const int r0 = 1 + t.chunk * R;
    const int r1 = min(r0 + R, N);
    // row y of z_j at a lane's columns (rows 0 and N are the Dirichlet ring: zero without a load)
    auto zrow = [&](const float* zp, double sj, int y) {
        RefineRow w;
        float2 ev = make_float2(0.f, 0.f);
        if (c.ld && y >= 1 && y < N) ev = *reinterpret_cast<const float2*>(zp + (long)y * epitch + c.col);
        w.v = make_double2(sj * (double)ev.x, sj * (double)ev.y);
        mask_cols(w.v, c.col, N);
        w.l = from_left(w.v.y);
        w.r = from_right(w.v.x);
        return w;
    };
    RefineRow up[K], cur[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { up[j] = zrow(z32.p[j], scale.s[j], r0 - 1); cur[j] = zrow(z32.p[j], scale.s[j], r0); }
    for (int y = r0; y < r1; ++y) {
        const long at = (long)y * pitch + c.col;
        RefineRow dn[K];
#pragma unroll
        for (int j = 0; j < K; ++j) dn[j] = zrow(z32.p[j], scale.s[j], y + 1);
        Lanes<double> k[9];
        load_coefs<NQ, 0>(a, at, c.ld, k);
        double2 o[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const Rows3<double> w{to_lanes(up[j].v), to_lanes(cur[j].v), to_lanes(dn[j].v), up[j].l, up[j].r, cur[j].l, cur[j].r, dn[j].l, dn[j].r};
            o[j] = from_lanes(stencil_sum<NQ>(w, k, [&](int x) { return k[0].a[x]; }));
            mask_cols(o[j], c.col, N);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            vstore<double2>(z.p[j] + at, cur[j].v, c.st);
            vstore<double2>(q.p[j] + at, o[j], c.st);
            up[j] = cur[j]; cur[j] = dn[j];
        }
    }
}

// one launch of k_refine_direction_multi on m = 2 .. 4 columns (host arrays of m pointers and scales) of a five- or
// nine-point level.  mgx.hip calls it; mgx_inst.hip (-DMGX_INST_KIND=10) defines it
void launch_refine_direction_multi(int m, bool nine, const float* const* z32, double* const* z, double* const* q, const double* scale,
                                   const Op9<double>& a, int N, long pitch, long epitch, const Launch& g, hipStream_t st);

#if (defined(MGX_INST_KIND) && MGX_INST_KIND == 10) || defined(MGX_SINGLE_TU)
void launch_refine_direction_multi(int m, bool nine, const float* const* z32, double* const* z, double* const* q, const double* scale,
                                   const Op9<double>& a, int N, long pitch, long epitch, const Launch& g, hipStream_t st)
{
    with_point_count(nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        with_column_count(m, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            MultiIn<float, K> zi;
            MultiOut<double, K> zz, qq;
            RefineScales<K> sc;
            for (int j = 0; j < K; ++j) { zi.p[j] = z32[j]; zz.p[j] = z[j]; qq.p[j] = q[j]; sc.s[j] = scale[j]; }
            hipLaunchKernelGGL((k_refine_direction_multi<NQ, K>), dim3(g.blocks), dim3(kBlock), 0, st, zi, a, zz, qq, sc, N, pitch, epitch, g.R,
                               g.strips, g.chunks);
        });
    });
}
#endif

} // namespace mgx
