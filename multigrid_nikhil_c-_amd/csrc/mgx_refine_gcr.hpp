// mgx_refine_gcr.hpp - the two passes of mgx_solve_refine_gcr that sit on the precision boundary: restarted GCR in fp64
// (mgx_krylov.hpp's passes on double vectors) around the float cycle of the handle's shadow hierarchy (mgx_refine.hpp).
//
//   k_refine_direction<NQ, K>  Z_j = z = scale * (double) z32,  Q_j = A z        reads z32 and the NQ grids of A; writes z, q
//   k_refine_update            x += alpha z', r -= alpha q', sum r^2 -> partial[],  r32 = (float)(r * inv_scale_next)
// k_refine_direction runs on K = 1 .. 4 columns per operator read (mgx_var.hpp, COLUMNS): K = 1 is mgx_solve_refine_gcr's
// pass, K = |active set| that of mgx_solve_multi_refine_gcr, which adds no kernel of its own - its float
// block cycle is mgx_solve_multi's on the shadow hierarchy, its orthogonalisation, mixed update and reductions are the
// passes here and in mgx_krylov.hpp on each column's view.
//
// Both run in the geometry of k_refine_pass: make_launch(N, 2, N - 1, rows_per_chunk) and lane_cols<2>, one wave marching
// down the R rows of its chunk of a strip, the float grid addressed with its own pitch (epitch >= pitch).
//
// k_refine_direction is k_pcg_direction<double, 1 | 2> on its first iteration with the conversion in front: a rolling
// three-row window of z in registers, the rows above and below the chunk recomputed from z32, ring rows zero without a
// load and column 0 and the padding masked, as prow does there; the x-neighbours from the adjacent lanes, A through
// load_coefs<NQ, 0> and stencil_sum<NQ> - the bits of k_pcg_direction fed the same z.  The scaling by a power of two
// is exact.  It writes no partial sums: GCR does not use z.q (k_gcr_orth forms q'.q' and r.q').
// Algorithmic bytes per point: 4 (z32) + 8 NQ (A) + 8 (z) + 8 (q): 60 on a five-point, 92 on a nine-point level; on K
// columns 8 NQ + 20 K against K (8 NQ + 20) - five-point, K = 4: 120 against 240; nine-point: 152 against 368.
// Per row all K columns' loads of row y + 1 are issued first, then the coefficients once, then the K sums; nothing is
// stored before every result of the row exists (the output pointers carry no __restrict__), and the stores of row y
// come before the loads of row y + 1's coefficients.  The column pointers and scales arrive by value and are indexed by
// unrolled constants only.  A wave without a tile returns at once (nothing below synchronises the workgroup).
//
// k_refine_update is k_pcg_update<double> with one more store, the scaled float residual the NEXT cycle consumes, into
// the shadow's finest right-hand side; inv_scale_next = 1 / pow2_floor(hist[k] / n) is known on the host when iteration
// k is enqueued (the lag of mgx_solve_refine).  After a breakdown nothing is touched.
// Bytes per point: 32 read (x, z', r, q') + 16 (x, r) + 4 (r32) written = 52.
#pragma once

#include "mgx_krylov.hpp"
#include "mgx_refine.hpp"

namespace mgx {

template <int K> struct RefineScales { double s[K]; };

template <int NQ, int K>
__global__ void __launch_bounds__(kBlock)
k_refine_direction(MultiIn<float, K> z32, Op9<double> a, MultiOut<double, K> z, MultiOut<double, K> q, RefineScales<K> scale,
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

// one launch of k_refine_direction on m = 1 .. kMultiMax columns (host arrays of m pointers and scales) of a five- or
// nine-point level.  mgx.hip calls it; mgx_inst.hip (-DMGX_INST_KIND=10) defines it
void launch_refine_direction(int m, bool nine, const float* const* z32, double* const* z, double* const* q, const double* scale,
                             const Op9<double>& a, int N, long pitch, long epitch, const Launch& g, hipStream_t st);

#if (defined(MGX_INST_KIND) && MGX_INST_KIND == 10) || defined(MGX_SINGLE_TU)
void launch_refine_direction(int m, bool nine, const float* const* z32, double* const* z, double* const* q, const double* scale,
                             const Op9<double>& a, int N, long pitch, long epitch, const Launch& g, hipStream_t st)
{
    with_point_count(nine, [&](auto nq) {
        with_count<kMultiMax>(m, [&](auto kc) {
            constexpr int NQ = decltype(nq)::value, K = decltype(kc)::value;
            RefineScales<K> sc;
            for (int j = 0; j < K; ++j) sc.s[j] = scale[j];
            hipLaunchKernelGGL((k_refine_direction<NQ, K>), dim3(g.blocks), dim3(kBlock), 0, st, columns_in<K>(z32), a, columns_out<K>(z),
                               columns_out<K>(q), sc, N, pitch, epitch, g.R, g.strips, g.chunks);
        });
    });
}
#endif

// (static: mgx.hip and the compilation of launch_refine_direction both include this header; only mgx.hip launches it)
static __global__ void __launch_bounds__(kBlock)
k_refine_update(double* __restrict__ x, const double* __restrict__ p, double* __restrict__ r, const double* __restrict__ q,
                float* __restrict__ r32, double inv_scale_next, const double* __restrict__ sc, double* __restrict__ partial,
                int N, long pitch, long epitch, int R, int strips, int chunks)
{
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc = 0.0;
    if (t.active && sc[kPcgBreak] == 0.0) {
        const double alpha = sc[kPcgAlpha];
        const Cols c = lane_cols<2>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                const double2 xx = vaxpy(vload<double2>(x + at, true), alpha, vload<double2>(p + at, true));
                const double2 rr = vaxmy(vload<double2>(r + at, true), alpha, vload<double2>(q + at, true));
                vstore<double2>(x + at, xx, true);
                vstore<double2>(r + at, rr, true);
                *reinterpret_cast<float2*>(r32 + (long)y * epitch + c.col) =
                    make_float2((float)(rr.x * inv_scale_next), (float)(rr.y * inv_scale_next));
                acc += vdot(rr, rr);
            }
        }
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

} // namespace mgx
