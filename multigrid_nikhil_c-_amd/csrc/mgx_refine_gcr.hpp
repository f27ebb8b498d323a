// mgx_refine_gcr.hpp - the two passes of mgx_solve_refine_gcr that sit on the precision boundary: restarted GCR in fp64
// (mgx_krylov.hpp's passes on double vectors) around the float cycle of the handle's shadow hierarchy (mgx_refine.hpp).
//
//   k_refine_direction<NQ>   Z_j = z = scale * (double) z32,  Q_j = A z          reads z32 and the NQ grids of A; writes z, q
//   k_refine_update          x += alpha z', r -= alpha q', sum r^2 -> partial[],  r32 = (float)(r * inv_scale_next)
// (k_refine_direction on K = 2 .. 4 columns, for mgx_solve_multi_refine_gcr: mgx_refine_multi.hpp)
//
// Both run in the geometry of k_refine_pass: make_launch(N, 2, N - 1, rows_per_chunk) and lane_cols<2>, one wave marching
// down the R rows of its chunk of a strip, the float grid addressed with its own pitch (epitch >= pitch).
//
// k_refine_direction is k_pcg_direction<double, 1 | 2> on its first iteration with the conversion in front: a rolling
// three-row window of z in registers, the rows above and below the chunk recomputed from z32, ring rows zero without a
// load and column 0 and the padding masked, as prow does there; the x-neighbours from the adjacent lanes, A through
// load_coefs<NQ, 0> and stencil_sum<NQ> - the bits of k_pcg_direction fed the same z.  The scaling by a power of two
// is exact.  It writes no partial sums: GCR does not use z.q (k_gcr_orth forms q'.q' and r.q').
// Algorithmic bytes per point: 4 (z32) + 8 NQ (A) + 8 (z) + 8 (q): 60 on a five-point, 92 on a nine-point level.
//
// k_refine_update is k_pcg_update<double> with one more store, the scaled float residual the NEXT cycle consumes, into
// the shadow's finest right-hand side; inv_scale_next = 1 / pow2_floor(hist[k] / n) is known on the host when iteration
// k is enqueued (the lag of mgx_solve_refine).  After a breakdown nothing is touched.
// Bytes per point: 32 read (x, z', r, q') + 16 (x, r) + 4 (r32) written = 52.
#pragma once

#include "mgx_krylov.hpp"
#include "mgx_refine.hpp"

namespace mgx {

template <int NQ>
__global__ void __launch_bounds__(kBlock)
k_refine_direction(const float* __restrict__ z32, Op9<double> a, double* __restrict__ z, double* __restrict__ q, double scale,
                   int N, long pitch, long epitch, int R, int strips, int chunks)
{
    const Tile t = wave_tile(strips, chunks);
    if (!t.active) return;
    const Cols c = lane_cols<2>(t.strip, N, pitch);
    const int r0 = 1 + t.chunk * R;
    const int r1 = min(r0 + R, N);
    // row y of z at a lane's columns (rows 0 and N are the Dirichlet ring: zero without a load)
    auto zrow = [&](int y) {
        RefineRow w;
        float2 ev = make_float2(0.f, 0.f);
        if (c.ld && y >= 1 && y < N) ev = *reinterpret_cast<const float2*>(z32 + (long)y * epitch + c.col);
        w.v = make_double2(scale * (double)ev.x, scale * (double)ev.y);
        mask_cols(w.v, c.col, N);
        w.l = from_left(w.v.y);
        w.r = from_right(w.v.x);
        return w;
    };
    RefineRow up = zrow(r0 - 1);
    RefineRow cur = zrow(r0);
    for (int y = r0; y < r1; ++y) {
        const RefineRow dn = zrow(y + 1);
        const long at = (long)y * pitch + c.col;
        Lanes<double> k[9];
        load_coefs<NQ, 0>(a, at, c.ld, k);
        const Rows3<double> w{to_lanes(up.v), to_lanes(cur.v), to_lanes(dn.v), up.l, up.r, cur.l, cur.r, dn.l, dn.r};
        double2 o = from_lanes(stencil_sum<NQ>(w, k, [&](int x) { return k[0].a[x]; }));
        mask_cols(o, c.col, N);
        vstore<double2>(z + at, cur.v, c.st);
        vstore<double2>(q + at, o, c.st);
        up = cur; cur = dn;
    }
}

__global__ void __launch_bounds__(kBlock)
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
