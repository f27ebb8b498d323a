// mgx_refine.hpp - the fp64 pass of mgx_solve_refine (iterative refinement of a general-operator handle around the
// float cycle of its shadow hierarchy) and the grid conversion that gives the shadow its operator.
//
//   k_refine_pass<NQ, HAS_E>   u' = u + scale * (double) e,  r = b - A u',  sum r^2 -> partial[],
//                              r32 = (float)(r * inv_scale)
//   k_grid_f64_to_f32          a whole level grid (ring and padding included) rounded to float
//
// k_refine_pass is the general-operator counterpart of k_update_residual (mgx_kernels.hpp): a wave marches down the R
// rows of its chunk of a strip with a rolling three-row window of the UPDATED iterate in registers; the rows above and
// below the chunk are recomputed from u and e, not communicated, so the pass is out of place (u -> unew: an in-place
// update would race with the neighbouring chunk's reads of its edge rows).  The x-neighbours come from the adjacent
// lanes (from_left / from_right; NQ = 5: of the current row only), the NQ coefficient grids are streamed (load_coefs)
// and the residual is k_residual_var<double, NQ>'s expression: b - stencil_sum<NQ>() in CSR order, every product and
// sum rounded on its own, the ring, column 0 and the padding masked to zero - the same bits.  The sums of squares go
// per block, in a fixed order, into partial[] (k_reduce_partials adds them): no atomics, no LDS beyond that reduction.
// HAS_E = false: no correction (e is not read, unew is not written): the scaled residual of the iterate as it stands.
//
// Algorithmic bytes per point: 8 (u) + 4 (e) + 8 (b) + 8 NQ (A) + 8 (u') + 4 (r32): 72 on a five-point, 104 on a
// nine-point level (a chunk of R rows also re-reads two rows of u and e: L2 hits, see make_launch).
// The float grids have their own pitch (epitch >= pitch: level_pitch), so a lane's columns exist in both.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

// a row of the updated iterate at a lane's columns, with the elements left of its first and right of its last column
struct RefineRow { double2 v; double l, r; };

template <int NQ, bool HAS_E>
__global__ void __launch_bounds__(kBlock)
k_refine_pass(const double* __restrict__ u, const float* __restrict__ e, const double* __restrict__ rhs, Op9<double> a,
              double* __restrict__ unew, float* __restrict__ r32, double scale, double inv_scale,
              double* __restrict__ partial, int N, long pitch, long epitch, int row_lo, int row_hi, int R, int strips,
              int chunks)
{
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc = 0.0;
    if (t.active) {
        const Cols c = lane_cols<2>(t.strip, N, pitch);
        const int r0 = row_lo + t.chunk * R;
        const int r1 = min(r0 + R, row_hi);
        // updated row r (rows 0 and N, column 0 and the padding hold zeros in u and e and stay zero)
        auto updated = [&](int r) {
            RefineRow w;
            w.v = vload<double2>(u + (long)r * pitch + c.col, c.ld);
            if constexpr (HAS_E) {
                float2 ev = make_float2(0.f, 0.f);
                if (c.ld) ev = *reinterpret_cast<const float2*>(e + (long)r * epitch + c.col);
                w.v.x = w.v.x + scale * (double)ev.x;
                w.v.y = w.v.y + scale * (double)ev.y;
                if (c.col == 0) w.v.x = 0.0;
            }
            w.l = from_left(w.v.y);
            w.r = from_right(w.v.x);
            return w;
        };
        RefineRow up = updated(r0 - 1);
        RefineRow cur = updated(r0);
        for (int r = r0; r < r1; ++r) {
            const RefineRow dn = updated(r + 1);
            const long at = (long)r * pitch + c.col;
            const Lanes<double> b = load_lanes(rhs + at, c.ld);
            Lanes<double> k[9];
            load_coefs<NQ, 0>(a, at, c.ld, k);
            const Rows3<double> w{to_lanes(up.v), to_lanes(cur.v), to_lanes(dn.v), up.l, up.r, cur.l, cur.r, dn.l, dn.r};
            const Lanes<double> av = stencil_sum<NQ>(w, k, [&](int x) { return k[0].a[x]; });
            double2 o = make_double2(b.a[0] - av.a[0], b.a[1] - av.a[1]);
            mask_cols(o, c.col, N);
            if (c.st) {
                if constexpr (HAS_E) *reinterpret_cast<double2*>(unew + at) = cur.v;
                acc += o.x * o.x + o.y * o.y;
                *reinterpret_cast<float2*>(r32 + (long)r * epitch + c.col) = make_float2((float)(o.x * inv_scale), (float)(o.y * inv_scale));
            }
            up = cur; cur = dn;
        }
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// out = (float) in over rows 0 .. rows - 1 and columns 0 .. pitch_in - 1 of a level grid (pitch_out >= pitch_in; the
// columns beyond stay as allocated: zero)
static __global__ void k_grid_f64_to_f32(const double* __restrict__ in, float* __restrict__ out, long pitch_in, long pitch_out)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long r = blockIdx.y;
    if (c >= pitch_in) return;
    out[r * pitch_out + c] = (float)in[r * pitch_in + c];
}

// the launch of k_refine_pass on rows 1 .. N - 1 of a level: geometry from make_launch, with fewer, taller chunks when
// the partial-sum buffer is smaller than the launch (the rule of the MIXED solve's pass).  Returns the number of
// partial sums written, for k_reduce_partials
template <int NQ, bool HAS_E>
int launch_refine_pass(const double* u, const float* e, const double* rhs, const Op9<double>& a, double* unew, float* r32,
                       double scale, double inv_scale, double* partial, long partial_cap, int N, long pitch, long epitch,
                       int rpc, hipStream_t st)
{
    Launch g = make_launch(N, 2, N - 1, rpc);
    if (g.blocks > partial_cap) {
        const int R = (int)(((long)g.strips * (N - 1) / kWavesPerBlock + partial_cap - 9) / (partial_cap - 8)) + 1;
        g = make_launch(N, 2, N - 1, R);
    }
    hipLaunchKernelGGL((k_refine_pass<NQ, HAS_E>), dim3(g.blocks), dim3(kBlock), 0, st, u, e, rhs, a, unew, r32, scale, inv_scale,
                       partial, N, pitch, epitch, 1, N, g.R, g.strips, g.chunks);
    return g.blocks;
}

} // namespace mgx
