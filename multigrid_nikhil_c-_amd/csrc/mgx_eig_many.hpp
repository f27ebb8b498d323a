// mgx_eig_many.hpp - the kernels of mgx_eigs_many (absent in the reference): up to MGX_EIGS_MAX smallest eigenpairs by
// mgx_eigs' LOBPCG (mgx_eig.hpp) on blocks of at most MGX_MAX_RHS columns, each block iterating in the complement of the
// pairs already found (deflation by locking).  The driver is mgx_eig_many_host.hpp, its bookkeeping mgx_eig_many_plan.hpp.
//
// THE ITERATION (Y: the locked vectors, device resident, orthonormal):
//     Y = {}
//     while |Y| < nev:
//         kb = min(MGX_MAX_RHS, nev - |Y|);  X = the caller's guesses |Y| .. |Y| + kb - 1
//         X <- X - Y (Y^T X), twice               (once per block; skipped when Y is empty)
//         mgx_eigs' iteration on X (mgx_eig.hpp, THE ITERATION), with one change: after W_act = M R_act,
//             W_act <- W_act - Y (Y^T W_act)      (once per iteration; skipped when Y is empty)
//         the block ends as mgx_eigs ends: every column meets hist <= tol theta, or after max_iters iterations, or on
//         its failures
//         if it did not end converged: stop.   else Y <- [Y, X]
//     sort the computed pairs by lambda ascending (stable); vectors, stats and history slots follow
// Everything else of the block iteration is mgx_eigs' own (eig_block in mgx_eig_host.hpp): soft locking inside the block,
// A X and A P applied afresh, the Rayleigh-Ritz pencil of at most 12 columns on the host, the restart without P, two host
// synchronisations per iteration.  The projection adds none: its coefficients stay on the device.
//
// THE PROJECTION  V <- V - Y (Y^T V)  of k <= MGX_MAX_RHS columns V against m locked vectors:
//     dots      c_ij = Y_i . V_j in double, with lane_dot, eig_block_reduce and k_eig_reduce_rows in their fixed order; all
//               dots come from the unmodified V (classical Gram-Schmidt);
//     subtract  V_j = ((V_j - c_0j Y_0) - c_1j Y_1) - ... with i ascending over all m locked vectors; each c_ij is read
//               from device memory and rounded to T once, every product and every difference is rounded in T.
//
// THE KERNELS use the layout, strips and lanes of mgx_eig.hpp; column pointers come by value and are indexed by unrolled
// constants only; none uses scratch.
//   k_eig_project_dots<T, KY, KW>  the KY x KW sums of a chunk of KY locked vectors against the KW columns, the rows marched as
//                                  k_eig_gram marches them.  Every vector of the chunk is read once, V once per chunk: the
//                                  driver cuts the m locked vectors into chunks of kEigChunk = 8 (32 accumulators, as
//                                  k_eig_gram<T, 4, 4>), so m <= 15 takes at most two launches and m + 2 k vector reads.
//   k_eig_project_sub<T, KW>       one launch for all m locked vectors: the Y_i pointers come from a device table, the c_ij
//                                  are wave-uniform loads, the KW columns are accumulated in registers: m + KW vectors read,
//                                  KW written.  All loads of a row come before its stores (V is updated in place).
#pragma once

#include "mgx_eig.hpp"

namespace mgx {

constexpr int kEigChunk = 8;                    // locked vectors per launch of k_eig_project_dots
constexpr int kEigManyMax = 16;                 // MGX_EIGS_MAX

// partial[(i * KW + j) * stride + block] = the block's sum of y_i . w_j; halo lanes and the columns that are not
// unknowns contribute zero
template <typename T, int KY, int KW>
__global__ void __launch_bounds__(kBlock)
k_eig_project_dots(MultiIn<T, KY> y, MultiIn<T, KW> w, double* __restrict__ partial, int stride, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    __shared__ double wsum[KY * KW][kWavesPerBlock];
    double acc[KY * KW];
#pragma unroll
    for (int e = 0; e < KY * KW; ++e) acc[e] = 0.0;
    const Tile t = wave_tile(strips, chunks);
    const Cols c = lane_cols<VecOf<T>::W>(t.strip, N, pitch);
    if (t.active) {
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        const bool ld = c.ld && c.st;
        for (int row = r0; row < r1; ++row) {
            const long at = c.col + (long)row * pitch;
            Lanes<T> a[KY], b[KW];
#pragma unroll
            for (int i = 0; i < KY; ++i) {
                V v = vload<V>(y.p[i] + at, ld);
                mask_cols(v, c.col, N);
                a[i] = to_lanes(v);
            }
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                V v = vload<V>(w.p[j] + at, ld);
                mask_cols(v, c.col, N);
                b[j] = to_lanes(v);
            }
#pragma unroll
            for (int i = 0; i < KY; ++i)
#pragma unroll
                for (int j = 0; j < KW; ++j) acc[i * KW + j] += lane_dot(a[i], b[j]);
        }
    }
    eig_block_reduce<KY * KW>(acc, wsum, partial, stride);
}

// w_j <- ((w_j - c[0 * KW + j] y_0) - c[1 * KW + j] y_1) - ... over the m vectors of the device table ytab
template <typename T, int KW>
__global__ void __launch_bounds__(kBlock)
k_eig_project_sub(const T* const* __restrict__ ytab, int m, MultiOut<T, KW> w, const double* __restrict__ coef, int N, long pitch, int R, int strips,
                  int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const Tile t = wave_tile(strips, chunks);
    if (!t.active) return;
    const Cols c = lane_cols<W>(t.strip, N, pitch);
    const int r0 = 1 + t.chunk * R;
    const int r1 = min(r0 + R, N);
    const bool ld = c.ld && c.st;
    for (int row = r0; row < r1; ++row) {
        const long at = c.col + (long)row * pitch;
        Lanes<T> s[KW];
#pragma unroll
        for (int j = 0; j < KW; ++j) s[j] = to_lanes(vload<V>(w.p[j] + at, ld));
        // four locked vectors in flight per lane: the loads of a group are independent of its subtractions
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const Lanes<T> v = to_lanes(vload<V>(ytab[i] + at, ld));
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                const T cij = (T)coef[i * KW + j];
#pragma unroll
                for (int x = 0; x < W; ++x) s[j].a[x] = s[j].a[x] - cij * v.a[x];
            }
        }
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            V o = from_lanes(s[j]);
            mask_cols(o, c.col, N);
            vstore<V>(w.p[j] + at, o, c.st);
        }
    }
}

// ---- launches (the geometry is EigGeom::g, a Krylov pass's) ------------------------------------------------------------------
// coef[i * kw + j] = y_i . w_j for i < m <= kEigManyMax - 1, j < kw <= kMultiMax: one launch and one reduction per chunk of
// kEigChunk vectors.  partial holds kEigChunk * kMultiMax * g.blocks doubles and is reused by the chunks (one stream)
template <typename T>
void launch_eig_project_dots(int m, int kw, const T* const* y, const T* const* w, double* partial, double* coef, const EigGeom& e, hipStream_t st)
{
    const Launch& g = e.g;
    for (int i0 = 0; i0 < m; i0 += kEigChunk) {
        const int ky = m - i0 < kEigChunk ? m - i0 : kEigChunk;
        with_count<kEigChunk>(ky, [&](auto ty) {
            constexpr int KY = decltype(ty)::value;
            with_count<kMultiMax>(kw, [&](auto tw) {
                constexpr int KW = decltype(tw)::value;
                hipLaunchKernelGGL((k_eig_project_dots<T, KY, KW>), dim3(g.blocks), dim3(kBlock), 0, st, columns_in<KY>(y + i0), columns_in<KW>(w), partial,
                                   g.blocks, e.N, e.pitch, g.R, g.strips, g.chunks);
            });
        });
        hipLaunchKernelGGL(k_eig_reduce_rows, dim3(ky * kw), dim3(kReduceThreads), 0, st, partial, g.blocks, g.blocks, coef + i0 * kw);
    }
}

// w_j <- w_j - sum_i coef[i * kw + j] y_i in the order stated above; ytab: the device table of the m pointers
template <typename T>
void launch_eig_project_sub(int m, int kw, const T* const* ytab, T* const* w, const double* coef, const EigGeom& e, hipStream_t st)
{
    const Launch& g = e.g;
    with_count<kMultiMax>(kw, [&](auto tw) {
        constexpr int KW = decltype(tw)::value;
        hipLaunchKernelGGL((k_eig_project_sub<T, KW>), dim3(g.blocks), dim3(kBlock), 0, st, ytab, m, columns_out<KW>(w), coef, e.N, e.pitch, g.R, g.strips,
                           g.chunks);
    });
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=12) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
#define MGX_EIG_MANY_EXTERN(T)                                                                                                              \
    extern template void launch_eig_project_dots<T>(int, int, const T* const*, const T* const*, double*, double*, const EigGeom&, hipStream_t); \
    extern template void launch_eig_project_sub<T>(int, int, const T* const*, T* const*, const double*, const EigGeom&, hipStream_t);
MGX_EIG_MANY_EXTERN(double)
MGX_EIG_MANY_EXTERN(float)
#undef MGX_EIG_MANY_EXTERN
#endif

} // namespace mgx
