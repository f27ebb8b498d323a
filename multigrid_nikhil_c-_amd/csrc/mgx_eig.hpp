// mgx_eig.hpp - the kernels of mgx_eigs (absent in the reference): the nev <= MGX_MAX_RHS smallest eigenpairs of the
// finest-level operator A of a general-operator handle by LOBPCG, preconditioned by mgx_solve_multi's block cycle
// (mgx_multi.hpp, mgx_multi_host.hpp).  The driver is mgx_eig_host.hpp, the small dense problem mgx_eig_dense.hpp.
//
// THE ITERATION (X, AX, P, AP: nev vectors each; W, AW: one per active column; theta: nev Ritz values):
//     X <- guesses;  AX = A X;  (theta, C) = RR([X], [AX]);  X <- X C;  AX <- A X;  P = none
//     for k = 0 .. :
//         R_j = AX_j - theta_j X_j;  hist_j[k] = ||R_j||                  (all columns, every iteration)
//         act = { j : not hist_j[k] <= tol theta_j };  stop if act is empty or k = max_iters
//         W_act = M R_act      (mgx_solve_multi's cycle from zero on the columns of act, R as the finest right-hand side)
//         AW = A W
//         S = [X, W_act, P], AS = [AX, AW, AP]   (P absent in iteration 0 and after a restart; at most 3 nev columns)
//         (theta, C) = RR(S, AS)
//         P <- S C with the X rows of C zeroed;  X <- S C;  AX <- A X and AP <- A P (both applied afresh)
// RR(S, AS): G = S^T S and H = S^T A S on the device (k_eig_gram), the pencil on the host (mgx_eig_dense.hpp).  A
// deficient pivot repeats the step once without P (a restart, from the sums already on the host); if it is still
// deficient the call ends with the reason in mgx_last_error.
// SOFT LOCKING: a column whose residual meets the tolerance gets no cycle and no column of W, but it stays in X, is
// still rewritten by every Ritz rotation and returns to `act` if its residual rises above the tolerance again - not the
// "frozen for good" rule of the block solvers.
// AX is recomputed from X in every iteration, so the residuals reported are those of the returned pair, not of a
// recurrence.  AP is recomputed from P as well: the recurrence AP <- AS C (the same traffic: 8 in and 4 out against NQ + 8)
// loses the small P_j of locked columns to the absolute error it carries along, after which their residuals rise by a
// factor of ten per iteration (profiles/eig_kernel_trace_summary.md has the trace).
// Every sum runs in a fixed order without atomics: the call is deterministic.  Two host synchronisations per iteration:
// the residual norms, the Gram sums.
//
// THE KERNELS.  W is the finest u of the workspace column (where the cycle leaves it), R its finest b; X, AX, AW, P and
// AP are the call's own five vectors per column.  All use the layout, strips and lanes of mgx_var.hpp / mgx_multi.hpp;
// column pointers come by value (MultiIn / MultiOut) and are indexed by unrolled constants only; none uses scratch.
//   k_eig_gram<T, KL, KC, DIAG>   the KL x 2 KC inner products of a left block with a right block [B, A B] of KC columns
//                                 each, in double; DIAG: B is the left block itself (KC = KL) and is not read again.
//                                 Every vector is read once per launch.  The driver launches the upper block triangle
//                                 of {X, W, P}: (X,X) (X,W) (X,P) (W,W) (W,P) (P,P).  X^T X and X^T A X are COMPUTED,
//                                 not taken as I and Theta.  Vector reads per iteration, four columns with P:
//                                 3 diagonal pairs of 8 + 3 off-diagonal pairs of 12 = 60 (52 if (X,X) were skipped).
//   k_eig_combine<T, KI, KO>      out_j = sum_i c_ij in_i, KI <= 12, KO <= 4; the coefficients are doubles in the
//                                 kernel arguments (no copy to the device), rounded to T once; each product is rounded
//                                 in T and the sum runs in T over i ascending from the first product.  Every input is
//                                 read once; outputs may alias inputs (all inputs of a lane are loaded before its
//                                 first store; no __restrict__).  X (12 in, 4 out) and P (8 in, 4 out).
//   k_eig_residual<T, K>          R_j = AX_j - theta_j X_j (theta rounded to T) into the finest right-hand side of the
//                                 column, with the per-block sums of R_j^2 (k_reduce_partials ends them): 2 K in, K out.
//   k_apply_var_multi<T, NQ, K>   out_j = A v_j, the operator read once for the set: NQ + 2 K words per point, built
//                                 from load_rows / load_coefs / stencil_sum as k_residual_var is.  AX and AP (K = nev),
//                                 AW (K = |act|).
// The cycle itself is the handle's one walk (vcycle) on the set of active columns.
#pragma once

#include "mgx_multi.hpp"

namespace mgx {

constexpr int kEigMaxIn = 3 * kMultiMax;

// the per-lane products of one row, in double, left to right
template <typename T> __device__ __forceinline__ double lane_dot(const Lanes<T>& a, const Lanes<T>& b)
{
    double s = (double)a.a[0] * (double)b.a[0];
#pragma unroll
    for (int x = 1; x < VecOf<T>::W; ++x) s += (double)a.a[x] * (double)b.a[x];
    return s;
}

// NE doubles per lane -> NE per workgroup, in block_reduce's order: down each wave by shuffles, the waves through LDS,
// thread e adds the wave results of sum e in wave order and stores partial[e * stride + block]
template <int NE>
__device__ __forceinline__ void eig_block_reduce(const double (&acc)[NE], double (*wsum)[kWavesPerBlock], double* __restrict__ partial, int stride)
{
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        double v = acc[e];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
        if ((threadIdx.x & 63) == 0) wsum[e][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < NE) {
        double s = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) s += wsum[threadIdx.x][w];
        partial[(long)threadIdx.x * stride + blockIdx.x] = s;
    }
}

// partial[(i * 2 KC + j) * stride + block] = the block's sum of l_i . r_j, r = [B, A B] (2 KC vectors); a wave marches
// down R rows of its strip.  Halo lanes and the columns that are not unknowns contribute zero
template <typename T, int KL, int KC, bool DIAG>
__global__ void __launch_bounds__(kBlock)
k_eig_gram(MultiIn<T, KL> l, MultiIn<T, 2 * KC> r, double* __restrict__ partial, int stride, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    static_assert(!DIAG || KL == KC, "a diagonal pair has one block");
    constexpr int KR = 2 * KC;
    __shared__ double wsum[KL * KR][kWavesPerBlock];
    double acc[KL * KR];
#pragma unroll
    for (int e = 0; e < KL * KR; ++e) acc[e] = 0.0;
    const Tile t = wave_tile(strips, chunks);
    const Cols c = lane_cols<VecOf<T>::W>(t.strip, N, pitch);
    if (t.active) {
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        const bool ld = c.ld && c.st;
        for (int y = r0; y < r1; ++y) {
            const long at = c.col + (long)y * pitch;
            Lanes<T> a[KL], b[KR];
#pragma unroll
            for (int i = 0; i < KL; ++i) {
                V v = vload<V>(l.p[i] + at, ld);
                mask_cols(v, c.col, N);
                a[i] = to_lanes(v);
            }
#pragma unroll
            for (int j = 0; j < KR; ++j) {
                if (DIAG && j < KL) { b[j] = a[j < KL ? j : 0]; continue; }
                V v = vload<V>(r.p[j] + at, ld);
                mask_cols(v, c.col, N);
                b[j] = to_lanes(v);
            }
#pragma unroll
            for (int i = 0; i < KL; ++i)
#pragma unroll
                for (int j = 0; j < KR; ++j) acc[i * KR + j] += lane_dot(a[i], b[j]);
        }
    }
    eig_block_reduce<KL * KR>(acc, wsum, partial, stride);
}

// out[e] = the sum of partial[e * stride .. + n) in k_reduce_partials' order, one workgroup per sum
static __global__ void __launch_bounds__(kReduceThreads) k_eig_reduce_rows(const double* __restrict__ partial, int n, int stride, double* __restrict__ out)
{
    __shared__ double wsum[kReduceThreads / kWave];
    const double* p = partial + (long)blockIdx.x * stride;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * kReduceThreads < n; i += 4 * kReduceThreads) {
        a0 += p[i];
        a1 += p[i + kReduceThreads];
        a2 += p[i + 2 * kReduceThreads];
        a3 += p[i + 3 * kReduceThreads];
    }
    for (; i < n; i += kReduceThreads) a0 += p[i];
    double acc = (a0 + a1) + (a2 + a3);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kReduceThreads / kWave; ++w) s += wsum[w];
        out[blockIdx.x] = s;
    }
}

template <int KI, int KO> struct EigCoef { double c[KI][KO]; };

template <typename T, int KI, int KO>
__global__ void __launch_bounds__(kBlock)
k_eig_combine(MultiIn<T, KI> in, MultiOut<T, KO> out, EigCoef<KI, KO> cf, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const Tile t = wave_tile(strips, chunks);
    if (!t.active) return;
    const Cols c = lane_cols<W>(t.strip, N, pitch);
    const int r0 = 1 + t.chunk * R;
    const int r1 = min(r0 + R, N);
    const bool ld = c.ld && c.st;
    for (int y = r0; y < r1; ++y) {
        const long at = c.col + (long)y * pitch;
        Lanes<T> v[KI];
#pragma unroll
        for (int i = 0; i < KI; ++i) v[i] = to_lanes(vload<V>(in.p[i] + at, ld));
        V o[KO];
#pragma unroll
        for (int j = 0; j < KO; ++j) {
            Lanes<T> s;
#pragma unroll
            for (int x = 0; x < W; ++x) s.a[x] = (T)cf.c[0][j] * v[0].a[x];
#pragma unroll
            for (int i = 1; i < KI; ++i)
#pragma unroll
                for (int x = 0; x < W; ++x) s.a[x] = s.a[x] + (T)cf.c[i][j] * v[i].a[x];
            o[j] = from_lanes(s);
            mask_cols(o[j], c.col, N);
        }
#pragma unroll
        for (int j = 0; j < KO; ++j) vstore<V>(out.p[j] + at, o[j], c.st);
    }
}

template <int K> struct EigTheta { double t[K]; };

template <typename T, int K>
__global__ void __launch_bounds__(kBlock)
k_eig_residual(MultiIn<T, K> ax, MultiIn<T, K> x, MultiOut<T, K> r, MultiOut<double, K> partial, EigTheta<K> th, int N, long pitch, int R,
               int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[K][kWavesPerBlock];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    const Tile t = wave_tile(strips, chunks);
    const Cols c = lane_cols<W>(t.strip, N, pitch);
    if (t.active) {
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        const bool ld = c.ld && c.st;
        for (int y = r0; y < r1; ++y) {
            const long at = c.col + (long)y * pitch;
            Lanes<T> a[K], b[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { a[j] = to_lanes(vload<V>(ax.p[j] + at, ld)); b[j] = to_lanes(vload<V>(x.p[j] + at, ld)); }
            V o[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                Lanes<T> d;
#pragma unroll
                for (int q = 0; q < W; ++q) d.a[q] = a[j].a[q] - (T)th.t[j] * b[j].a[q];
                o[j] = from_lanes(d);
                mask_cols(o[j], c.col, N);
                const Lanes<T> m = to_lanes(o[j]);
                acc[j] += lane_dot(m, m);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) vstore<V>(r.p[j] + at, o[j], c.st);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) block_reduce<kWavesPerBlock>(acc[j], wsum[j], partial.p[j] + blockIdx.x, ReduceSum{});
}

template <typename T, int NQ, int K>
__global__ void __launch_bounds__(kBlock)
k_apply_var_multi(MultiIn<T, K> vin, MultiOut<T, K> out, Op9<T> a, int N, long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    RowTile<T> t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = load_rows<T>(vin.p[j], N, pitch, row_lo, row_hi, strips, rows_alloc);
    if (!t[0].active) return;
    Lanes<T> k[9];
    load_coefs<NQ, 0>(a, t[0].at, t[0].in, k);
    V ov[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
        ov[j] = masked_row(stencil_sum<NQ>(rows_of<NQ>(t[j]), k, [&](int x) { return k[0].a[x]; }), t[j], N);
#pragma unroll
    for (int j = 0; j < K; ++j) vstore<V>(out.p[j] + t[j].at, ov[j], t[j].st);
}

// ---- launches: host arrays of pointers in, the column counts resolved to instances -----------------------------------------
// the geometry of k_eig_gram, k_eig_combine and k_eig_residual is a Krylov pass's (make_launch(N, W, N - 1, rows_per_chunk)),
// that of k_apply_var_multi the cycle's (one row per wave)
struct EigGeom { int N; long pitch; int rows; Launch g, g1; };

// out[i * 2 kc + j], i < kl, j < 2 kc: l_i . r_j, r = [B, A B]; diag: B is l (kl == kc, r[0 .. kc) ignored).
// partial holds 2 kl kc * g.blocks doubles
template <typename T>
void launch_eig_gram(int kl, int kc, bool diag, const T* const* l, const T* const* r, double* partial, double* out, const EigGeom& e, hipStream_t st)
{
    const Launch& g = e.g;
    with_count<kMultiMax>(kl, [&](auto tl) {
        constexpr int KL = decltype(tl)::value;
        with_count<kMultiMax>(kc, [&](auto tc) {
            constexpr int KC = decltype(tc)::value;
            MultiIn<T, KL> li;
            MultiIn<T, 2 * KC> ri;
            for (int i = 0; i < KL; ++i) li.p[i] = l[i];
            for (int j = 0; j < 2 * KC; ++j) ri.p[j] = r[j];
            if constexpr (KL == KC) {
                if (diag) {
                    hipLaunchKernelGGL((k_eig_gram<T, KL, KC, true>), dim3(g.blocks), dim3(kBlock), 0, st, li, ri, partial, g.blocks, e.N, e.pitch,
                                       g.R, g.strips, g.chunks);
                    return;
                }
            }
            hipLaunchKernelGGL((k_eig_gram<T, KL, KC, false>), dim3(g.blocks), dim3(kBlock), 0, st, li, ri, partial, g.blocks, e.N, e.pitch, g.R,
                               g.strips, g.chunks);
        });
    });
    hipLaunchKernelGGL(k_eig_reduce_rows, dim3(2 * kl * kc), dim3(kReduceThreads), 0, st, partial, g.blocks, g.blocks, out);
}

// out_j = sum_i c[i * ko + j] in_i, ki <= kEigMaxIn, ko <= kMultiMax
template <typename T>
void launch_eig_combine(int ki, int ko, const T* const* in, T* const* out, const double* c, const EigGeom& e, hipStream_t st)
{
    const Launch& g = e.g;
    with_count<kEigMaxIn>(ki, [&](auto ti) {
        constexpr int KI = decltype(ti)::value;
        with_count<kMultiMax>(ko, [&](auto to) {
            constexpr int KO = decltype(to)::value;
            MultiIn<T, KI> vi;
            MultiOut<T, KO> vo;
            EigCoef<KI, KO> cf;
            for (int i = 0; i < KI; ++i) {
                vi.p[i] = in[i];
                for (int j = 0; j < KO; ++j) cf.c[i][j] = c[i * KO + j];
            }
            for (int j = 0; j < KO; ++j) vo.p[j] = out[j];
            hipLaunchKernelGGL((k_eig_combine<T, KI, KO>), dim3(g.blocks), dim3(kBlock), 0, st, vi, vo, cf, e.N, e.pitch, g.R, g.strips, g.chunks);
        });
    });
}

// r_j = ax_j - theta_j x_j, sums[j] = ||r_j||^2 through part[j] (g.blocks doubles each)
template <typename T>
void launch_eig_residual(int k, const T* const* ax, const T* const* x, T* const* r, double* const* part, double* const* sums, const double* theta,
                         const EigGeom& e, hipStream_t st)
{
    const Launch& g = e.g;
    with_count<kMultiMax>(k, [&](auto tk) {
        constexpr int K = decltype(tk)::value;
        MultiIn<T, K> a, b;
        MultiOut<T, K> o;
        MultiOut<double, K> p;
        EigTheta<K> th;
        for (int j = 0; j < K; ++j) { a.p[j] = ax[j]; b.p[j] = x[j]; o.p[j] = r[j]; p.p[j] = part[j]; th.t[j] = theta[j]; }
        hipLaunchKernelGGL((k_eig_residual<T, K>), dim3(g.blocks), dim3(kBlock), 0, st, a, b, o, p, th, e.N, e.pitch, g.R, g.strips, g.chunks);
    });
    for (int j = 0; j < k; ++j) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, part[j], g.blocks, sums[j]);
}

// out_j = A v_j on k <= kMultiMax columns of a five- or nine-point level
template <typename T>
void launch_eig_apply(int k, bool nine, const T* const* v, T* const* out, const Op9<T>& a, const EigGeom& e, hipStream_t st)
{
    const Launch& g = e.g1;
    with_point_count(nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        with_count<kMultiMax>(k, [&](auto tk) {
            constexpr int K = decltype(tk)::value;
            MultiIn<T, K> vi;
            MultiOut<T, K> vo;
            for (int j = 0; j < K; ++j) { vi.p[j] = v[j]; vo.p[j] = out[j]; }
            hipLaunchKernelGGL((k_apply_var_multi<T, NQ, K>), dim3(g.blocks), dim3(kBlock), 0, st, vi, vo, a, e.N, e.pitch, 1, e.N, g.strips, e.rows);
        });
    });
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=11) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
#define MGX_EIG_EXTERN(T)                                                                                                                   \
    extern template void launch_eig_gram<T>(int, int, bool, const T* const*, const T* const*, double*, double*, const EigGeom&, hipStream_t); \
    extern template void launch_eig_combine<T>(int, int, const T* const*, T* const*, const double*, const EigGeom&, hipStream_t);             \
    extern template void launch_eig_residual<T>(int, const T* const*, const T* const*, T* const*, double* const*, double* const*,             \
                                                const double*, const EigGeom&, hipStream_t);                                                  \
    extern template void launch_eig_apply<T>(int, bool, const T* const*, T* const*, const Op9<T>&, const EigGeom&, hipStream_t);
MGX_EIG_EXTERN(double)
MGX_EIG_EXTERN(float)
#undef MGX_EIG_EXTERN
#endif

} // namespace mgx
