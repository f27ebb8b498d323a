// mgx_krylov.hpp - the device side of the Krylov solves (their host side: mgx_krylov_host.hpp).
//
// mgx_solve_pcg: conjugate gradients on the finest level, preconditioned by one V-cycle from zero (absent in the
// reference).
//
// Flexible PCG with the Polak-Ribiere beta; per iteration, after the V-cycle z = M r:
//   k_pcg_dots       rho_new = r.z and gamma = z.q                         reads r, z, q           3 sizeof(T)
//   k_pcg_direction  p' = z + beta p, q = A p', delta = p'.q               reads z, p; writes p', q 4 sizeof(T)
//                    (general operators: + the five / nine coefficient     (+ 5 / 9 sizeof(T))
//                    grids of a five- / nine-point finest level)
//   k_pcg_update     x += alpha p, r -= alpha q, ||r||^2                   reads x, p, r, q;
//                                                                          writes x, r             6 sizeof(T)
//   k_pcg_reduce     the per-block partials of one pass summed in a fixed order by one workgroup, and the scalar
//                    that depends on them (alpha after delta; beta and rho after the dots): no host round trip
// 13 sizeof(T) per fine point and iteration: 104 B in double, 52 B in float (18 / 22 with the coefficient grids of a
// five- / nine-point finest operator: the direction pass alone moves 4 / 9 / 13 sizeof(T)).
//
// Every pass covers rows 1 .. N-1 in the geometry of k_residual (row chunks marching down a column strip,
// W-wide vectors, halo lanes 0 and 63 never store) and masks columns 0 and >= N, so the Dirichlet ring and the
// padding of p, q and x stay zero: A reads them as neighbours.  p is written out of place (p' into a second
// buffer): a wave's halo rows and halo lanes are another wave's output.  Dots are accumulated in double whatever
// T is, per lane, then per wave (shuffles), per workgroup (LDS) and over the workgroups (k_pcg_reduce): the same
// order on every call - no atomics.  alpha and beta are doubles on the device, rounded to T once where applied.
//
// mgx_solve_gcr: restarted GCR with right preconditioning (FGMRES(m) in exact arithmetic), for
// operators and cycles that are not symmetric.  Vectors in T, dots in double, scalars doubles rounded to T once
// where they are applied, every elementwise operation rounded separately:
//   r = b - A x;  h0 = ||r||;  basis empty
//   iteration k:  j = k mod restart;  if j == 0: basis empty
//     z = M r                                   (zero-start cycle)
//     q = A z                                   (stencil order of k_pcg_direction: residual_vec / stencil_sum<5 | 9>)
//     h_i = (q.Q_i) / s_i   for i < j           (classical Gram-Schmidt: all dots from the unmodified q)
//     q' = ((q - h_0 Q_0) - h_1 Q_1) - ... ;  z' = the same combination of z and Z_i
//     s_j = q'.q';  rho = r.q';  breakdown unless s_j > 0 and finite;  alpha = rho / s_j
//     x += alpha z';  r -= alpha q';  history <- sqrt(r.r);  Z_j = z', Q_j = q'
//     stop when ||r|| <= tol h0 or k + 1 == max_iters
// per iteration, after the cycle:
//   k_pcg_direction  first_it = 1: Z_j = z (out of lv.u), Q_j = q = A z        as above       4 (+ 5 | 9) sizeof(T)
//   k_gcr_dots<J>    q.Q_i, i < J (J = j >= 1)               reads q, Q_0 .. Q_{J-1}          (1 + J) sizeof(T)
//   k_gcr_orth<J>    q', z' in place in slot J, q'.q', r.q'  reads q, z, r, J pairs; writes q', z'
//                                                                                             (5 + 2J) sizeof(T)
//                    (J = 0: the two dots only, reads q and r, stores nothing:                2 sizeof(T))
//   k_pcg_update     x += alpha Z_j, r -= alpha Q_j, ||r||^2                                  6 sizeof(T)
//   k_gcr_reduce     the partials of k_gcr_dots -> h_i, of k_gcr_orth -> s_j, rho, alpha and the breakdown flag
// J is a template parameter (dispatched by a switch on the host): accumulators and basis pointers indexed by a
// compile-time count stay in registers and kernel arguments, a run-time count would send them to scratch.
#pragma once

#include "mgx_kernels.hpp"
#include "mgx_var.hpp"

namespace mgx {

// the device-side scalars of one PCG solve: the first slots of the block both methods share (mgx_solver::kry.sc)
enum { kPcgRho = 0, kPcgDelta, kPcgAlpha, kPcgBeta, kPcgGamma, kPcgRR, kPcgBreak, kPcgScalars = 8 };
enum { kPcgInit = 0, kPcgAlphaMode = 1, kPcgRRMode = 2, kPcgBetaMode = 3 };

// sum of a lane's products in double: a.x b.x + a.y b.y (+ a.z b.z + a.w b.w), pairwise like k_residual's sums
__device__ __forceinline__ double vdot(const double2& a, const double2& b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ double vdot(const float4& a, const float4& b)
{
    return ((double)a.x * (double)b.x + (double)a.y * (double)b.y) + ((double)a.z * (double)b.z + (double)a.w * (double)b.w);
}
__device__ __forceinline__ double2 vaxpy(const double2& x, double a, const double2& y) { return make_double2(x.x + a * y.x, x.y + a * y.y); }
__device__ __forceinline__ float4 vaxpy(const float4& x, float a, const float4& y)
{
    return make_float4(x.x + a * y.x, x.y + a * y.y, x.z + a * y.z, x.w + a * y.w);
}
__device__ __forceinline__ double2 vaxmy(const double2& x, double a, const double2& y) { return make_double2(x.x - a * y.x, x.y - a * y.y); }
__device__ __forceinline__ float4 vaxmy(const float4& x, float a, const float4& y)
{
    return make_float4(x.x - a * y.x, x.y - a * y.y, x.z - a * y.z, x.w - a * y.w);
}

// A u of the constant stencil, the operator of residual_vec: -(((N + W) + E) + S) + 4 u
__device__ __forceinline__ double2 poisson_vec(const double2& up, const double2& cur, const double2& dn)
{
    const double l = from_left(cur.y), r = from_right(cur.x);
    return make_double2(-nbr(up.x, l, cur.y, dn.x) + 4.0 * cur.x, -nbr(up.y, cur.x, r, dn.y) + 4.0 * cur.y);
}
__device__ __forceinline__ float4 poisson_vec(const float4& up, const float4& cur, const float4& dn)
{
    const NbrPairs t = nbr_pairs(up, cur, dn);
    const f32x2 p0 = {cur.x, cur.y}, p1 = {cur.z, cur.w};
    const f32x2 o0 = -t.t0 + 4.f * p0, o1 = -t.t1 + 4.f * p1;
    return make_float4(o0.x, o0.y, o1.x, o1.y);
}

// rho_new = r.z -> partial[b],  gamma = z.q -> partial[nb + b]   (nb = gridDim.x)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_pcg_dots(const T* __restrict__ r, const T* __restrict__ z, const T* __restrict__ q, double* __restrict__ partial,
           int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[2][kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double rz = 0.0, zq = 0.0;
    if (t.active) {
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                const V rr = vload<V>(r + at, true), zz = vload<V>(z + at, true), qq = vload<V>(q + at, true);
                rz += vdot(rr, zz);
                zq += vdot(zz, qq);
            }
        }
    }
    block_reduce<kWavesPerBlock>(rz, wsum[0], partial + blockIdx.x, ReduceSum{});
    block_reduce<kWavesPerBlock>(zq, wsum[1], partial + (long)gridDim.x + blockIdx.x, ReduceSum{});
}

// p' = z + beta p (first_it: p' = z, p not read), q = A p', delta partials p'.q.  A lane forms p' of its row
// neighbours from z and p as it marches down (rows r0-1 .. r1), its column neighbours come from the adjacent lanes.
// OP 0: the constant five-point stencil in the order of residual_vec (A u = -(((N + W) + E) + S) + 4 u);
// OP 1: the level's five coefficient grids a, in the order of stencil_sum<5>();
// OP 2: its nine coefficient grids, in the order of stencil_sum<9>() (the CSR order of mgx_var.hpp): a lane then also
// needs the elements left and right of its vector in the rows above and below (Rows3::ul, ur, dl, dr), p' of the
// adjacent lanes in those rows; ring rows and columns are zero without a load, as for the other two.
template <typename T, int OP>
__global__ void __launch_bounds__(kBlock)
k_pcg_direction(const T* __restrict__ z, const T* __restrict__ p, T* __restrict__ pn, T* __restrict__ q,
                const double* __restrict__ sc, int first_it, double* __restrict__ partial, Op9<T> a,
                int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc = 0.0;
    if (t.active) {
        const T beta = first_it ? (T)0 : (T)sc[kPcgBeta];
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        // rows 0 and N are the Dirichlet ring: p' = 0 there without a load
        auto prow = [&](int y) -> V {
            const bool in = c.ld && y >= 1 && y < N;
            const long at = c.col + (long)y * pitch;
            V v = vload<V>(z + at, in);
            if (!first_it) v = vaxpy(v, beta, vload<V>(p + at, in));
            mask_cols(v, c.col, N);
            return v;
        };
        V up = prow(r0 - 1);
        V cur = prow(r0);
        // OP 2: the edge values of the rows above and at y from the adjacent lanes, two moves per new row: those of
        // row y + 1 are taken when it is formed and handed up as the march goes down
        T ul = (T)0, ur = (T)0, cl = (T)0, cr = (T)0;
        if constexpr (OP == 2) {
            ul = from_left(last(up)); ur = from_right(first(up));
            cl = from_left(last(cur)); cr = from_right(first(cur));
        }
        for (int y = r0; y < r1; ++y) {
            const V dn = prow(y + 1);
            const long at = c.col + (long)y * pitch;
            V o;
            if constexpr (OP == 0) {
                o = poisson_vec(up, cur, dn);
            } else if constexpr (OP == 1) {
                Lanes<T> k[9];
                load_coefs<5, 0>(a, at, c.ld, k);
                Rows3<T> u{to_lanes(up), to_lanes(cur), to_lanes(dn)};
                u.cl = from_left(last(cur)); u.cr = from_right(first(cur));
                o = from_lanes(stencil_sum<5>(u, k, [&](int x) { return k[0].a[x]; }));
            } else {
                Lanes<T> k[9];
                load_coefs<9, 0>(a, at, c.ld, k);
                const T dl = from_left(last(dn)), dr = from_right(first(dn));
                const Rows3<T> u{to_lanes(up), to_lanes(cur), to_lanes(dn), ul, ur, cl, cr, dl, dr};
                o = from_lanes(stencil_sum<9>(u, k, [&](int x) { return k[0].a[x]; }));
                ul = cl; ur = cr; cl = dl; cr = dr;
            }
            mask_cols(o, c.col, N);
            vstore<V>(pn + at, cur, c.st);
            vstore<V>(q + at, o, c.st);
            if (c.st) acc += vdot(cur, o);
            up = cur; cur = dn;
        }
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// x += alpha p, r -= alpha q, partials of ||r||^2.  After a breakdown (sc[kPcgBreak] != 0) nothing is updated.
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_pcg_update(T* __restrict__ x, const T* __restrict__ p, T* __restrict__ r, const T* __restrict__ q,
             const double* __restrict__ sc, double* __restrict__ partial, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc = 0.0;
    if (t.active && sc[kPcgBreak] == 0.0) {
        const T alpha = (T)sc[kPcgAlpha];
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                const V xx = vaxpy(vload<V>(x + at, true), alpha, vload<V>(p + at, true));
                const V rr = vaxmy(vload<V>(r + at, true), alpha, vload<V>(q + at, true));
                vstore<V>(x + at, xx, true);
                vstore<V>(r + at, rr, true);
                acc += vdot(rr, rr);
            }
        }
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// fixed-order sum of n partials (the order of k_reduce_partials)
__device__ __forceinline__ double pcg_reduce_sum(const double* __restrict__ part, int n, double* wsum)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * kReduceThreads < n; i += 4 * kReduceThreads) {
        a0 += part[i];
        a1 += part[i + kReduceThreads];
        a2 += part[i + 2 * kReduceThreads];
        a3 += part[i + 3 * kReduceThreads];
    }
    for (; i < n; i += kReduceThreads) a0 += part[i];
    double acc = (a0 + a1) + (a2 + a3);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kReduceThreads / kWave; ++w) s += wsum[w];
    return s;                                   // the same value in every thread
}

// one workgroup: the partials of the pass just run and the scalars that follow from them
//   kPcgInit:       rho = r.z, beta = 0, no breakdown
//   kPcgAlphaMode:  delta = p.q; alpha = rho / delta, or a breakdown (delta not > 0 or not finite: alpha = 0)
//   kPcgRRMode:     ||r||^2
//   kPcgBetaMode:   rho_new = r.z, gamma = z.q; beta = -alpha gamma / rho; rho = rho_new
static __global__ void __launch_bounds__(kReduceThreads) k_pcg_reduce(const double* __restrict__ part, int n, int mode, double* __restrict__ sc)
{
    __shared__ double wsum[kReduceThreads / kWave];
    const double s0 = pcg_reduce_sum(part, n, wsum);
    const double s1 = (mode == kPcgBetaMode) ? pcg_reduce_sum(part + n, n, wsum) : 0.0;
    if (threadIdx.x != 0) return;
    if (mode == kPcgInit) {
        sc[kPcgRho] = s0; sc[kPcgBeta] = 0.0; sc[kPcgBreak] = 0.0;
    } else if (mode == kPcgAlphaMode) {
        sc[kPcgDelta] = s0;
        const bool ok = (s0 > 0.0) && isfinite(s0);
        sc[kPcgAlpha] = ok ? sc[kPcgRho] / s0 : 0.0;
        sc[kPcgBreak] = ok ? 0.0 : 1.0;
    } else if (mode == kPcgRRMode) {
        sc[kPcgRR] = s0;
    } else {
        sc[kPcgGamma] = s1;
        sc[kPcgBeta] = -sc[kPcgAlpha] * s1 / sc[kPcgRho];
        sc[kPcgRho] = s0;
    }
}

// ---- mgx_solve_gcr ------------------------------------------------------------------------------------------------
constexpr int kGcrMaxRestart = 8;              // MGX_GCR_MAX_RESTART
// the whole scalar block, as a GCR solve uses it: the first kPcgScalars slots are k_pcg_update's and k_pcg_reduce's (rho = r.q',
// delta = s_j = q'.q', alpha, ||r||^2, the breakdown flag), then s_i of the basis and h_i of this iteration
enum { kGcrS = kPcgScalars, kGcrH = kGcrS + kGcrMaxRestart, kGcrScalars = kGcrH + kGcrMaxRestart };
enum { kGcrHMode = 0, kGcrAlphaMode = 1 };

// the earlier vectors of the basis, by value: Q_i = A Z_i, i < J <= 7
template <typename T> struct GcrBasis { const T* Q[kGcrMaxRestart - 1]; const T* Z[kGcrMaxRestart - 1]; };

// q.Q_i -> partial[i nb + b], i < J   (nb = gridDim.x)
template <typename T, int J>
__global__ void __launch_bounds__(kBlock)
k_gcr_dots(const T* __restrict__ q, GcrBasis<T> bs, double* __restrict__ partial, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[J][kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc[J];
#pragma unroll
    for (int i = 0; i < J; ++i) acc[i] = 0.0;
    if (t.active) {
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                const V qq = vload<V>(q + at, true);
#pragma unroll
                for (int i = 0; i < J; ++i) acc[i] += vdot(qq, vload<V>(bs.Q[i] + at, true));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < J; ++i) block_reduce<kWavesPerBlock>(acc[i], wsum[i], partial + (long)i * gridDim.x + blockIdx.x, ReduceSum{});
}

// q' = ((q - h_0 Q_0) - h_1 Q_1) - ..., z' likewise from z and Z_i, both in place (slot J: a lane reads and writes its
// own vector only); q'.q' -> partial[b], r.q' -> partial[nb + b].  J = 0: q' = q and z' = z, nothing is stored.
template <typename T, int J>
__global__ void __launch_bounds__(kBlock)
k_gcr_orth(T* q, T* z, const T* __restrict__ r, GcrBasis<T> bs, const double* __restrict__ sc, double* __restrict__ partial,
           int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[2][kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double ss = 0.0, rq = 0.0;
    if (t.active) {
        T h[J > 0 ? J : 1];
#pragma unroll
        for (int i = 0; i < J; ++i) h[i] = (T)sc[kGcrH + i];
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                V qq = vload<V>(q + at, true);
                const V rr = vload<V>(r + at, true);
                if constexpr (J > 0) {
                    V zz = vload<V>(z + at, true);
#pragma unroll
                    for (int i = 0; i < J; ++i) {
                        qq = vaxmy(qq, h[i], vload<V>(bs.Q[i] + at, true));
                        zz = vaxmy(zz, h[i], vload<V>(bs.Z[i] + at, true));
                    }
                    mask_cols(qq, c.col, N);
                    mask_cols(zz, c.col, N);
                    vstore<V>(q + at, qq, true);
                    vstore<V>(z + at, zz, true);
                }
                ss += vdot(qq, qq);
                rq += vdot(rr, qq);
            }
        }
    }
    block_reduce<kWavesPerBlock>(ss, wsum[0], partial + blockIdx.x, ReduceSum{});
    block_reduce<kWavesPerBlock>(rq, wsum[1], partial + (long)gridDim.x + blockIdx.x, ReduceSum{});
}

// one workgroup, after the pass whose partials it sums (n per dot, in the order of k_pcg_reduce):
//   kGcrHMode:      h_i = (q.Q_i) / s_i for i < j
//   kGcrAlphaMode:  s_j = q'.q' (kept for the later iterations of this restart cycle, and in k_pcg_update's delta
//                   slot), rho = r.q'; alpha = rho / s_j, or a breakdown (s_j not > 0 or not finite: alpha = 0)
static __global__ void __launch_bounds__(kReduceThreads) k_gcr_reduce(const double* __restrict__ part, int n, int mode, int j, double* __restrict__ sc)
{
    __shared__ double wsum[kReduceThreads / kWave];
    if (mode == kGcrHMode) {
        for (int i = 0; i < j; ++i) {
            const double d = pcg_reduce_sum(part + (long)i * n, n, wsum);
            if (threadIdx.x == 0) sc[kGcrH + i] = d / sc[kGcrS + i];
        }
        return;
    }
    const double s = pcg_reduce_sum(part, n, wsum);
    const double rho = pcg_reduce_sum(part + n, n, wsum);
    if (threadIdx.x != 0) return;
    const bool ok = (s > 0.0) && isfinite(s);
    sc[kPcgDelta] = s;
    sc[kPcgRho] = rho;
    sc[kPcgAlpha] = ok ? rho / s : 0.0;
    sc[kPcgBreak] = ok ? 0.0 : 1.0;
    sc[kGcrS + j] = s;
}

// the two passes of iteration j = k mod restart (after k_pcg_direction has left z in zj and q = A z in qj), each
// followed by its reduction; bs holds the j earlier pairs.  passes: all of them in the solve; mgx_time_gcr_pass
// launches one streaming pass alone
enum { kGcrDotsPass = 1, kGcrOrthPass = 2, kGcrReducePass = 4, kGcrAllPasses = 7 };
template <typename T, int J>
void launch_gcr_orth_j(T* qj, T* zj, const T* r, const GcrBasis<T>& bs, double* sc, double* part, int N, long pitch, const Launch& g,
                       int passes, hipStream_t st)
{
    const bool red = passes & kGcrReducePass;
    if constexpr (J > 0) {
        if (passes & kGcrDotsPass)
            hipLaunchKernelGGL((k_gcr_dots<T, J>), dim3(g.blocks), dim3(kBlock), 0, st, (const T*)qj, bs, part, N, pitch, g.R, g.strips, g.chunks);
        if (red) hipLaunchKernelGGL(k_gcr_reduce, dim3(1), dim3(kReduceThreads), 0, st, part, g.blocks, (int)kGcrHMode, J, sc);
    }
    if (passes & kGcrOrthPass)
        hipLaunchKernelGGL((k_gcr_orth<T, J>), dim3(g.blocks), dim3(kBlock), 0, st, qj, zj, r, bs, (const double*)sc, part, N, pitch, g.R, g.strips,
                           g.chunks);
    if (red) hipLaunchKernelGGL(k_gcr_reduce, dim3(1), dim3(kReduceThreads), 0, st, part, g.blocks, (int)kGcrAlphaMode, J, sc);
}

template <typename T>
void launch_gcr_orth(int j, T* qj, T* zj, const T* r, const GcrBasis<T>& bs, double* sc, double* part, int N, long pitch, const Launch& g,
                     int passes, hipStream_t st)
{
    switch (j) {
        case 0: launch_gcr_orth_j<T, 0>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        case 1: launch_gcr_orth_j<T, 1>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        case 2: launch_gcr_orth_j<T, 2>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        case 3: launch_gcr_orth_j<T, 3>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        case 4: launch_gcr_orth_j<T, 4>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        case 5: launch_gcr_orth_j<T, 5>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        case 6: launch_gcr_orth_j<T, 6>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
        default: launch_gcr_orth_j<T, 7>(qj, zj, r, bs, sc, part, N, pitch, g, passes, st); break;
    }
}

// mgx.hip (through mgx_krylov_host.hpp) uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=7) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template void launch_gcr_orth<double>(int, double*, double*, const double*, const GcrBasis<double>&, double*, double*, int, long, const Launch&, int, hipStream_t);
extern template void launch_gcr_orth<float>(int, float*, float*, const float*, const GcrBasis<float>&, double*, double*, int, long, const Launch&, int, hipStream_t);
#endif

} // namespace mgx
