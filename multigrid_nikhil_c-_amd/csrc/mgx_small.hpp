// mgx_small.hpp - one visit of a small nine-point level in ONE launch of ONE workgroup (W- and F-cycles, mgx_set_cycle).
//
// A W-cycle visits level l 2^(finest - l) times, and a visit of a level with N <= 64 is 6-7 launches that move a few
// hundred kilobytes: pure launch latency.  k_small_visit performs what a visit does to the level between two visits of
// the level below, chosen by its stage arguments:
//   ascend   U += P e (e = U of the level below), then mu2 sweeps
//   descend  mu1 sweeps, the residual B - A U, its restriction into the coarse B, the coarse U zeroed
//   turn     ascend, then at once descend on the same level with the same B: what separates the two sub-cycles of a
//            W- or F-cycle
// Scope: nine-point levels of a GALERKIN hierarchy (either transfer, CONSISTENT or FW16, double or float), Jacobi.
//
// A lane owns VPL vectors of W columns (double: 2 x 2 = 4 points at 63^2 with 1024 lanes; float: 1 x 4).  It loads
// their D_inv, the eight off-diagonals of R_omega and b ONCE and keeps them in registers across every sweep; the iterate
// ping-pongs between two N x N arrays in LDS (rows and columns 0 .. N - 1: the ring row / column 0 is stored, zero; row
// and column N are a predicate), one workgroup barrier per sweep.  The operator's own nine coefficients, needed by the
// residual only, are loaded after the last sweep, when the registers of R_omega are free.  LDS: 2 N^2 sizeof(T) = 64 KB
// at N = 64 in double.
//
// Every value is formed by the device functions of the per-level kernels - stencil_sum<9> and jacobi_value
// (k_jacobi_var), stencil_sum<9> with the operator's centre (k_residual_var), opdep_restrict_value / opdep_prolong_*
// (k_restrict_opdep, k_prolong_opdep), restrict_fw_value / prolong_*_value (k_restrict, k_prolong) - so the result is
// bit-identical to the per-level launches (tests/test_gpu_wcycle.py compares them with MGX_SMALL_VISIT=0).
#pragma once

#include "mgx_opdep.hpp"

namespace mgx {

constexpr int kSmallBlock = 1024;
constexpr int kSmallMaxN = 64;

template <typename T> struct SmallVisit {
    T* u;                      // the level's iterate, updated in place
    const T* b;
    Op9<T> a, r;               // the operator and the off-diagonals of R_omega
    const T* dinv;
    T* cu;                     // U of the level below: e of the ascend stage, zeroed by the descend stage
    T* cb;                     // B of the level below
    Wt8<T> w;                  // weights of P between this level and the one below (opdep only)
    int N;
    long pitch, cpitch;
    int ascend, descend;       // stages; both: a turn
    int mu1, mu2;
    int opdep;
    T rc, omega;               // 1 - omega, omega
    T rscale;                  // c of R = c P^T: 1 (CONSISTENT) or 1/4 (FW16)
    T wgt;                     // the bilinear restriction's weight: 1/4 or 1/16
};

// the three rows around a lane's vector out of an N x N array in LDS (row N and column N: zero)
template <typename T>
__device__ __forceinline__ Rows3<T> small_rows(const T* s, int N, int row, int col)
{
    constexpr int W = VecOf<T>::W;
    Rows3<T> u;
    const bool dn = row + 1 < N, lf = col > 0, rt = col + W < N;
    const T* pu = s + (row - 1) * N + col;
    const T* pc = pu + N;
    const T* pd = pc + N;
#pragma unroll
    for (int x = 0; x < W; ++x) { u.up.a[x] = pu[x]; u.cur.a[x] = pc[x]; u.dn.a[x] = dn ? pd[x] : (T)0; }
    u.ul = lf ? pu[-1] : (T)0; u.cl = lf ? pc[-1] : (T)0; u.dl = (lf && dn) ? pd[-1] : (T)0;
    u.ur = rt ? pu[W] : (T)0; u.cr = rt ? pc[W] : (T)0; u.dr = (rt && dn) ? pd[W] : (T)0;
    return u;
}

// (P e) at fine point (y, x), 1 <= y, x <= N - 1; e and the weights from the arrays of the level below, whose ring is zero
template <typename T>
__device__ __forceinline__ T small_prolong(const SmallVisit<T>& a, int y, int x)
{
    const int I = y >> 1, J = x >> 1;
    const long c00 = (long)I * a.cpitch + J, c01 = c00 + 1, c10 = c00 + a.cpitch, c11 = c10 + 1;
    const T* e = a.cu;
    if (!a.opdep) {
        if (!(y & 1)) return (x & 1) ? prolong_edge_value(e[c00], e[c01]) : e[c00];
        return (x & 1) ? prolong_centre_value(e[c00], e[c10], e[c01], e[c11]) : prolong_edge_value(e[c00], e[c10]);
    }
    // slots of Wt8: n 0, s 1, w 2, e 3, nw 4, ne 5, sw 6, se 7
    if (!(y & 1)) return (x & 1) ? opdep_prolong_edge(a.w.w[3][c00], e[c00], a.w.w[2][c01], e[c01]) : e[c00];
    if (!(x & 1)) return opdep_prolong_edge(a.w.w[1][c00], e[c00], a.w.w[0][c10], e[c10]);
    return opdep_prolong_centre(a.w.w[7][c00], e[c00], a.w.w[6][c01], e[c01], a.w.w[5][c10], e[c10], a.w.w[4][c11], e[c11]);
}

template <typename T>
__global__ void __launch_bounds__(kSmallBlock)
k_small_visit(const SmallVisit<T> a)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    constexpr int VPL = (kSmallMaxN - 1) * (kSmallMaxN / W) > kSmallBlock ? 2 : 1;
    static_assert((kSmallMaxN - 1) * (kSmallMaxN / W) <= VPL * kSmallBlock, "a lane's vectors cover the largest level");
    extern __shared__ double2 small_lds[];
    T* src = reinterpret_cast<T*>(small_lds);
    T* dst = src + a.N * a.N;
    const int N = a.N, VR = N / W, total = (N - 1) * VR;

    bool on[VPL];
    int row[VPL], col[VPL];
    long at[VPL];
    Lanes<T> b[VPL], d[VPL], k[VPL][9];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int v = (int)threadIdx.x + j * kSmallBlock;
        on[j] = v < total;
        row[j] = 1 + v / VR;
        col[j] = (v % VR) * W;
        at[j] = (long)row[j] * a.pitch + col[j];
        b[j] = load_lanes(a.b + at[j], on[j]);
        d[j] = load_lanes(a.dinv + at[j], on[j]);
        load_coefs<9, 1>(a.r, at[j], on[j], k[j]);
    }
    // the ring row 0 of both arrays (column 0 is written, masked, with every vector)
    for (int i = threadIdx.x; i < N; i += blockDim.x) { src[i] = (T)0; dst[i] = (T)0; }
    // the iterate, corrected by P e on the way in (PS:620-624)
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        if (!on[j]) continue;
        Lanes<T> u = load_lanes(a.u + at[j], true);
        if (a.ascend) {
            Lanes<T> pe;
#pragma unroll
            for (int x = 0; x < W; ++x) pe.a[x] = (col[j] + x >= 1) ? small_prolong(a, row[j], col[j] + x) : (T)0;
#pragma unroll
            for (int x = 0; x < W; ++x) u.a[x] = u.a[x] + pe.a[x];
        }
        V uv = from_lanes(u);
        mask_cols(uv, col[j], N);
        u = to_lanes(uv);
#pragma unroll
        for (int x = 0; x < W; ++x) src[row[j] * N + col[j] + x] = u.a[x];
    }
    __syncthreads();

    const int sweeps = (a.ascend ? a.mu2 : 0) + (a.descend ? a.mu1 : 0);
    for (int it = 0; it < sweeps; ++it) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            if (!on[j]) continue;
            const T rc = a.rc;
            const Lanes<T> p1 = stencil_sum<9>(small_rows(src, N, row[j], col[j]), k[j], [&](int) { return rc; });      // MF:86
            Lanes<T> o;
#pragma unroll
            for (int x = 0; x < W; ++x) o.a[x] = jacobi_value(p1.a[x], a.omega, d[j].a[x], b[j].a[x]);                    // MF:88, 90
            V ov = from_lanes(o);
            mask_cols(ov, col[j], N);
            o = to_lanes(ov);
#pragma unroll
            for (int x = 0; x < W; ++x) dst[row[j] * N + col[j] + x] = o.a[x];
        }
        __syncthreads();
        T* t = src; src = dst; dst = t;
    }
    // the level's iterate back to its array
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        if (!on[j]) continue;
        Lanes<T> u;
#pragma unroll
        for (int x = 0; x < W; ++x) u.a[x] = src[row[j] * N + col[j] + x];
        vstore<V>(a.u + at[j], from_lanes(u), true);
    }
    if (!a.descend) return;

    // MF:150-153: r = b - A u into the other array
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        if (!on[j]) continue;
        Lanes<T> ka[9];
        load_coefs<9, 0>(a.a, at[j], true, ka);
        const Lanes<T> av = stencil_sum<9>(small_rows(src, N, row[j], col[j]), ka, [&](int x) { return ka[0].a[x]; });
        Lanes<T> o;
#pragma unroll
        for (int x = 0; x < W; ++x) o.a[x] = b[j].a[x] - av.a[x];
        V ov = from_lanes(o);
        mask_cols(ov, col[j], N);
        o = to_lanes(ov);
#pragma unroll
        for (int x = 0; x < W; ++x) dst[row[j] * N + col[j] + x] = o.a[x];
    }
    __syncthreads();
    // PS:531-546 / c P^T: one coarse point per lane ((N / 2 - 1)^2 <= 961), and the coarse guess zeroed (PS:613)
    const int NC = N / 2, nc = NC - 1;
    for (int p = threadIdx.x; p < nc * nc; p += blockDim.x) {
        const int I = 1 + p / nc, J = 1 + p % nc;
        const T* q = dst + (2 * I - 1) * N + 2 * J - 1;
        const long c = (long)I * a.cpitch + J;
        T o;
        if (a.opdep) {
            T wk[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) wk[x] = a.w.w[x][c];
            const T r0[3] = {q[0], q[1], q[2]}, r1[3] = {q[N], q[N + 1], q[N + 2]}, r2[3] = {q[2 * N], q[2 * N + 1], q[2 * N + 2]};
            o = opdep_restrict_value(wk, r0, r1, r2, a.rscale);
        } else {
            const Trip<T> top{q[0], q[1], q[2]}, mid{q[N], q[N + 1], q[N + 2]}, bot{q[2 * N], q[2 * N + 1], q[2 * N + 2]};
            o = restrict_fw_value(top, mid, bot, a.wgt);
        }
        a.cb[c] = o;
        a.cu[c] = (T)0;
    }
}

template <typename T> inline size_t small_visit_lds(int N) { return 2 * (size_t)N * N * sizeof(T); }

// once per process and type, outside any stream capture: the kernel may use 64 KB of dynamic LDS
template <typename T> hipError_t small_visit_prepare()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_small_visit<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)small_visit_lds<T>(kSmallMaxN));
}

template <typename T> void launch_small_visit(const SmallVisit<T>& a, hipStream_t st)
{
    const int vectors = (a.N - 1) * (a.N / VecOf<T>::W);
    const int lanes = std::min(kSmallBlock, (vectors + kWave - 1) / kWave * kWave);
    hipLaunchKernelGGL((k_small_visit<T>), dim3(1), dim3(lanes), small_visit_lds<T>(a.N), st, a);
}

// mgx.hip declares these instantiations; mgx_inst.hip (-DMGX_INST_KIND=5) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template hipError_t small_visit_prepare<double>();
extern template hipError_t small_visit_prepare<float>();
extern template void launch_small_visit<double>(const SmallVisit<double>&, hipStream_t);
extern template void launch_small_visit<float>(const SmallVisit<float>&, hipStream_t);
#endif

} // namespace mgx
