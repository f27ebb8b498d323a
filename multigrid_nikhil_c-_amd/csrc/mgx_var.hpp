// mgx_var.hpp - per-level GENERAL operators, five- or nine-point: the data model of the reference's second draft
// (Multigrid_functions.cpp = MF) on the structured grid, as gfx950 kernels.  The base header of the general-operator
// path: mgx_galerkin.hpp (R A P), mgx_opdep.hpp (operator-dependent transfers), mgx_cheby.hpp and mgx_krylov.hpp build on it.
//
//   MF:16-26  ProblemVar { A_sp_dict[level], A_jacobi_sp_dict[level] = {D_inv, R_omega}, b_dict, coarsest_level_matrix }
//   MF:33-41  csr_matrix_elements: CSR per level           -> coefficient grids per level (Op9)
//   MF:75-96  jacobirelaxation: v <- R_omega v + omega D^-1 b (gemv, gemv alpha = omega, vm::add; MF:86-90)
//                                                          -> k_jacobi_var (one pass instead of three)
//   MF:122-130 restriction2D: injection                    -> k_restrict_inject
//   MF:150-153 residual = f - A v (gemv, vm::sub)          -> k_residual_var
//   MF:63-72, 137-139 direct solve of the coarsest system  -> dense inverse by Gauss-Jordan (set-up), matvec per solve
//
// AN OPERATOR (A, or the off-diagonals of R_omega) is nine coefficient grids in the level's layout, in the SLOT ORDER
//     c, n, s, w, e, nw, ne, sw, se   (slots 0..8; op9_slot(dy, dx));
// a five-point operator (NQ = 5: the caller's STENCIL5 levels, a five-point finest GALERKIN level) leaves slots 5..8 null
// or stale and no NQ = 5 code reads them; R A P is nine-point (NQ = 9: the coarse GALERKIN levels, and the finest one
// after mgx_set_stencil9 / mgx_set_tensor).
// (A u)_ij = sum over (dy, dx) of a_(dy,dx) u_(i+dy)(j+dx); the Dirichlet ring of the grid layout is zero, so
// boundary-adjacent points need no special case.  A CSR row of a row-major operator lists its columns in the CSR ORDER
//     NW, N, NE, W, C, E, SW, S, SE   (five-point: N, W, C, E, S - the same order with the corners left out),
// and that is the order every sum is taken in (stencil_sum, the one place that maps slots to it); no contraction
// (-ffp-contract=off): bit-identical to the oracle's restatement (oracle/mg_oracle_var.inc, tests/galerkin_ref.py).
//
// Roofline: every coefficient is read once per sweep, so a sweep moves v, b, D_inv and the NQ - 1 grids of R_omega in and
// v' out: (NQ + 3) sizeof(T) per point - 8 on five-point levels (64 B in double against the constant stencil's 24 B), 12
// on nine-point levels; the residual moves v, b and the NQ grids of A in and r out, the same count.  Both are single
// passes of independent rows (one wave per row and strip, like k_jacobi_rows; 16-byte lanes, the column neighbours from
// the adjacent lanes by DPP): HBM-bound, no temporal fusion (a K-level pass would need K-row windows of NQ more arrays
// in registers).
//
// COLUMNS.  The passes that read an operator (k_jacobi_var, k_residual_var, k_var_dense_solve here; k_prolong_opdep,
// k_refine_direction, the kernels of mgx_multi.hpp and mgx_eig.hpp on top) run on K = 1 .. kMultiMax vectors per launch:
// the coefficients are loaded ONCE into registers and applied to K columns, so a sweep moves (NQ + 3K) sizeof(T) per
// point instead of K (NQ + 3) - five-point, K = 4: 17 words against 32; nine-point: 21 against 48.  K = 1 is the pass of
// mgx_solve and its relatives on the level's own vectors; there is one body, so a column has the same bits however the
// columns are grouped into launches.  K is a compile-time parameter; the column pointers arrive by value (MultiIn /
// MultiOut) and are indexed by unrolled constants only (a run-time index would put the arrays into scratch).  The host
// passes arrays of m pointers to one launch_* helper per pass, which resolves NQ and m to an instance.
// ALIASING: distinct columns never alias, but the qualifier __restrict__ cannot sit on the elements of a by-value array,
// so the kernels order their memory operations by hand: a row-per-wave pass issues every load of the wave (all K columns'
// rows, their right-hand sides, then the coefficients) before its first store; a marching pass issues all loads of a
// row before that row's stores.  A store between two columns' loads would order them.
#pragma once

#include "mgx_kernels.hpp"

#include <type_traits>

namespace mgx {

template <typename T> struct Lanes { T a[VecOf<T>::W]; };
__device__ __forceinline__ Lanes<double> to_lanes(const double2& v) { return Lanes<double>{{v.x, v.y}}; }
__device__ __forceinline__ Lanes<float> to_lanes(const float4& v) { return Lanes<float>{{v.x, v.y, v.z, v.w}}; }
__device__ __forceinline__ double2 from_lanes(const Lanes<double>& l) { return make_double2(l.a[0], l.a[1]); }
__device__ __forceinline__ float4 from_lanes(const Lanes<float>& l) { return make_float4(l.a[0], l.a[1], l.a[2], l.a[3]); }

template <typename T> struct Op9 { const T* a[9]; };     // c, n, s, w, e, nw, ne, sw, se (corners null on five-point levels)
template <typename T> struct Op9Out { T* a[9]; };

constexpr int kMultiMax = 4;                              // MGX_MAX_RHS
template <typename T, int K> struct MultiIn { const T* p[K]; };          // the K columns of a launch
template <typename T, int K> struct MultiOut { T* p[K]; };

// storage slot of the coefficient that points at (dy, dx)
__host__ __device__ constexpr int op9_slot(int dy, int dx)
{
    return dy < 0 ? (dx < 0 ? 5 : dx == 0 ? 1 : 6) : dy == 0 ? (dx < 0 ? 3 : dx == 0 ? 0 : 4) : (dx < 0 ? 7 : dx == 0 ? 2 : 8);
}

// slots q0 .. NQ - 1 of an operator at a lane's columns
template <int NQ, int Q0, typename T>
__device__ __forceinline__ void load_coefs(const Op9<T>& op, long at, bool pred, Lanes<T> (&k)[9])
{
    using V = typename VecOf<T>::type;
#pragma unroll
    for (int q = Q0; q < NQ; ++q) k[q] = to_lanes(vload<V>(op.a[q] + at, pred));
}

// what a lane's W points read of the iterate: its own vectors of the three rows (u = up, c = current, d = down) and,
// from the adjacent lanes, the element left (l) of its first and right (r) of its last column in each row.  A five-point
// sum reads cl and cr only
template <typename T> struct Rows3 { Lanes<T> up, cur, dn; T ul, ur, cl, cr, dl, dr; };

// sum_k coef_k * neighbour_k in CSR order, one IEEE multiplication and one addition per term, the first term present
// starting the accumulator.  k: the coefficients in slot order; `centre` is the coefficient of the point itself (an
// array element for A, the scalar 1 - omega for R_omega: slot 0 of k is not read here)
template <int NQ, typename T, typename CF>
__device__ __forceinline__ Lanes<T> stencil_sum(const Rows3<T>& u, const Lanes<T> (&k)[9], CF centre)
{
    static_assert(NQ == 5 || NQ == 9, "five- or nine-point operators");
    constexpr int W = VecOf<T>::W;
    Lanes<T> o;
#pragma unroll
    for (int x = 0; x < W; ++x) {
        const int xl = x == 0 ? 0 : x - 1, xr = x == W - 1 ? x : x + 1;
        const T nb[3][3] = {{x == 0 ? u.ul : u.up.a[xl], u.up.a[x], x == W - 1 ? u.ur : u.up.a[xr]},
                            {x == 0 ? u.cl : u.cur.a[xl], u.cur.a[x], x == W - 1 ? u.cr : u.cur.a[xr]},
                            {x == 0 ? u.dl : u.dn.a[xl], u.dn.a[x], x == W - 1 ? u.dr : u.dn.a[xr]}};
        T acc = (T)0;
        bool started = false;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if constexpr (NQ == 5) { if (dy != 0 && dx != 0) continue; }
                const T term = ((dy == 0 && dx == 0) ? centre(x) : k[op9_slot(dy, dx)].a[x]) * nb[1 + dy][1 + dx];
                acc = started ? acc + term : term;
                started = true;
            }
        o.a[x] = acc;
    }
    return o;
}

// the tile of a wave in a one-row-per-wave pass over rows [row_lo, row_hi): `at` the offset of the lane's vector in row
// row_lo + chunk, `in` the predicate of every load at `at`, `st` that of the stores, up / cur / dn the iterate around it.
// A wave without a tile (active = false) loads nothing: all its predicates are false
template <typename T> struct RowTile {
    using V = typename VecOf<T>::type;
    bool active, in, st;
    long at, col;
    V up, cur, dn;
};

template <typename T>
__device__ __forceinline__ RowTile<T> load_rows(const T* __restrict__ vin, int N, long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    const Tile t = wave_tile(strips, row_hi - row_lo);
    const Cols c = lane_cols<VecOf<T>::W>(t.strip, N, pitch);
    const int row = row_lo + t.chunk;
    const bool ld = c.ld && t.active;
    RowTile<T> r;
    r.active = t.active;
    r.col = c.col;
    r.at = c.col + (long)row * pitch;
    r.in = ld && row >= 0 && row < rows_alloc;
    r.st = c.st && r.in;
    r.up = vload<V>(vin + r.at - pitch, ld && row >= 1 && row <= rows_alloc);
    r.cur = vload<V>(vin + r.at, r.in);
    r.dn = vload<V>(vin + r.at + pitch, ld && row >= -1 && row + 1 < rows_alloc);
    return r;
}

// the three rows of a tile with their edge values from the adjacent lanes; NQ = 5 issues the DPP moves of the current
// row only.  Called after the pass's other loads have been issued
template <int NQ, typename T>
__device__ __forceinline__ Rows3<T> rows_of(const RowTile<T>& t)
{
    Rows3<T> u{to_lanes(t.up), to_lanes(t.cur), to_lanes(t.dn)};
    if constexpr (NQ == 9) { u.ul = from_left(last(t.up)); u.ur = from_right(first(t.up)); }
    u.cl = from_left(last(t.cur)); u.cr = from_right(first(t.cur));
    if constexpr (NQ == 9) { u.dl = from_left(last(t.dn)); u.dr = from_right(first(t.dn)); }
    return u;
}

template <typename T> __device__ __forceinline__ Lanes<T> load_lanes(const T* p, bool pred)
{
    return to_lanes(vload<typename VecOf<T>::type>(p, pred));
}
// a lane's W results as a vector, columns 0 and >= N zero; store_row: into the lane's columns of the tile's row
template <typename T> __device__ __forceinline__ typename VecOf<T>::type masked_row(const Lanes<T>& o, const RowTile<T>& t, int N)
{
    typename VecOf<T>::type ov = from_lanes(o);
    mask_cols(ov, t.col, N);
    return ov;
}
template <typename T> __device__ __forceinline__ void store_row(T* out, const Lanes<T>& o, const RowTile<T>& t, int N)
{
    vstore<typename VecOf<T>::type>(out + t.at, masked_row(o, t, N), t.st);
}

// MF:86-90: the Jacobi value J(v) = R_omega v + omega (D_inv b) of one point, p1 = (R_omega v) there
template <typename T> __device__ __forceinline__ T jacobi_value(T p1, T omega, T dinv, T b) { return p1 + omega * (dinv * b); }

// MF:75-96: one sweep of v_j' = J(v_j) = R_omega v_j + omega D^-1 b_j on K columns, out of place; rows [row_lo, row_hi).
// r: the off-diagonals of R_omega in slots 1 .. NQ - 1 (its diagonal is the scalar rc = 1 - omega)
template <typename T, int NQ, int K>
__global__ void __launch_bounds__(kBlock)
k_jacobi_var(MultiIn<T, K> vin, MultiIn<T, K> rhs, MultiOut<T, K> vout, const T* __restrict__ dinv, Op9<T> r,
             int N, long pitch, int row_lo, int row_hi, int strips, T rc, T omega, int rows_alloc)
{
    constexpr int W = VecOf<T>::W;
    RowTile<T> t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = load_rows<T>(vin.p[j], N, pitch, row_lo, row_hi, strips, rows_alloc);
    if (!t[0].active) return;
    Lanes<T> b[K];
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = load_lanes(rhs.p[j] + t[0].at, t[0].in);
    const Lanes<T> d = load_lanes(dinv + t[0].at, t[0].in);
    Lanes<T> k[9];
    load_coefs<NQ, 1>(r, t[0].at, t[0].in, k);
    Lanes<T> o[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const Lanes<T> p1 = stencil_sum<NQ>(rows_of<NQ>(t[j]), k, [&](int) { return rc; });                                     // MF:86
#pragma unroll
        for (int x = 0; x < W; ++x) o[j].a[x] = jacobi_value(p1.a[x], omega, d.a[x], b[j].a[x]);                               // MF:88, 90
    }
#pragma unroll
    for (int j = 0; j < K; ++j) store_row(vout.p[j], o[j], t[j], N);
}

// the sum of the squares of a lane's W values, in double, pairwise
template <typename T> __device__ __forceinline__ double lane_squares(const Lanes<T>& q)
{
    if constexpr (VecOf<T>::W == 2) return (double)q.a[0] * (double)q.a[0] + (double)q.a[1] * (double)q.a[1];
    else return ((double)q.a[0] * (double)q.a[0] + (double)q.a[1] * (double)q.a[1]) +
                ((double)q.a[2] * (double)q.a[2] + (double)q.a[3] * (double)q.a[3]);
}

// MF:150-153: r_j = b_j - A v_j on K columns.  MODE 0: out.p[j] = r_j;  MODE 1: partial.p[j][block] = the block's sum of
// r_j^2 (the norm the solve reports), the same points in the same order whatever K is
template <typename T, int NQ, int MODE, int K>
__global__ void __launch_bounds__(kBlock)
k_residual_var(MultiIn<T, K> vin, MultiIn<T, K> rhs, MultiOut<T, K> out, MultiOut<double, K> partial, Op9<T> a,
               int N, long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[K][kWavesPerBlock];
    RowTile<T> t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = load_rows<T>(vin.p[j], N, pitch, row_lo, row_hi, strips, rows_alloc);
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    if (t[0].active) {
        Lanes<T> b[K];
#pragma unroll
        for (int j = 0; j < K; ++j) b[j] = load_lanes(rhs.p[j] + t[0].at, t[0].in);
        Lanes<T> k[9];
        load_coefs<NQ, 0>(a, t[0].at, t[0].in, k);
        V ov[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const Lanes<T> av = stencil_sum<NQ>(rows_of<NQ>(t[j]), k, [&](int x) { return k[0].a[x]; });
            Lanes<T> o;
#pragma unroll
            for (int x = 0; x < W; ++x) o.a[x] = b[j].a[x] - av.a[x];
            ov[j] = masked_row(o, t[j], N);
            // one column squares its residual here, K > 1 in the loop below: the same sums either way, but the compiler
            // makes the float K = 1 norm pass wait for every load when the squares follow in a second loop (9 and 14
            // s_waitcnt vmcnt against 2, 2.7 % slower at 4096^2), and taking them here for K > 1 would change the
            // registers of those instances
            if constexpr (MODE != 0 && K == 1) { if (t[j].st) acc[j] = lane_squares(to_lanes(ov[j])); }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (MODE == 0) vstore<V>(out.p[j] + t[j].at, ov[j], t[j].st);
            else if (K > 1 && t[j].st) acc[j] = lane_squares(to_lanes(ov[j]));
        }
    }
    if (MODE != 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) block_reduce<kWavesPerBlock>(acc[j], wsum[j], partial.p[j] + blockIdx.x, ReduceSum{});
    }
}

// MF:122-130: coarse(I, J) = wgt * fine(2I, 2J); optionally zero the coarse guess (PS:613) in the same pass
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_restrict_inject(const T* __restrict__ fine, T* __restrict__ coarse, T* __restrict__ coarse_zero, int NC, long pitch,
                  long cpitch, T wgt)
{
    const int J = blockIdx.x * blockDim.x + threadIdx.x;
    const int I = blockIdx.y + 1;
    if (J < 1 || J >= NC || I >= NC) return;
    coarse[(long)I * cpitch + J] = wgt * fine[(long)(2 * I) * pitch + 2 * J];
    if (coarse_zero) coarse_zero[(long)I * cpitch + J] = (T)0;
}

// A_jacobi_sp_dict[level] from A_sp_dict[level] (MF:28-32): D_inv = 1 / c into slot 0 of j, R_x = -(omega (D_inv a_x))
// for the off-diagonals into slots 1 .. NQ - 1; the diagonal of R_omega is 1 - omega exactly (D^-1 A has a unit diagonal)
// and is not stored
template <typename T, int NQ>
__global__ void k_var_build_jacobi(Op9<T> a, Op9Out<T> j, int N, long pitch, T omega)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c < 1 || c >= N || r < 1 || r >= N) return;
    const long at = (long)r * pitch + c;
    const T d = (T)1 / a.a[0][at];
    j.a[0][at] = d;
#pragma unroll
    for (int q = 1; q < NQ; ++q) j.a[q][at] = -(omega * (d * a.a[q][at]));
}

// -div(a grad u) on a level from the nodal coefficient of the finest grid (rows 0..Nf of Nf + 1 doubles),
// sampled at the level's nodes (stride q); face coefficient = mean of its two nodes (oracle: stencil_from_nodes)
template <typename T>
__global__ void k_var_from_nodes(const double* __restrict__ a, int Nf, int q, Op9Out<T> o, int N, long pitch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c < 1 || c >= N || r < 1 || r >= N) return;
    const long ld = (long)Nf + 1;
    auto node = [&](int i, int j) { return a[(long)(i * q) * ld + (long)(j * q)]; };
    const double ctr = node(r, c);
    const double fn = 0.5 * (ctr + node(r - 1, c)), fs = 0.5 * (ctr + node(r + 1, c));
    const double fw = 0.5 * (ctr + node(r, c - 1)), fe = 0.5 * (ctr + node(r, c + 1));
    const long at = (long)r * pitch + c;
    o.a[0][at] = (T)(((fn + fw) + fe) + fs);
    o.a[1][at] = (T)(-fn); o.a[2][at] = (T)(-fs); o.a[3][at] = (T)(-fw); o.a[4][at] = (T)(-fe);
}

// -d_x(axx d_x u) - d_y(ayy d_y u) - d_x(axy d_y u) - d_y(axy d_x u) on the finest level from the three nodal
// coefficients of its own grid (rows 0..N of N + 1 doubles each; x along a row, y grows with the row index): the
// five-point part is k_var_from_nodes' with ayy on the n / s faces and axx on the w / e faces; the mixed term is the
// central difference of central differences, a corner coefficient = a quarter of the sum of axy at the two edge
// neighbours it lies between, negative towards nw and se (tests/nine_ref.py: tensor9).  The four corners of a point sum
// to zero; e(i,j) = w(i,j+1), se(i,j) = nw(i+1,j+1), ne(i,j) = sw(i-1,j+1) bit for bit.  All in double, one rounding to T
template <typename T>
__global__ void k_var_from_tensor(const double* __restrict__ axx, const double* __restrict__ axy, const double* __restrict__ ayy,
                                  Op9Out<T> o, int N, long pitch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c < 1 || c >= N || r < 1 || r >= N) return;
    const long ld = (long)N + 1;
    const long nd = (long)r * ld + c;
    const double fn = 0.5 * (ayy[nd] + ayy[nd - ld]), fs = 0.5 * (ayy[nd] + ayy[nd + ld]);
    const double fw = 0.5 * (axx[nd] + axx[nd - 1]), fe = 0.5 * (axx[nd] + axx[nd + 1]);
    const double aN = axy[nd - ld], aS = axy[nd + ld], aW = axy[nd - 1], aE = axy[nd + 1];
    const long at = (long)r * pitch + c;
    o.a[0][at] = (T)(((fn + fw) + fe) + fs);
    o.a[1][at] = (T)(-fn); o.a[2][at] = (T)(-fs); o.a[3][at] = (T)(-fw); o.a[4][at] = (T)(-fe);
    o.a[5][at] = (T)(-(0.25 * (aW + aN))); o.a[6][at] = (T)(0.25 * (aE + aN));
    o.a[7][at] = (T)(0.25 * (aW + aS)); o.a[8][at] = (T)(-(0.25 * (aE + aS)));
}

// ---- direct bottom solve of a general coarsest operator (MF:63-72, 137-139) ---------------------------------
// Dense inverse of the n^2 x n^2 matrix by Gauss-Jordan elimination without pivoting (diagonally dominant
// M-matrices), in double whatever the hierarchy's type: two launches per pivot at set-up time, one matvec per
// solve.  Every element update is its own IEEE operations in the oracle's order (orc_dense_inverse): same bits.

// the coarsest operator as a dense matrix (and the identity next to it) for k_gj_prow / k_gj_elim
template <typename T, int NQ>
__global__ void k_var_dense_fill(double* __restrict__ M, double* __restrict__ Inv, Op9<T> a, int n, long pitch)
{
    const int NN = n * n;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;      // column
    const int k = blockIdx.y;                                  // row = unknown (ri, rj)
    if (j >= NN) return;
    const int ri = k / n, rj = k - ri * n;
    const int ci = j / n, cj = j - ci * n;
    const int dy = ci - ri, dx = cj - rj;
    double v = 0.0;
    if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1 && (NQ == 9 || dy == 0 || dx == 0))
        v = (double)a.a[op9_slot(dy, dx)][(long)(ri + 1) * pitch + (rj + 1)];
    M[(long)k * NN + j] = v;
    Inv[(long)k * NN + j] = (j == k) ? 1.0 : 0.0;
}
static __global__ void k_gj_prow(const double* __restrict__ M, const double* __restrict__ Inv, double* __restrict__ pm,
                                 double* __restrict__ pi, int NN, int k)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= NN) return;
    const double p = M[(long)k * NN + k];
    pm[j] = M[(long)k * NN + j] / p;
    pi[j] = Inv[(long)k * NN + j] / p;
}
// one workgroup per row: every thread reads the row's multiplier before any thread overwrites it
static __global__ void k_gj_elim(double* __restrict__ M, double* __restrict__ Inv, const double* __restrict__ pm,
                                 const double* __restrict__ pi, int NN, int k)
{
    const int i = blockIdx.x;
    double* mi = M + (long)i * NN;
    double* ii = Inv + (long)i * NN;
    const double f = mi[k];
    __syncthreads();
    for (int j = threadIdx.x; j < NN; j += blockDim.x) {
        if (i == k) { mi[j] = pm[j]; ii[j] = pi[j]; }
        else { mi[j] = mi[j] - f * pm[j]; ii[j] = ii[j] - f * pi[j]; }
    }
}
// x_j = Inv b_j on the coarsest grid, K columns: one thread per unknown, every element of Inv read once, each column's
// row sum in order (deterministic, n^2 <= 961 terms)
template <typename T, int K>
__global__ void k_var_dense_solve(const double* __restrict__ Inv, MultiIn<T, K> b, MultiOut<T, K> x, int n, long pitch)
{
    const int NN = n * n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NN) return;
    const double* row = Inv + (long)i * NN;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for (int q = 0; q < NN; ++q) {
        const int bi = q / n, bj = q - bi * n;
        const double m = row[q];
        const long at = (long)(bi + 1) * pitch + (bj + 1);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += m * (double)b.p[j][at];
    }
    const int ri = i / n, rj = i - ri * n;
#pragma unroll
    for (int j = 0; j < K; ++j) x.p[j][(long)(ri + 1) * pitch + (rj + 1)] = (T)acc[j];
}

// ---- host side -----------------------------------------------------------------------------------------------
// what a launch needs of a level: the operator a, its D_inv and the off-diagonals r of R_omega (slots 1 .. 8; both
// with null corners on five-point levels)
template <typename T> struct VarLevel {
    Op9<T> a, r;
    const T* dinv;
    bool nine;
    int N, rows;
    long pitch;
};

// f(double{}) or f(float{}): the working type as a tag
template <typename F> void with_float_type(bool f64, F&& f) { if (f64) f(double{}); else f(float{}); }
// f(tag) with decltype(tag)::value == 9 or 5: the point count NQ of a level's operator as a compile-time constant
template <typename F> void with_point_count(bool nine, F&& f)
{
    if (nine) f(std::integral_constant<int, 9>{}); else f(std::integral_constant<int, 5>{});
}

// f(tag) with decltype(tag)::value == k, MIN <= k <= MAX: a count (of columns, mostly) as a compile-time constant
template <int MAX, int MIN = 1, typename F> void with_count(int k, F&& f)
{
    if constexpr (MAX > MIN) {
        if (k < MAX) { with_count<MAX - 1, MIN>(k, f); return; }
    }
    f(std::integral_constant<int, MAX>{});
}

// the first K pointers of a host array as kernel arguments (p null: K null pointers)
template <int K, typename T> MultiIn<T, K> columns_in(const T* const* p)
{
    MultiIn<T, K> o;
    for (int j = 0; j < K; ++j) o.p[j] = p[j];
    return o;
}
template <int K, typename T> MultiOut<T, K> columns_out(T* const* p)
{
    MultiOut<T, K> o;
    for (int j = 0; j < K; ++j) o.p[j] = p ? p[j] : nullptr;
    return o;
}

// ---- the launches of the passes above: m = 1 .. kMultiMax columns as host arrays of m pointers, one wave per row and strip ----
// one sweep vout_j = J(vin_j) with the right-hand sides rhs_j
template <typename T>
void launch_jacobi_var(const VarLevel<T>& v, int m, const T* const* vin, const T* const* rhs, T* const* vout, T rc, T omega, hipStream_t st)
{
    const Launch g = make_launch(v.N, VecOf<T>::W, v.N - 1, 1);
    with_point_count(v.nine, [&](auto nq) {
        with_count<kMultiMax>(m, [&](auto kc) {
            constexpr int NQ = decltype(nq)::value, K = decltype(kc)::value;
            hipLaunchKernelGGL((k_jacobi_var<T, NQ, K>), dim3(g.blocks), dim3(kBlock), 0, st, columns_in<K>(vin), columns_in<K>(rhs),
                               columns_out<K>(vout), v.dinv, v.r, v.N, v.pitch, 1, v.N, g.strips, rc, omega, v.rows);
        });
    });
}

// MODE 0: out_j = rhs_j - A vin_j;  MODE 1: sums[j][0] = the sum of its squares through partial[j] (one double per
// workgroup of the pass), each column reduced by its own k_reduce_partials
template <typename T, int MODE>
void launch_residual_var(const VarLevel<T>& v, int m, const T* const* vin, const T* const* rhs, T* const* out, double* const* partial,
                         double* const* sums, hipStream_t st)
{
    const Launch g = make_launch(v.N, VecOf<T>::W, v.N - 1, 1);
    with_point_count(v.nine, [&](auto nq) {
        with_count<kMultiMax>(m, [&](auto kc) {
            constexpr int NQ = decltype(nq)::value, K = decltype(kc)::value;
            hipLaunchKernelGGL((k_residual_var<T, NQ, MODE, K>), dim3(g.blocks), dim3(kBlock), 0, st, columns_in<K>(vin), columns_in<K>(rhs),
                               columns_out<K>(out), columns_out<K>(partial), v.a, v.N, v.pitch, 1, v.N, g.strips, v.rows);
        });
    });
    if (MODE == 1)
        for (int j = 0; j < m; ++j) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, partial[j], g.blocks, sums[j]);
}

// x_j = inv b_j on the n x n unknowns of the coarsest level
template <typename T>
void launch_var_dense_solve(const double* inv, int m, const T* const* b, T* const* x, int n, long pitch, hipStream_t st)
{
    with_count<kMultiMax>(m, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        hipLaunchKernelGGL((k_var_dense_solve<T, K>), dim3((n * n + 63) / 64), dim3(64), 0, st, inv, columns_in<K>(b), columns_out<K>(x), n, pitch);
    });
}

} // namespace mgx
