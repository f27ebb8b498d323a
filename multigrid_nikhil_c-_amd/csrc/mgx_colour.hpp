// mgx_colour.hpp - multicolour Gauss-Seidel smoothing for the general-operator hierarchies (cfg.smoother =
// MGX_SMOOTHER_COLOR_GS / COLOR_SGS with op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN): the standard point
// smoother, about twice the smoothing of a damped Jacobi sweep per pass over the coefficients.  tests/colour_ref.py
// states everything below in numpy, operation by operation.
//
// THE SWEEP.  The points of a level are split into colours such that no point has a neighbour of its own colour; a
// sweep updates the colours one after the other, every point of a colour from the current state of its neighbours:
//     x_ij = (b_ij - S_ij) * D_inv_ij,      S_ij = sum of the off-diagonal terms a_k u_k of A (not of R_omega)
// in the CSR order of stencil_sum with the centre left out (NW, N, NE, W, E, SW, S, SE; five-point: N, W, E, S), the
// first term starting the accumulator, every product and sum rounded on its own (-ffp-contract=off).  D_inv is the
// level's stored 1 / c (slot 0 of the Jacobi splitting).  Coefficients that point at the Dirichlet ring are read and
// multiplied by the ring of the iterate, which is zero (the rule of k_residual_var).  No damping: cfg.omega is not used.
//   five-point level (NQ = 5), two colours: colour 0 = the points with (grid row + grid column) even, then colour 1
//                    (odd) - the oracle's convention for its Poisson red-black sweep (red = even first);
//   nine-point level (NQ = 9), four colours by (row parity, column parity) of the grid indices, in the order
//                    (odd, odd), (odd, even), (even, odd), (even, even): the points that are not coarse points first,
//                    the coarse points last, as the zebra sweeps take the odd lines first.
// A REVERSE sweep takes the colours in the opposite order with the same update.  MGX_SMOOTHER_COLOR_GS sweeps forward in
// every block; MGX_SMOOTHER_COLOR_SGS sweeps forward in the blocks before a restriction (and in mgx_smooth,
// mgx_time_smoother and the first mu1 sweeps of a bottom = SMOOTH visit) and in reverse in the blocks after a
// correction (and the last mu2 sweeps of a bottom = SMOOTH visit), which makes the cycle a symmetric preconditioner.
//
// TWO KERNEL FORMS.
//   k_gs_colour<T, NQ>  one colour, in place; the geometry of k_jacobi_var: one wave per row and strip, 16-byte lanes,
//             the row's x-neighbours by DPP.  The columns of a vector start at an even grid column, so the elements a
//             launch updates are those of one element parity, the same for every lane of a wave.  A five-point launch
//             covers all interior rows (the parity alternates with the row), a nine-point launch the rows of the colour's
//             row parity (half the waves).  A lane stores its whole vector: the other elements carry the values just
//             loaded, which no wave of the launch writes.  A sweep is 2 (NQ = 5) or 4 (NQ = 9) launches; every launch
//             fetches b, D_inv and the coefficient lines of its rows in full for half of their points:
//             2 (NQ + 3) sizeof(T) per point and sweep on five-point levels (16), 2 (NQ + 3) on nine-point ones too (24:
//             four launches over half the rows each).  Works on every level down to N = 4.
//   k_gs_rb<T>  both colours of a five-point sweep in one launch, out of place (u -> tmp, swapped like a Jacobi pass).  A
//             wave takes gs_chunk_rows(N) consecutive rows of a strip and marches down them with a rolling window in
//             registers: as the old row r + 2 arrives, the first colour of row r + 1 is computed from the old rows r, r + 1,
//             r + 2, then the second colour of row r from the first-colour rows r - 1, r, r + 1, and row r is stored.  The
//             first-colour values of the row above and the row below the chunk (and of the halo lanes' columns) are
//             recomputed from the old iterate: the same expression on the same inputs, so the same bits, and the result
//             is bit-identical to two k_gs_colour launches, forward and reverse alike.  v, b, D_inv and the four
//             coefficient grids come in once and v' goes out once: 8 sizeof(T) per point and sweep, the bytes of a
//             Jacobi sweep, plus 2 / R of the seven input grids for the two recomputed rows of a chunk of R rows
//             (R = 16: + 11 %).  Levels with fewer interior rows than a chunk (N < 16) use the per-colour form, as does
//             every five-point level of a handle created under MGX_GS_FUSED=0.
// NINE-POINT LEVELS STAY UNFUSED: with four colours the last colour of row r depends on the first colour three rows on,
// a dependency depth of four rows; the window of such a pass holds four states of the iterate and three rows of
// eleven input grids, beyond a wave's registers at a useful occupancy.
// No atomics and no reductions: two runs give the same bits, and so do graph replay and MGX_GRAPH=0.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

// b, D_inv and the off-diagonals of A (slots 1 .. NQ - 1) at a lane's columns of one row
template <typename T> struct GsRow { Lanes<T> b, d, k[9]; };

template <int NQ, typename T>
__device__ __forceinline__ GsRow<T> load_gs_row(const T* __restrict__ rhs, const T* __restrict__ dinv, const Op9<T>& a, long at, bool pred)
{
    GsRow<T> g;
    g.b = load_lanes(rhs + at, pred);
    g.d = load_lanes(dinv + at, pred);
    load_coefs<NQ, 1>(a, at, pred, g.k);
    return g;
}

// the three rows of the iterate around a lane's columns with their edge values from the adjacent lanes
template <int NQ, typename T>
__device__ __forceinline__ Rows3<T> rows_of(const Lanes<T>& up, const Lanes<T>& cur, const Lanes<T>& dn)
{
    constexpr int W = VecOf<T>::W;
    Rows3<T> u{up, cur, dn};
    if constexpr (NQ == 9) { u.ul = from_left(up.a[W - 1]); u.ur = from_right(up.a[0]); }
    u.cl = from_left(cur.a[W - 1]); u.cr = from_right(cur.a[0]);
    if constexpr (NQ == 9) { u.dl = from_left(dn.a[W - 1]); u.dr = from_right(dn.a[0]); }
    return u;
}

// stencil_sum without the centre: sum of a_k u_k over the neighbours in CSR order, the first term starting the accumulator
template <int NQ, typename T>
__device__ __forceinline__ Lanes<T> offdiag_sum(const Rows3<T>& u, const Lanes<T> (&k)[9])
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
                if (dy == 0 && dx == 0) continue;
                if constexpr (NQ == 5) { if (dy != 0 && dx != 0) continue; }
                const T term = k[op9_slot(dy, dx)].a[x] * nb[1 + dy][1 + dx];
                acc = started ? acc + term : term;
                started = true;
            }
        o.a[x] = acc;
    }
    return o;
}

// one colour of one row at a lane's columns [col, col + W): the elements of parity wp (col is even, so the parity of an
// element is that of its grid column) that are unknowns (1 <= column < N, row_in) get (b - S) D_inv, the others keep cur.
// Both kernel forms update through this one function: same expression, same bits
template <int NQ, typename T>
__device__ __forceinline__ Lanes<T> gs_colour_row(const Lanes<T>& up, const Lanes<T>& cur, const Lanes<T>& dn, const GsRow<T>& g, int wp,
                                                  long col, int N, bool row_in)
{
    constexpr int W = VecOf<T>::W;
    const Lanes<T> S = offdiag_sum<NQ>(rows_of<NQ>(up, cur, dn), g.k);
    Lanes<T> o;
#pragma unroll
    for (int x = 0; x < W; ++x) {
        const bool upd = row_in && (x & 1) == wp && col + x >= 1 && col + x < N;
        o.a[x] = upd ? (g.b.a[x] - S.a[x]) * g.d.a[x] : cur.a[x];
    }
    return o;
}

// one colour, in place.  Wave q of the launch takes grid row row0 + rstep q (nrows of them).  NQ = 5: par is the colour,
// the elements updated in a row have parity (par + row) & 1;  NQ = 9: par is the colour's column parity
template <typename T, int NQ>
__global__ void __launch_bounds__(kBlock)
k_gs_colour(T* __restrict__ v, const T* __restrict__ rhs, const T* __restrict__ dinv, Op9<T> a, int N, long pitch, int row0, int rstep,
            int nrows, int strips, int par)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const Tile t = wave_tile(strips, nrows);
    if (!t.active) return;
    const Cols c = lane_cols<W>(t.strip, N, pitch);
    const int row = row0 + rstep * t.chunk;
    if (row < 1 || row >= N) return;                          // (wave-uniform; rows row - 1 .. row + 1 are inside the arrays)
    const long at = c.col + (long)row * pitch;
    const Lanes<T> up = load_lanes(v + at - pitch, c.ld), cur = load_lanes(v + at, c.ld), dn = load_lanes(v + at + pitch, c.ld);
    const GsRow<T> g = load_gs_row<NQ>(rhs, dinv, a, at, c.ld);
    const int wp = NQ == 5 ? ((par + row) & 1) : par;
    const Lanes<T> o = gs_colour_row<NQ>(up, cur, dn, g, wp, c.col, N, true);
    vstore<V>(v + at, from_lanes(o), c.st);
}

// rows per chunk of k_gs_rb on a level of N intervals, and whether the level has a chunk's worth of rows at all
inline int gs_chunk_rows(int N) { return N >= 1024 ? 16 : 8; }
inline bool gs_fused_level(int N) { return N - 1 >= gs_chunk_rows(N); }

// both colours of a five-point sweep, out of place: vout = second(first(vin)) on rows [1, N), `first` the colour taken
// first (0: a forward sweep, 1: a reverse one).  Wave (chunk, strip) takes rows [1 + chunk R, min(1 + (chunk + 1) R, N))
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_gs_rb(const T* __restrict__ vin, const T* __restrict__ rhs, T* __restrict__ vout, const T* __restrict__ dinv, Op9<T> a, int N, long pitch,
        int R, int strips, int chunks, int first)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const Tile t = wave_tile(strips, chunks);
    if (!t.active) return;
    const Cols c = lane_cols<W>(t.strip, N, pitch);
    const int r0 = 1 + t.chunk * R;
    const int r1 = min(r0 + R, N);
    const T* pv = vin + c.col;

    // a row y of the iterate is read iff 0 <= y <= N; it has b, D_inv and coefficients iff it is an unknown row
    auto row_in = [&](int y) { return y >= 1 && y < N; };
    auto old_row = [&](int y) { return load_lanes(pv + (long)y * pitch, c.ld && y >= 0 && y <= N); };
    auto gs_row = [&](int y) { return load_gs_row<5>(rhs, dinv, a, c.col + (long)y * pitch, c.ld && row_in(y)); };
    // H(y): row y after the first colour, from the old rows y - 1, y, y + 1 (the ring rows stay what they are: zero)
    auto first_colour = [&](const Lanes<T>& u, const Lanes<T>& m, const Lanes<T>& d, const GsRow<T>& g, int y) {
        return gs_colour_row<5>(u, m, d, g, (first + y) & 1, c.col, N, row_in(y));
    };

    // the window at row r: A = H(r - 1), B = H(r), O0 / O1 / O2 = old rows r, r + 1, r + 2, gcur / gnext = the inputs
    // of rows r and r + 1; old row r + 3 and the inputs of row r + 2 are in flight
    Lanes<T> O0 = old_row(r0), O1 = old_row(r0 + 1), O2 = old_row(r0 + 2);
    GsRow<T> gcur = gs_row(r0), gnext = gs_row(r0 + 1);
    Lanes<T> A, B;
    {
        const Lanes<T> Om2 = old_row(r0 - 2), Om1 = old_row(r0 - 1);
        const GsRow<T> gm1 = gs_row(r0 - 1);
        A = first_colour(Om2, Om1, O0, gm1, r0 - 1);
        B = first_colour(Om1, O0, O1, gcur, r0);
    }
    for (int r = r0; r < r1; ++r) {
        const bool more = r + 1 < r1;
        const Lanes<T> O3 = load_lanes(pv + (long)(r + 3) * pitch, c.ld && more && r + 3 <= N);
        const GsRow<T> gnext2 = load_gs_row<5>(rhs, dinv, a, c.col + (long)(r + 2) * pitch, c.ld && more && row_in(r + 2));
        const Lanes<T> Cn = first_colour(O0, O1, O2, gnext, r + 1);                               // H(r + 1)
        const Lanes<T> o = gs_colour_row<5>(A, B, Cn, gcur, (first + r + 1) & 1, c.col, N, true);  // the second colour of row r
        vstore<V>(vout + c.col + (long)r * pitch, from_lanes(o), c.st);
        A = B; B = Cn; O0 = O1; O1 = O2; O2 = O3; gcur = gnext; gnext = gnext2;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------
// what a launch needs of a level: the operator and its D_inv
template <typename T> struct ColourLevel {
    Op9<T> a;
    const T* dinv;
    bool nine;
    int N;
    long pitch;
};

// one sweep of v in place, one launch per colour.  Returns the launches made
template <typename T>
int launch_gs_colours(const ColourLevel<T>& l, T* v, const T* b, bool reverse, hipStream_t st)
{
    int launches = 0;
    auto colour = [&](auto nq, int row0, int rstep, int nrows, int par) {
        constexpr int NQ = decltype(nq)::value;
        if (nrows <= 0) return;
        const Launch g = make_launch(l.N, VecOf<T>::W, nrows, 1);
        hipLaunchKernelGGL((k_gs_colour<T, NQ>), dim3(g.blocks), dim3(kBlock), 0, st, v, b, l.dinv, l.a, l.N, l.pitch, row0, rstep, nrows,
                           g.strips, par);
        ++launches;
    };
    if (!l.nine) {
        for (int i = 0; i < 2; ++i) colour(std::integral_constant<int, 5>{}, 1, 1, l.N - 1, reverse ? 1 - i : i);
    } else {
        // (row parity, column parity): (odd, odd), (odd, even), (even, odd), (even, even); odd rows 1, 3, .. N - 1,
        // even rows 2, 4, .. N - 2
        for (int i = 0; i < 4; ++i) {
            const int k = reverse ? 3 - i : i;
            const int rp = k < 2 ? 1 : 0, cp = (k & 1) ? 0 : 1;
            colour(std::integral_constant<int, 9>{}, rp ? 1 : 2, 2, rp ? l.N / 2 : l.N / 2 - 1, cp);
        }
    }
    return launches;
}

// one sweep of a five-point level with gs_fused_level(N), vin -> vout, one launch
template <typename T>
void launch_gs_rb(const ColourLevel<T>& l, const T* vin, const T* b, T* vout, bool reverse, hipStream_t st)
{
    const Launch g = make_launch(l.N, VecOf<T>::W, l.N - 1, gs_chunk_rows(l.N));
    hipLaunchKernelGGL((k_gs_rb<T>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, l.dinv, l.a, l.N, l.pitch, g.R, g.strips, g.chunks,
                       reverse ? 1 : 0);
}

// mgx.hip declares these instantiations; mgx_inst.hip (-DMGX_INST_KIND=7) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template int launch_gs_colours<double>(const ColourLevel<double>&, double*, const double*, bool, hipStream_t);
extern template int launch_gs_colours<float>(const ColourLevel<float>&, float*, const float*, bool, hipStream_t);
extern template void launch_gs_rb<double>(const ColourLevel<double>&, const double*, const double*, double*, bool, hipStream_t);
extern template void launch_gs_rb<float>(const ColourLevel<float>&, const float*, const float*, float*, bool, hipStream_t);
#endif

} // namespace mgx
