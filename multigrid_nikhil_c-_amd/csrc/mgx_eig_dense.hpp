// mgx_eig_dense.hpp - the small dense part of mgx_eigs' Rayleigh-Ritz step (mgx_eig_host.hpp), in plain C++ with no HIP
// so that a CPU program can include and test it (tests/test_eig_cpu.py compiles it under -fsanitize=address,undefined).
//
// rayleigh_ritz(n, nev, G, H, theta, C): the nev smallest pairs of the pencil H y = theta G y, 1 <= nev <= n <= kMax = 12,
// G = S^T S and H = S^T A S of a basis S of n columns (row-major n x n; only what the caller filled is read: both
// triangles, averaged):
//   1. symmetrise: G <- (G + G^T) / 2, H likewise;
//   2. scale: d_i = 1 / sqrt(G_ii);  G <- D G D (its diagonal set to exactly 1), H <- D H D;
//   3. factor G = L L^T by Cholesky, row by row.  A pivot (the remaining diagonal before its square root) is DEFICIENT if
//      it is not positive and finite or below 64 eps of the unit diagonal: the basis is numerically dependent;
//   4. M = L^-1 H L^-T by two triangular solves, symmetrised;
//   5. cyclic Jacobi on M (rows p < q in order, Rutishauser's rotation, until the off-diagonal norm is below
//      1e-2 eps ||M||_F, at most kSweeps sweeps): M = Y diag(mu) Y^T;
//   6. the nev smallest mu ascending (ties by index) are theta; C = D L^-T Y of those columns (row-major n x nev), so
//      that X = S C has X^T X = I and X^T A X = diag(theta) up to rounding.
// Nothing is allocated; every array is kMax x kMax on the stack.
#pragma once

#include <cmath>

namespace mgx_eig_dense {

constexpr int kMax = 12;
constexpr int kSweeps = 60;
constexpr double kEps = 2.220446049250313e-16;
constexpr double kPivotMin = 64.0 * kEps;

struct Result {
    bool ok;            // false: deficient (index and pivot say where), theta and C are not written
    int index;
    double pivot;
};

inline bool positive_finite(double x) { return x > 0.0 && std::isfinite(x); }

// M = V diag(w) V^T for symmetric M (n x n, ld kMax), destroyed; V's columns are the eigenvectors
inline void cyclic_jacobi(int n, double (*M)[kMax], double (*V)[kMax], double* w)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        double off = 0.0, all = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = 0; q < n; ++q) (p == q ? all : off) += M[p][q] * M[p][q];
        all += off;
        if (!(off > 1e-4 * kEps * kEps * all)) break;        // (also ends on NaN: the caller checks theta)
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = M[p][q];
                if (apq == 0.0) continue;
                const double th = (M[q][q] - M[p][p]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {                    // columns p and q
                    const double kp = M[k][p], kq = M[k][q];
                    M[k][p] = c * kp - s * kq;
                    M[k][q] = s * kp + c * kq;
                }
                for (int k = 0; k < n; ++k) {                    // rows p and q
                    const double pk = M[p][k], qk = M[q][k];
                    M[p][k] = c * pk - s * qk;
                    M[q][k] = s * pk + c * qk;
                }
                M[p][q] = M[q][p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double kp = V[k][p], kq = V[k][q];
                    V[k][p] = c * kp - s * kq;
                    V[k][q] = s * kp + c * kq;
                }
            }
    }
    for (int i = 0; i < n; ++i) w[i] = M[i][i];
}

inline Result rayleigh_ritz(int n, int nev, const double* Gin, const double* Hin, double* theta, double* C)
{
    double G[kMax][kMax], H[kMax][kMax], L[kMax][kMax], d[kMax];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            G[i][j] = 0.5 * (Gin[i * n + j] + Gin[j * n + i]);
            H[i][j] = 0.5 * (Hin[i * n + j] + Hin[j * n + i]);
        }
    for (int i = 0; i < n; ++i) {
        if (!positive_finite(G[i][i])) return Result{false, i, G[i][i]};
        d[i] = 1.0 / std::sqrt(G[i][i]);
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            G[i][j] = i == j ? 1.0 : d[i] * G[i][j] * d[j];
            H[i][j] = d[i] * H[i][j] * d[j];
        }
    // G = L L^T
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = G[i][j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!positive_finite(s) || s < kPivotMin) return Result{false, i, s};
                L[i][i] = std::sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    // Y = L^-1 H (column by column), M = Y L^-T = (L^-1 Y^T)^T
    double Y[kMax][kMax], M[kMax][kMax];
    for (int c = 0; c < n; ++c)
        for (int i = 0; i < n; ++i) {
            double s = H[i][c];
            for (int k = 0; k < i; ++k) s -= L[i][k] * Y[k][c];
            Y[i][c] = s / L[i][i];
        }
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < n; ++i) {
            double s = Y[r][i];
            for (int k = 0; k < i; ++k) s -= L[i][k] * M[r][k];
            M[r][i] = s / L[i][i];
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) M[i][j] = M[j][i] = 0.5 * (M[i][j] + M[j][i]);
    double V[kMax][kMax], w[kMax];
    cyclic_jacobi(n, M, V, w);
    // the nev smallest, ascending (selection: ties and NaN keep their index order)
    int order[kMax];
    bool used[kMax] = {};
    for (int j = 0; j < nev; ++j) {
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (!used[i] && (best < 0 || w[i] < w[best])) best = i;
        used[best] = true;
        order[j] = best;
    }
    for (int j = 0; j < nev; ++j) {
        theta[j] = w[order[j]];
        // z = L^-T y by back substitution, then the scaling
        double z[kMax];
        for (int i = n - 1; i >= 0; --i) {
            double s = V[i][order[j]];
            for (int k = i + 1; k < n; ++k) s -= L[k][i] * z[k];
            z[i] = s / L[i][i];
        }
        for (int i = 0; i < n; ++i) C[i * nev + j] = d[i] * z[i];
    }
    return Result{true, -1, 0.0};
}

} // namespace mgx_eig_dense
