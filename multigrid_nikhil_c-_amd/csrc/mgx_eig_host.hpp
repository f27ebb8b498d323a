// mgx_eig_host.hpp - the host side of mgx_eigs and mgx_time_eig_pass (absent in the reference): LOBPCG with soft locking
// around mgx_solve_multi's block cycle.  The iteration is stated in mgx_eig.hpp, whose kernels this file launches; the
// small dense problem is mgx_eig_dense.hpp's.  Included by mgx.hip after mgx_multi_host.hpp.
#pragma once

#include "mgx_eig_dense.hpp"

namespace {

constexpr int kEigPairs = 6;                                          // the upper block triangle of {X, W, P}
constexpr int kEigPairSums = 2 * MGX_MAX_RHS * MGX_MAX_RHS;           // sums of one pair: KL x [B, A B]

void eig_free(mgx_solver::EigWs& w)
{
    for (int c = 0; c < MGX_MAX_RHS; ++c)
        for (void** p : {&w.X[c], &w.AX[c], &w.AW[c], &w.P[c], &w.AP[c]}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
    if (w.gpart) (void)hipFree(w.gpart);
    if (w.gsum) (void)hipFree(w.gsum);
    if (w.gsum_host) (void)hipHostFree(w.gsum_host);
    w.gpart = w.gsum = w.gsum_host = nullptr;
    w.cols = 0;
}

template <typename T> EigGeom eig_geom(const mgx_solver* s)
{
    const Level& l = s->lv[s->cfg.finest_level];
    return EigGeom{l.N, l.pitch, l.rows, make_launch(l.N, VecOf<T>::W, l.N - 1, s->rows_per_chunk), make_launch(l.N, VecOf<T>::W, l.N - 1, 1)};
}

// X, AX, AW, P, AP of columns [0, nev) and the Gram buffers exist afterwards (multi_ensure has made the workspace
// columns).  A failure frees the column it was allocating and leaves what existed
int eig_ensure(mgx_solver* s, int nev, int blocks)
{
    auto& w = s->eig;
    const Level& l = s->lv[s->cfg.finest_level];
    auto bad = [&](const char* what) {
        (void)hipGetLastError();
        return s->fail(MGX_ERR_ALLOC, std::string("mgx_eigs: allocation failed for ") + what);
    };
    if (!w.gpart && hipMalloc((void**)&w.gpart, (size_t)kEigPairSums * blocks * sizeof(double)) != hipSuccess) { w.gpart = nullptr; return bad("the Gram partial sums"); }
    if (!w.gsum && hipMalloc((void**)&w.gsum, kEigPairs * kEigPairSums * sizeof(double)) != hipSuccess) { w.gsum = nullptr; return bad("the Gram sums"); }
    if (!w.gsum_host && hipHostMalloc((void**)&w.gsum_host, kEigPairs * kEigPairSums * sizeof(double)) != hipSuccess) {
        w.gsum_host = nullptr;
        return bad("the pinned Gram sums");
    }
    for (int c = w.cols; c < nev; ++c) {
        bool ok = true;
        for (void** p : {&w.X[c], &w.AX[c], &w.AW[c], &w.P[c], &w.AP[c]})
            if (!(ok = alloc_zeroed(s, p, l.bytes))) break;
        if (!ok) {
            (void)hipStreamSynchronize(s->stream);
            for (void** p : {&w.X[c], &w.AX[c], &w.AW[c], &w.P[c], &w.AP[c]}) {
                if (*p) (void)hipFree(*p);
                *p = nullptr;
            }
            return bad(("the vectors of column " + std::to_string(c)).c_str());
        }
        w.cols = c + 1;
    }
    return MGX_OK;
}

// one block of the basis: k vectors V with A V
struct EigBlock { int k; void* v[MGX_MAX_RHS]; void* av[MGX_MAX_RHS]; };

template <typename T>
struct EigRun {
    mgx_solver* s;
    int nev;
    EigGeom e;
    double theta[MGX_MAX_RHS] = {};

    Level& fine() const { return s->lv[s->cfg.finest_level]; }

    void apply(int k, void* const* v, void* const* out) const
    {
        const T* vi[MGX_MAX_RHS];
        T* vo[MGX_MAX_RHS];
        for (int j = 0; j < k; ++j) { vi[j] = (const T*)v[j]; vo[j] = (T*)out[j]; }
        launch_eig_apply<T>(k, fine().nine, vi, vo, op9_of<T>(fine()), e, s->stream);
    }

    // pair number `slot`: left block a against [b, A b]; a == b: the diagonal pair
    void gram(int slot, const EigBlock& a, const EigBlock& b, bool diag) const
    {
        const T *l[MGX_MAX_RHS], *r[2 * MGX_MAX_RHS];
        for (int i = 0; i < a.k; ++i) l[i] = (const T*)a.v[i];
        for (int j = 0; j < b.k; ++j) { r[j] = (const T*)b.v[j]; r[b.k + j] = (const T*)b.av[j]; }
        launch_eig_gram<T>(a.k, b.k, diag, l, r, s->eig.gpart, s->eig.gsum + slot * kEigPairSums, e, s->stream);
    }

    void combine(int ki, void* const* in, int ko, void* const* out, const double* c) const
    {
        const T* vi[mgx::kEigMaxIn];
        T* vo[MGX_MAX_RHS];
        for (int i = 0; i < ki; ++i) vi[i] = (const T*)in[i];
        for (int j = 0; j < ko; ++j) vo[j] = (T*)out[j];
        launch_eig_combine<T>(ki, ko, vi, vo, c, e, s->stream);
    }

    // R_j = AX_j - theta_j X_j into the finest b of every column, ||R_j|| into r: one copy, one host synchronisation
    int residuals(double* r) const
    {
        auto& ws = s->multi;
        auto& w = ws.lv[s->cfg.finest_level];
        const T *ax[MGX_MAX_RHS], *x[MGX_MAX_RHS];
        T* rr[MGX_MAX_RHS];
        double *part[MGX_MAX_RHS], *sums[MGX_MAX_RHS];
        for (int j = 0; j < nev; ++j) {
            ax[j] = (const T*)s->eig.AX[j]; x[j] = (const T*)s->eig.X[j]; rr[j] = (T*)w.b[j];
            part[j] = ws.part[j]; sums[j] = ws.sums + j;
        }
        launch_eig_residual<T>(nev, ax, x, rr, part, sums, theta, e, s->stream);
        HIPCHK(s, hipGetLastError());
        HIPCHK(s, hipMemcpyAsync(ws.sums_host, ws.sums, MGX_MAX_RHS * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));
        for (int j = 0; j < nev; ++j) r[j] = std::sqrt(ws.sums_host[j]);
        return MGX_OK;
    }

    // the Gram sums of the upper block triangle of blk[0 .. nb) to the host: one copy, one host synchronisation.
    // G and H (n x n, n = the blocks' columns): the upper block triangle filled, the lower its transpose
    int gram_all(const EigBlock* blk, int nb, double* G, double* H, int n) const
    {
        int slot = 0;
        for (int a = 0; a < nb; ++a)
            for (int b = a; b < nb; ++b) gram(slot++, blk[a], blk[b], a == b);
        HIPCHK(s, hipGetLastError());
        HIPCHK(s, hipMemcpyAsync(s->eig.gsum_host, s->eig.gsum, kEigPairs * kEigPairSums * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));
        int off[4] = {0, 0, 0, 0};
        for (int a = 0; a < nb; ++a) off[a + 1] = off[a] + blk[a].k;
        slot = 0;
        for (int a = 0; a < nb; ++a)
            for (int b = a; b < nb; ++b) {
                const double* sums = s->eig.gsum_host + (slot++) * kEigPairSums;
                const int ka = blk[a].k, kb = blk[b].k;
                for (int i = 0; i < ka; ++i)
                    for (int j = 0; j < kb; ++j) {
                        const double g = sums[i * 2 * kb + j], h = sums[i * 2 * kb + kb + j];
                        G[(off[a] + i) * n + off[b] + j] = g;
                        H[(off[a] + i) * n + off[b] + j] = h;
                        if (a != b) { G[(off[b] + j) * n + off[a] + i] = g; H[(off[b] + j) * n + off[a] + i] = h; }
                    }
            }
        return MGX_OK;
    }
};

inline bool eig_theta_ok(const double* theta, int nev, int* which)
{
    for (int j = 0; j < nev; ++j)
        if (!mgx_eig_dense::positive_finite(theta[j])) { *which = j; return false; }
    return true;
}

// what one block of LOBPCG leaves on the host (its Ritz vectors are the workspace's X[0 .. nev), on the device)
struct EigBlockResult {
    std::vector<double> hist[MGX_MAX_RHS];
    double fu[MGX_MAX_RHS] = {};
    int cycles[MGX_MAX_RHS] = {};
    double theta[MGX_MAX_RHS] = {};
    bool failed = false;
    std::string reason;
    bool converged(int j, double tol) const { return !failed && hist[j].back() <= tol * theta[j]; }
};

// THE ITERATION of mgx_eig.hpp on the nev <= MGX_MAX_RHS host guesses x, in the workspace columns [0, nev) (which exist).
// `who` opens every message.  project(k, columns) constrains k device columns to the space the caller iterates in: the
// guesses twice before the first Rayleigh-Ritz step, W_act once per iteration after the cycle (mgx_eigs: nothing;
// mgx_eigs_many: against the locked vectors, mgx_eig_many.hpp).  The stream is idle on return
template <typename T, typename Project>
int eig_block(EigRun<T>& run, const void* x, double tol, int max_iters, const std::string& who, Project&& project, EigBlockResult& out)
{
    namespace de = mgx_eig_dense;
    mgx_solver* s = run.s;
    const int nev = run.nev;
    const int L = s->cfg.finest_level;
    Level& l = s->lv[L];
    auto& ew = s->eig;
    auto& w = s->multi.lv[L];
    const size_t nn = (size_t)(l.N - 1) * (size_t)(l.N - 1);
    for (int j = 0; j < nev; ++j)
        if (int rc = copy_in(s, l, ew.X[j], (const T*)x + (size_t)j * nn, nn)) return rc;
    project(nev, ew.X);
    project(nev, ew.X);

    auto& hist = out.hist;
    auto& fu = out.fu;
    auto& cycles = out.cycles;
    double G[de::kMax * de::kMax], H[de::kMax * de::kMax], C[de::kMax * MGX_MAX_RHS], theta[MGX_MAX_RHS];
    std::string& reason = out.reason;
    bool& failed = out.failed;

    // the initial Rayleigh-Ritz step on the guesses
    EigBlock bx{nev, {}, {}};
    for (int j = 0; j < nev; ++j) { bx.v[j] = ew.X[j]; bx.av[j] = ew.AX[j]; }
    run.apply(nev, ew.X, ew.AX);
    if (int rc = run.gram_all(&bx, 1, G, H, nev)) return rc;
    de::Result rr = de::rayleigh_ritz(nev, nev, G, H, theta, C);
    if (!rr.ok)
        return s->fail(MGX_ERR_INVALID, who + ": the guesses are linearly dependent (or not finite): Cholesky pivot " + std::to_string(rr.pivot) +
                                            " at column " + std::to_string(rr.index));
    for (int j = 0; j < nev; ++j) run.theta[j] = theta[j];
    run.combine(nev, ew.X, nev, ew.X, C);
    run.apply(nev, ew.X, ew.AX);
    int which = 0;
    if (!eig_theta_ok(theta, nev, &which)) {
        failed = true;
        reason = who + ": Ritz value " + std::to_string(which) + " of the guesses is " + std::to_string(theta[which]) +
                 ", not a positive finite number: the operator is not symmetric positive definite";
    }

    bool have_p = false;
    const bool trace = env_int("MGX_EIG_TRACE", 0) != 0;
    for (int k = 0;; ++k) {
        double r[MGX_MAX_RHS] = {};
        if (int rc = run.residuals(r)) return rc;                          // host synchronisation 1
        for (int j = 0; j < nev; ++j) hist[j].push_back(r[j]);
        if (failed) break;
        MultiSet act{};
        for (int j = 0; j < nev; ++j)
            if (!(r[j] <= tol * run.theta[j])) act.act[act.m++] = j;
        if (act.m == 0 || k == max_iters) break;
        // W_act = M R_act: the cycle from zero, R already the finest right-hand side of the columns
        if (int rc = zero_u(s, L, act)) return rc;
        vcycle(s, L, false, 0, s->cycle, act, fu);
        EigBlock bw{act.m, {}, {}}, bp{nev, {}, {}};
        for (int i = 0; i < act.m; ++i) {
            const int c = act.act[i];
            ++cycles[c];
            bw.v[i] = w.u[c];
            bw.av[i] = ew.AW[c];
        }
        project(act.m, bw.v);
        for (int j = 0; j < nev; ++j) { bp.v[j] = ew.P[j]; bp.av[j] = ew.AP[j]; }
        run.apply(act.m, bw.v, bw.av);
        const EigBlock blk[3] = {bx, bw, bp};
        const int np = have_p ? nev : 0;
        const int n = nev + act.m + np;
        if (int rc = run.gram_all(blk, have_p ? 3 : 2, G, H, n)) return rc;   // host synchronisation 2
        rr = de::rayleigh_ritz(n, nev, G, H, theta, C);
        const de::Result first_try = rr;
        int used = n;
        if (!rr.ok && have_p) {
            // restart: the same step without P, from the sums already here (the leading block of G and H)
            used = nev + act.m;
            double G2[de::kMax * de::kMax], H2[de::kMax * de::kMax];
            for (int i = 0; i < used; ++i)
                for (int j = 0; j < used; ++j) { G2[i * used + j] = G[i * n + j]; H2[i * used + j] = H[i * n + j]; }
            rr = de::rayleigh_ritz(used, nev, G2, H2, theta, C);
        }
        // MGX_EIG_TRACE=1: one line per iteration on stderr (the basis, whether the step was a restart and why)
        if (trace)
            std::fprintf(stderr, "[mgx_eigs] iteration %d: |act| %d, basis %d columns%s%s (pivot %.3g at column %d)\n", k + 1, act.m, used,
                         have_p ? (used == n ? ", with P" : ", RESTART without P") : ", no P yet", rr.ok ? "" : ", DEFICIENT", first_try.pivot,
                         first_try.index);
        if (!rr.ok) {
            failed = true;
            reason = who + ": iteration " + std::to_string(k + 1) + ": the basis [X, W" + std::string(have_p ? ", P" : "") +
                     "] is rank deficient with and without P (Cholesky pivot " + std::to_string(rr.pivot) + " at column " + std::to_string(rr.index) + ")";
            break;
        }
        if (!eig_theta_ok(theta, nev, &which)) {
            failed = true;
            reason = who + ": iteration " + std::to_string(k + 1) + ": Ritz value " + std::to_string(which) + " is " + std::to_string(theta[which]) +
                     ", not a positive finite number: the operator is not symmetric positive definite";
            break;
        }
        const bool with_p = used == n && have_p;
        // X <- S C (reads the old P), then P <- [W, P] C_wp; AP and AX are applied afresh.  (AP <- [AW, AP] C_wp, the
        // recurrence, costs the same traffic and is not stable: the P_j of a locked column shrinks to rounding level while
        // the recurrence keeps the absolute error of AP_j, and the Gram entries of that column go wrong - the locked
        // columns' residuals then rise by a factor of ten per iteration; tests/eig_ref.py shows it in numpy)
        void* in[mgx::kEigMaxIn];
        int ki = 0;
        for (int j = 0; j < nev; ++j) in[ki++] = bx.v[j];
        for (int i = 0; i < act.m; ++i) in[ki++] = bw.v[i];
        if (with_p)
            for (int j = 0; j < nev; ++j) in[ki++] = bp.v[j];
        run.combine(ki, in, nev, ew.X, C);
        run.combine(ki - nev, in + nev, nev, ew.P, C + nev * nev);
        run.apply(nev, ew.P, ew.AP);
        have_p = true;
        for (int j = 0; j < nev; ++j) run.theta[j] = theta[j];
        run.apply(nev, ew.X, ew.AX);
    }
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    for (int j = 0; j < nev; ++j) out.theta[j] = run.theta[j];
    return MGX_OK;
}

template <typename T>
int eigs_t(mgx_solver* s, int nev, void* x, double* lambda, double tol, int max_iters, mgx_stats* stats, double* history, int history_cap)
{
    const auto t0 = std::chrono::steady_clock::now();
    EigRun<T> run{s, nev, eig_geom<T>(s)};
    if (int rc = multi_ensure(s, nev)) return rc;
    if (int rc = eig_ensure(s, nev, run.e.g.blocks)) return rc;
    EigBlockResult res;
    if (int rc = eig_block<T>(run, x, tol, max_iters, "mgx_eigs", [](int, void* const*) {}, res)) return rc;
    Level& l = s->lv[s->cfg.finest_level];
    const size_t nn = (size_t)(l.N - 1) * (size_t)(l.N - 1);
    for (int j = 0; j < nev; ++j) {
        if (int rc = copy_out(s, l, s->eig.X[j], (T*)x + (size_t)j * nn, nn)) return rc;
        lambda[j] = res.theta[j];
    }
    for (int j = 0; j < nev; ++j)
        finish_solve(stats ? stats + j : nullptr, history ? history + (size_t)j * (size_t)history_cap : nullptr, history_cap, res.hist[j],
                     res.cycles[j], res.converged(j, tol), t0, res.fu[j]);
    if (stats) {
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int j = 0; j < nev; ++j) stats[j].seconds = seconds;
    }
    if (!res.reason.empty()) s->err = res.reason;
    return MGX_OK;
}

// mgx_time_eig_pass: `repeats` launches of one pass on the first nev columns of the workspace, between two events.
//   MGX_EIG_PASS_GRAM      k_eig_gram<T, nev, nev, false>: X against [P, AP], with the reduction of its sums
//   MGX_EIG_PASS_COMBINE   k_eig_combine<T, 3 nev, nev>: X <- [X, W, P] with the identity on X (X keeps its values)
//   MGX_EIG_PASS_RESIDUAL  k_eig_residual<T, nev> with theta = 1 into the finest b of the columns, with its reductions
//   MGX_EIG_PASS_APPLY     k_apply_var_multi<T, NQ, nev>: AX <- A X
template <typename T>
int eig_time_pass(mgx_solver* s, int pass, int nev, int repeats, double* ms)
{
    EigRun<T> run{s, nev, eig_geom<T>(s)};
    auto& ew = s->eig;
    auto& w = s->multi.lv[s->cfg.finest_level];
    for (int j = 0; j < nev; ++j) run.theta[j] = 1.0;
    EigBlock bx{nev, {}, {}}, bp{nev, {}, {}};
    void* in[mgx::kEigMaxIn];
    double c[mgx::kEigMaxIn * MGX_MAX_RHS] = {};
    for (int j = 0; j < nev; ++j) {
        bx.v[j] = ew.X[j]; bx.av[j] = ew.AX[j]; bp.v[j] = ew.P[j]; bp.av[j] = ew.AP[j];
        in[j] = ew.X[j]; in[nev + j] = w.u[j]; in[2 * nev + j] = ew.P[j];
        c[j * nev + j] = 1.0;
    }
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) {
            if (pass == MGX_EIG_PASS_GRAM) run.gram(0, bx, bp, false);
            else if (pass == MGX_EIG_PASS_COMBINE) run.combine(3 * nev, in, nev, ew.X, c);
            else if (pass == MGX_EIG_PASS_APPLY) run.apply(nev, ew.X, ew.AX);
            else {
                const T *ax[MGX_MAX_RHS], *x[MGX_MAX_RHS];
                T* rr[MGX_MAX_RHS];
                double *part[MGX_MAX_RHS], *sums[MGX_MAX_RHS];
                for (int j = 0; j < nev; ++j) {
                    ax[j] = (const T*)ew.AX[j]; x[j] = (const T*)ew.X[j]; rr[j] = (T*)w.b[j];
                    part[j] = s->multi.part[j]; sums[j] = s->multi.sums + j;
                }
                launch_eig_residual<T>(nev, ax, x, rr, part, sums, run.theta, run.e, s->stream);
            }
        }
    });
    if (!rc) *ms /= repeats;
    return rc;
}

} // namespace
