// mgx_newton_host.hpp - the host side of mgx_newton and mgx_time_newton_pass (absent in the reference; the pass and its
// arithmetic are mgx_newton.hpp's).  Included by mgx.hip after mgx_theta_host.hpp, whose zero-order term
// (reaction_base, reaction_shift) carries the Jacobian's diagonal.
#pragma once

namespace {

void newton_free(mgx_solver::NewtonWs& w)
{
    for (void** p : {&w.un, &w.ut, &w.f, &w.kap, &w.dn}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

// which handles run Newton steps: those that carry a zero-order term (reaction_guard), with the hierarchy built - the
// transfer it was built with is the one every step rebuilds it with
int newton_guard(mgx_solver* s, const char* fn)
{
    if (int rc = reaction_guard(s, fn)) return rc;
    if (!s->gal_built) return s->fail(MGX_ERR_STATE, std::string(fn) + ": Galerkin hierarchy not built (mgx_build_galerkin[_transfer]): the steps rebuild it with the transfer of that build");
    return MGX_OK;
}

// one launch of k_newton_pass on the finest level and the reduction of its sums: b, dn (and ut when step) from un (and the
// linear solve's result in U), *r = ||b||_2.  One D2H of one double and one host synchronisation
int newton_pass(mgx_solver* s, bool step, double lam, void* b, double* r)
{
    const Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->nwt;
    const void* centre = s->rx.set ? s->rx.c0 : l.A[0];       // A0's: slot 0 carries the term once one is set
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        launch_newton_pass<T>(var_level<T>(l), step, (const T*)w.un, (const T*)l.u, (const T*)w.f, (const T*)w.kap, (const T*)centre, (T*)w.ut,
                              (T*)b, (T*)w.dn, newton_poly<T>(w.p1, w.p2, w.p3, (T)lam), s->partial, s->sum_dev, s->stream);
    });
    s->norm_blocks_ready = 0;                                 // partial[] holds this pass's sums
    HIPCHK(s, hipGetLastError());
    if (!r) return MGX_OK;
    HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    *r = std::sqrt(*s->sum_host);
    return MGX_OK;
}

int newton(mgx_solver* s, const mgx_newton_opts& o, const void* kappa, size_t count, mgx_newton_stats* nstats, mgx_stats* lin_stats,
           double* step_lengths, double* history, int history_cap)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int L = s->cfg.finest_level;
    Level& l = s->lv[L];
    auto& w = s->nwt;
    // the whole workspace before anything is touched: a failure leaves the operator and the hierarchy as they were
    const struct { void** p; const char* what; } grids[] = {{&w.un, "the iterate"}, {&w.ut, "the trial iterate"}, {&w.f, "the right-hand side"},
                                                            {&w.kap, "kappa"}, {&w.dn, "the Jacobian's diagonal term"},
                                                            {&s->rx.c0, "the base centre"}, {&s->rx.d, "the zero-order term"}};
    for (const auto& g : grids)
        if (int rc = reaction_grid(s, g.p, "mgx_newton", g.what)) return rc;
    w.p1 = o.p1; w.p2 = o.p2; w.p3 = o.p3;
    if (int rc = copy_in(s, l, w.kap, kappa, count)) return rc;
    HIPCHK(s, hipMemcpyAsync(w.un, l.u, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipMemcpyAsync(w.f, l.b, l.bytes, hipMemcpyDeviceToDevice, s->stream));

    std::vector<double> hist(1, 0.0);
    int backtracks = 0, lin_iters = 0, rc = MGX_OK;
    std::string msg;                                          // what mgx_last_error says after the call
    if ((rc = newton_pass(s, false, 0.0, l.b, &hist[0])) != MGX_OK) msg = s->err;
    for (int k = 0; rc == MGX_OK && k < o.max_newton && !(hist[k] <= o.tol * hist[0]); ++k) {
        // the Jacobian A0 + diag(d) of the iterate: what mgx_set_reaction(d) + mgx_build_galerkin_transfer leave
        if ((rc = reaction_base(s)) != MGX_OK) { msg = s->err; break; }
        std::swap(s->rx.d, w.dn);
        if ((rc = reaction_shift(s)) == MGX_OK) rc = s->work_f64 ? galerkin_build_t<double>(s, s->transfer) : galerkin_build_t<float>(s, s->transfer);
        if (rc == MGX_OK) rc = zero_u(s, L);                 // (B holds b: the pass wrote it there)
        if (rc == MGX_OK) {
            s->norm_blocks_ready = 0;
            s->err.clear();
            mgx_stats st{};
            if (o.solver == MGX_STEP_SOLVE) rc = mgx_solve(s, o.lin_tol, o.lin_max_iters, &st, nullptr, 0);
            else if (o.solver == MGX_STEP_GCR) rc = mgx_solve_gcr(s, o.lin_tol, o.lin_max_iters, o.restart, &st, nullptr, 0);
            else rc = mgx_solve_refine_gcr(s, o.lin_tol, o.lin_max_iters, o.restart, &st, nullptr, 0);
            if (rc == MGX_OK) {
                if (lin_stats) lin_stats[k] = st;
                lin_iters += st.cycles;
            }
        }
        if (rc != MGX_OK) { msg = "mgx_newton: step " + std::to_string(k) + ": " + s->err; break; }
        // backtracking on ||F||: the trial un + lam de with lam = 1, 1/2, ... (the solvers swap u and tmp: l.u afresh)
        double lam = 1.0, r = 0.0;
        bool accepted = false;
        for (int j = 0;;) {
            if ((rc = newton_pass(s, true, lam, l.b, &r)) != MGX_OK) { msg = "mgx_newton: step " + std::to_string(k) + ": " + s->err; break; }
            if (r <= (1.0 - 1e-4 * lam) * hist[k]) { accepted = true; break; }       // (NaN rejects)
            ++backtracks;
            if (++j > o.max_backtracks) break;
            lam *= 0.5;
        }
        if (rc != MGX_OK) break;
        if (!accepted) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "mgx_newton: step %d: line search failed: smallest lam tried %.17g gave ||F|| = %.17g against %.17g of the iterate",
                          k, lam, r, hist[k]);
            msg = buf;
            break;
        }
        std::swap(w.un, w.ut);
        hist.push_back(r);
        if (step_lengths) step_lengths[k] = lam;
    }
    // U = the last accepted iterate, B = the caller's f, on every path
    const hipError_t e1 = hipMemcpyAsync(l.u, w.un, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    const hipError_t e2 = hipMemcpyAsync(l.b, w.f, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    const hipError_t e3 = hipStreamSynchronize(s->stream);
    s->norm_blocks_ready = 0;
    s->err = msg;
    if (rc != MGX_OK) return rc;
    for (hipError_t e : {e1, e2, e3})
        if (e != hipSuccess) return s->fail(MGX_ERR_HIP, std::string("mgx_newton: restoring U and B: ") + hipGetErrorString(e));
    if (nstats) {
        nstats->iterations = (int)hist.size() - 1;
        nstats->converged = hist.back() <= o.tol * hist[0] ? 1 : 0;
        nstats->initial_residual = hist.front();
        nstats->final_residual = hist.back();
        nstats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        nstats->linear_iterations = lin_iters;
        nstats->backtracks = backtracks;
        nstats->history_len = (int)hist.size();
    }
    if (history)
        for (int i = 0; i < (int)hist.size() && i < history_cap; ++i) history[i] = hist[i];
    return MGX_OK;
}

} // namespace
