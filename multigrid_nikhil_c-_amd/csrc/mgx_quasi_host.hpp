// mgx_quasi_host.hpp - the host side of mgx_quasi and mgx_time_quasi_pass (absent in the reference; the pass and its
// arithmetic are mgx_quasi.hpp's).  Included by mgx.hip after mgx_newton_host.hpp, whose run record and
// report it shares (NewtonRun, newton_report).  The loop is mgx_newton's (newton_iterate) with another pass and another way
// to put the operator in place - a sibling, not an instance: newton_iterate shifts the centre of a fixed A0 and rebuilds
// with the handle's transfer, this one replaces all five grids of the finest level and rebuilds with opt.transfer.
//
// The pass writes its five coefficient grids into a second set (QuasiWs::A2); an iteration makes them the level's by
// swapping the ten pointers.  So a rejected trial never touches the operator of the last linear solve, no iteration
// leaves the handle's operator alone, and mgx_time_quasi_pass has somewhere to write.
#pragma once

namespace {

void quasi_free(mgx_solver::QuasiWs& w)
{
    std::vector<void**> all = {&w.un, &w.ut, &w.f, (void**)&w.an};
    for (void*& p : w.A2) all.push_back(&p);
    for (void** p : all) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

// which handles run the iteration (the message names the reason).  No operator and no hierarchy are needed beforehand
int quasi_guard(mgx_solver* s, const char* fn)
{
    NO_DIST(s)
    if (!s->var) return s->fail(MGX_ERR_STATE, std::string(fn) + ": handle was created with op = MGX_OPERATOR_POISSON (the constant stencil has no coefficients)");
    if (!s->galerkin)
        return s->fail(MGX_ERR_STATE, std::string(fn) + ": op = MGX_OPERATOR_STENCIL5: the caller owns every level's stencil, but the coarse operators "
                                                        "of a nonlinear step are R A P of the finest; this entry point is for MGX_OPERATOR_GALERKIN");
    return MGX_OK;
}

// the checks on the options, in the documented order
int quasi_opts_check(mgx_solver* s, const mgx_quasi_opts* o, const char* fn)
{
    const std::string pre = std::string(fn) + ": ";
    if (!std::isfinite(o->k0) || !std::isfinite(o->k1) || !std::isfinite(o->k2)) return s->fail(MGX_ERR_INVALID, pre + "k0, k1, k2 must be finite");
    if (o->method != MGX_QUASI_PICARD && o->method != MGX_QUASI_NEWTON) return s->fail(MGX_ERR_INVALID, pre + "method must be MGX_QUASI_PICARD or MGX_QUASI_NEWTON");
    if (o->transfer != MGX_TRANSFER_BILINEAR && o->transfer != MGX_TRANSFER_OPERATOR)
        return s->fail(MGX_ERR_INVALID, pre + "transfer must be MGX_TRANSFER_BILINEAR or MGX_TRANSFER_OPERATOR");
    if (o->solver < MGX_STEP_SOLVE || o->solver > MGX_STEP_REFINE_GCR)
        return s->fail(MGX_ERR_INVALID, pre + "solver must be MGX_STEP_SOLVE, MGX_STEP_GCR or MGX_STEP_REFINE_GCR");
    if (!(o->lin_tol >= 0.0)) return s->fail(MGX_ERR_INVALID, pre + "lin_tol >= 0 required");
    if (o->lin_max_iters < 0) return s->fail(MGX_ERR_INVALID, pre + "lin_max_iters >= 0 required");
    if (o->solver != MGX_STEP_SOLVE && (o->restart < 1 || o->restart > MGX_GCR_MAX_RESTART))
        return s->fail(MGX_ERR_INVALID, pre + "1 <= restart <= MGX_GCR_MAX_RESTART required");
    if (!(o->tol >= 0.0)) return s->fail(MGX_ERR_INVALID, pre + "tol >= 0 required");
    if (o->max_iters < 0) return s->fail(MGX_ERR_INVALID, pre + "max_iters >= 0 required");
    if (o->max_backtracks < 0 || o->max_backtracks > 30) return s->fail(MGX_ERR_INVALID, pre + "0 <= max_backtracks <= 30 required");
    return MGX_OK;
}

// every grid of mgx_quasi before anything is touched: a failure leaves the handle as it was (grids already allocated stay
// for the next attempt)
int quasi_workspace(mgx_solver* s, const char* fn)
{
    auto& w = s->qsi;
    const Level& l = s->lv[s->cfg.finest_level];
    if (int rc = reaction_grid(s, &w.un, fn, "the iterate")) return rc;
    if (int rc = reaction_grid(s, &w.ut, fn, "the trial iterate")) return rc;
    if (int rc = reaction_grid(s, &w.f, fn, "the right-hand side")) return rc;
    for (void*& p : w.A2)
        if (int rc = reaction_grid(s, &p, fn, "the next operator")) return rc;
    if (!w.an && !alloc_zeroed(s, (void**)&w.an, (size_t)l.rows * (size_t)l.pitch * sizeof(double)))
        return s->fail(MGX_ERR_ALLOC, std::string(fn) + ": allocation failed for the nodal coefficient");
    return MGX_OK;
}

// one launch of k_quasi_pass on the finest level and the reduction of its sums: the five grids of A2, b (and ut when step)
// from un (and the linear solve's result in U), *r = ||b||_2.  One D2H of one double and one host synchronisation
int quasi_pass(mgx_solver* s, bool step, bool newton, double lam, void* b, double* r)
{
    const Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->qsi;
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        Quasi5Out<T> out;
        for (int q = 0; q < 5; ++q) out.a[q] = (T*)w.A2[q];
        launch_quasi_pass<T>(l.N, l.rows, l.pitch, step, newton, (const T*)w.un, (const T*)l.u, (const T*)w.f, w.an, out, (T*)w.ut, (T*)b,
                             quasi_poly<T>(w.k0, w.k1, w.k2, (T)lam), s->partial, s->sum_dev, s->stream);
    });
    s->norm_blocks_ready = 0;                                 // partial[] holds this pass's sums
    HIPCHK(s, hipGetLastError());
    if (!r) return MGX_OK;
    HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    *r = std::sqrt(*s->sum_host);
    return MGX_OK;
}

// the iteration on the loaded grids: un the guess, f the right-hand side, an and k0 .. k2.  It leaves the last accepted
// iterate in un; B holds the right-hand side of the last pass
int quasi_iterate(mgx_solver* s, const mgx_quasi_opts& o, mgx_stats* lin_stats, double* step_lengths, NewtonRun& run)
{
    const std::string pre = "mgx_quasi: step ";
    const int L = s->cfg.finest_level;
    Level& l = s->lv[L];
    auto& w = s->qsi;
    const bool newton = o.method == MGX_QUASI_NEWTON;
    std::vector<double>& hist = run.hist;
    std::string& msg = run.msg;
    hist.assign(1, 0.0);
    int rc = MGX_OK;
    if ((rc = quasi_pass(s, false, newton, 0.0, l.b, &hist[0])) != MGX_OK) msg = s->err;
    for (int k = 0; rc == MGX_OK && k < o.max_iters && !(hist[k] <= o.tol * hist[0]); ++k) {
        // A(u_k) or J(u_k) becomes the finest operator: what mgx_set_stencil + mgx_build_galerkin_transfer leave
        for (int q = 0; q < 5; ++q) std::swap(l.A[q], w.A2[q]);
        l.nine = false;
        galerkin_invalidate(s);
        rc = s->work_f64 ? galerkin_build_t<double>(s, o.transfer) : galerkin_build_t<float>(s, o.transfer);
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
                run.lin_iters += st.cycles;
            }
        }
        if (rc != MGX_OK) { msg = pre + std::to_string(k) + ": " + s->err; break; }
        // backtracking on ||F||: the trial un + lam de with lam = 1, 1/2, ... (the solvers swap u and tmp: l.u afresh)
        double lam = 1.0, r = 0.0;
        bool accepted = false;
        for (int j = 0;;) {
            if ((rc = quasi_pass(s, true, newton, lam, l.b, &r)) != MGX_OK) { msg = pre + std::to_string(k) + ": " + s->err; break; }
            if (r <= (1.0 - 1e-4 * lam) * hist[k]) { accepted = true; break; }       // (NaN rejects)
            ++run.backtracks;
            if (++j > o.max_backtracks) break;
            lam *= 0.5;
        }
        if (rc != MGX_OK) break;
        if (!accepted) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%d: line search failed: smallest lam tried %.17g gave ||F|| = %.17g against %.17g of the iterate", k, lam, r,
                          hist[k]);
            msg = pre + buf;
            break;
        }
        std::swap(w.un, w.ut);
        hist.push_back(r);
        if (step_lengths) step_lengths[k] = lam;
    }
    return rc;
}

// U = the last accepted iterate and B = the workspace's f, on every path of a call; then the status of the call
int quasi_leave(mgx_solver* s, int rc, const std::string& msg)
{
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->qsi;
    const hipError_t e1 = hipMemcpyAsync(l.u, w.un, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    const hipError_t e2 = hipMemcpyAsync(l.b, w.f, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    const hipError_t e3 = hipStreamSynchronize(s->stream);
    s->norm_blocks_ready = 0;
    s->err = msg;
    if (rc != MGX_OK) return rc;
    for (hipError_t e : {e1, e2, e3})
        if (e != hipSuccess) return s->fail(MGX_ERR_HIP, std::string("mgx_quasi: restoring U and B: ") + hipGetErrorString(e));
    return MGX_OK;
}

int quasi(mgx_solver* s, const mgx_quasi_opts& o, const double* a_nodes, mgx_newton_stats* nstats, mgx_stats* lin_stats, double* step_lengths,
          double* history, int history_cap)
{
    const auto t0 = std::chrono::steady_clock::now();
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->qsi;
    if (int rc = quasi_workspace(s, "mgx_quasi")) return rc;
    w.k0 = o.k0; w.k1 = o.k1; w.k2 = o.k2;
    // the (N + 1)^2 nodes, boundary included, into the level's rows and pitch; the padding stays zero
    const size_t row = ((size_t)l.N + 1) * sizeof(double);
    HIPCHK(s, hipMemcpy2DAsync(w.an, (size_t)l.pitch * sizeof(double), a_nodes, row, row, (size_t)l.N + 1, hipMemcpyHostToDevice, s->stream));
    HIPCHK(s, hipMemcpyAsync(w.un, l.u, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipMemcpyAsync(w.f, l.b, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));

    NewtonRun run;
    int rc = quasi_iterate(s, o, lin_stats, step_lengths, run);
    if ((rc = quasi_leave(s, rc, run.msg)) != MGX_OK) return rc;
    newton_report(run, o.tol, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), nstats, history, history_cap);
    return MGX_OK;
}

} // namespace
