// mgx_theta_host.hpp - the host side of mgx_set_reaction / mgx_get_reaction, mgx_theta_steps and mgx_time_theta_rhs
// (absent in the reference; the kernels and the arithmetic are mgx_theta.hpp's).  Included by mgx.hip
// after the solvers' host headers.
#pragma once

namespace {

void reaction_free(mgx_solver::ReactionWs& w)
{
    for (void** p : {&w.c0, &w.d, &w.g}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    w.set = false;
}

// which handles carry a zero-order term (the message names the reason), and the finest operator must have been given
int reaction_guard(mgx_solver* s, const char* fn)
{
    NO_DIST(s)
    if (!s->var) return s->fail(MGX_ERR_STATE, std::string(fn) + ": handle was created with op = MGX_OPERATOR_POISSON (the constant stencil has no coefficients)");
    if (!s->galerkin)
        return s->fail(MGX_ERR_STATE, std::string(fn) + ": op = MGX_OPERATOR_STENCIL5: the caller owns every level's stencil and adds the term there "
                                                        "(mgx_set_stencil); this entry point is for MGX_OPERATOR_GALERKIN");
    if (!s->lv[s->cfg.finest_level].stencil_set)
        return s->fail(MGX_ERR_STATE, std::string(fn) + ": finest operator not set (mgx_set_stencil / mgx_set_coefficient / mgx_set_stencil9 / mgx_set_tensor)");
    return MGX_OK;
}

// one finest-level grid of the workspace exists, zeroed (ring and padding stay zero: only interiors are written)
int reaction_grid(mgx_solver* s, void** p, const char* fn, const char* what)
{
    if (*p) return MGX_OK;
    if (!alloc_zeroed(s, p, s->lv[s->cfg.finest_level].bytes)) return s->fail(MGX_ERR_ALLOC, std::string(fn) + ": allocation failed for " + what);
    return MGX_OK;
}

// the device half of mgx_set_reaction, in two steps (c0 and d exist).  reaction_base: c0 holds the centre of A0 - copied
// from slot 0 unless a term is set (then slot 0 is shifted and c0 already holds it).  reaction_shift: slot 0 = c0 + d from
// the d on the device (mgx_set_reaction uploads it; mgx_newton's pass wrote it there), the hierarchy invalidated
int reaction_base(mgx_solver* s)
{
    Level& l = s->lv[s->cfg.finest_level];
    if (!s->rx.set) HIPCHK(s, hipMemcpyAsync(s->rx.c0, l.A[0], l.bytes, hipMemcpyDeviceToDevice, s->stream));
    return MGX_OK;
}

int reaction_shift(mgx_solver* s)
{
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->rx;
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        launch_reaction_shift<T>((const T*)w.c0, (const T*)w.d, (T*)l.A[0], l.N, l.pitch, s->stream);
    });
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    galerkin_invalidate(s);
    w.set = true;
    return MGX_OK;
}

int set_reaction(mgx_solver* s, const void* d, size_t count)
{
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->rx;
    if (!d) {
        if (!w.set) return MGX_OK;                            // nothing to remove: hierarchy and graphs stay
        HIPCHK(s, hipMemcpyAsync(l.A[0], w.c0, l.bytes, hipMemcpyDeviceToDevice, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));
        galerkin_invalidate(s);                               // (lowers w.set)
        return MGX_OK;
    }
    const size_t n = (size_t)l.N - 1;
    if (count != n * n) return s->fail(MGX_ERR_INVALID, "mgx_set_reaction: vector length must be n*n with n = 2^finest_level - 1");
    // both grids before anything is touched: a failure leaves the operator and the hierarchy as they were
    if (int rc = reaction_grid(s, &w.c0, "mgx_set_reaction", "the base centre")) return rc;
    if (int rc = reaction_grid(s, &w.d, "mgx_set_reaction", "the zero-order term")) return rc;
    if (int rc = reaction_base(s)) return rc;
    if (int rc = copy_in(s, l, w.d, d, count)) return rc;
    return reaction_shift(s);
}

// one launch of k_theta_rhs on the finest level: out <- the right-hand side of a theta step from u
void theta_rhs(mgx_solver* s, double theta, const void* u, const void* g, void* out)
{
    const Level& l = s->lv[s->cfg.finest_level];
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        launch_theta_rhs<T>(var_level<T>(l), (const T*)u, (const T*)s->rx.d, (const T*)g, (T*)out, theta, s->stream);
    });
}

int theta_steps(mgx_solver* s, double theta, int nsteps, const void* g, int solver, double tol, int max_iters, int restart, int* steps_done,
                mgx_stats* stats, double* history, int history_cap)
{
    Level& l = s->lv[s->cfg.finest_level];
    const size_t n = (size_t)l.N - 1;
    if (g) {
        if (int rc = reaction_grid(s, &s->rx.g, "mgx_theta_steps", "the source term")) return rc;
        if (int rc = copy_in(s, l, s->rx.g, g, n * n)) return rc;
    }
    for (int k = 0; k < nsteps; ++k) {
        theta_rhs(s, theta, l.u, g ? s->rx.g : nullptr, l.b);        // (l.u afresh: the solvers swap u and tmp)
        HIPCHK(s, hipGetLastError());
        s->norm_blocks_ready = 0;
        s->err.clear();
        mgx_stats st{};
        double* const hk = history ? history + (size_t)k * (size_t)history_cap : nullptr;
        int rc = MGX_OK;
        if (solver == MGX_STEP_SOLVE) rc = mgx_solve(s, tol, max_iters, &st, hk, history_cap);
        else if (solver == MGX_STEP_GCR) rc = mgx_solve_gcr(s, tol, max_iters, restart, &st, hk, history_cap);
        else rc = mgx_solve_refine_gcr(s, tol, max_iters, restart, &st, hk, history_cap);
        if (rc) {
            s->err = "mgx_theta_steps: step " + std::to_string(k) + ": " + s->err;
            return rc;
        }
        if (stats) stats[k] = st;
        if (steps_done) *steps_done = k + 1;
        if (!st.converged) {
            s->err = "mgx_theta_steps: step " + std::to_string(k) + " did not converge: " +
                     (s->err.empty() ? "residual " + std::to_string(st.final_residual / st.initial_residual) + " of the initial one after max_iters = " +
                                           std::to_string(max_iters) + " iterations"
                                     : s->err) +
                     "; the later steps were not taken";
            break;
        }
    }
    return MGX_OK;
}

} // namespace
