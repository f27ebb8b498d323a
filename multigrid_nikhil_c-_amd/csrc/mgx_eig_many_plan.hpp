// mgx_eig_many_plan.hpp - the host bookkeeping of mgx_eigs_many in plain C++ (no HIP; host/eig_many_check.cpp runs it under
// the sanitizers): the block partition of nev, the stable order of the computed pairs, and the scatter of vectors, stats
// and history slots into the caller's arrays under that order.
#pragma once

#include <vector>

#include "../../include/mgx.h"

namespace mgx_eig_many {

constexpr int kMax = MGX_EIGS_MAX;
constexpr int kBlockMax = MGX_MAX_RHS;

// nev = size[0] + size[1] + ...: blocks of kBlockMax, the last one the rest; returns the number of blocks
inline int partition(int nev, int* size)
{
    int nb = 0;
    for (int done = 0; done < nev; done += kBlockMax) size[nb++] = nev - done < kBlockMax ? nev - done : kBlockMax;
    return nb;
}

// order[r] = the pair (numbered as computed: block after block) that comes r-th by ascending lambda.  Stable: pairs of
// equal lambda keep the order in which they were computed, and so does a pair whose lambda compares with nothing (NaN).
// An insertion sort: a block that is ascending in itself is never reordered
inline void stable_order(int done, const double* lambda, int* order)
{
    for (int p = 0; p < done; ++p) {
        int r = p;
        while (r > 0 && lambda[p] < lambda[order[r - 1]]) { order[r] = order[r - 1]; --r; }
        order[r] = p;
    }
}

// what one computed pair brings along
struct Pair {
    double lambda = 0.0;
    const std::vector<double>* hist = nullptr;       // its residual history (never empty)
    int cycles = 0;
    bool converged = false;
    double fine_updates = 0.0;
};

// the caller's arrays for nev pairs of which the first `done` were computed: slot r receives pair order[r] - its lambda,
// its stats (NULL: none), the first history_cap entries of its history (NULL: none) and, through copy_vector(pair, slot),
// its vector.  The slots done .. nev - 1 get lambda = 0 and all-zero stats; their vectors and history slots are not
// touched.  Returns MGX_OK or the first status copy_vector returned
template <typename CopyVector>
int scatter(int nev, int done, const Pair* pair, double seconds, double* lambda, mgx_stats* stats, double* history, int history_cap,
            CopyVector copy_vector)
{
    double lam[kMax];
    int order[kMax];
    for (int p = 0; p < done; ++p) lam[p] = pair[p].lambda;
    stable_order(done, lam, order);
    for (int r = 0; r < done; ++r) {
        const Pair& q = pair[order[r]];
        if (int rc = copy_vector(order[r], r)) return rc;
        lambda[r] = q.lambda;
        if (stats) {
            mgx_stats& st = stats[r];
            st.cycles = q.cycles;
            st.initial_residual = q.hist->front();
            st.final_residual = q.hist->back();
            st.converged = q.converged ? 1 : 0;
            st.seconds = seconds;
            st.fine_updates = q.fine_updates;
            st.history_len = (int)q.hist->size();
        }
        if (history) {
            double* slot = history + (size_t)r * (size_t)history_cap;
            for (int i = 0; i < (int)q.hist->size() && i < history_cap; ++i) slot[i] = (*q.hist)[i];
        }
    }
    for (int r = done; r < nev; ++r) {
        lambda[r] = 0.0;
        if (stats) stats[r] = mgx_stats{};
    }
    return MGX_OK;
}

} // namespace mgx_eig_many
