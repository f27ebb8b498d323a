// eig_many_check.cpp - csrc/mgx_eig_many_plan.hpp on cases read from a text file, for tests/test_eig_many_cpu.py (which builds
// this program with -fsanitize=address,undefined and runs it directly; no HIP, no device).
//   input:  the number of cases, then per case: nev computed history_cap, the `computed` lambdas (as computed, block after
//           block), the `computed` history lengths.  Pair p has the history p, p + 0.001, p + 0.002, ...; the caller's
//           vector slot r holds -1 - r (its guess), pair p's vector is p
//   output: per case five lines: the block sizes; what the nev vector slots hold; lambda; history_len of the nev stats; the
//           nev * history_cap history entries (prefilled with -7).  Every array is allocated at its exact size, so an
//           overrun is the sanitizer's to report
#include "../csrc/mgx_eig_many_plan.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char** argv)
{
    namespace em = mgx_eig_many;
    if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    int count = 0;
    if (std::fscanf(f, "%d", &count) != 1) return 2;
    for (int c = 0; c < count; ++c) {
        int nev = 0, done = 0, cap = 0;
        if (std::fscanf(f, "%d %d %d", &nev, &done, &cap) != 3 || nev < 1 || nev > em::kMax || done < 1 || done > nev || cap < 0) return 2;
        std::vector<int> size((nev + em::kBlockMax - 1) / em::kBlockMax);
        const int nb = em::partition(nev, size.data());
        if (nb != (int)size.size()) return 3;
        std::vector<em::Pair> pair(done);
        std::vector<std::vector<double>> hist(done);
        for (int p = 0; p < done; ++p)
            if (std::fscanf(f, "%lf", &pair[p].lambda) != 1) return 2;
        for (int p = 0; p < done; ++p) {
            int len = 0;
            if (std::fscanf(f, "%d", &len) != 1 || len < 1) return 2;
            for (int k = 0; k < len; ++k) hist[p].push_back(p + 0.001 * k);
            pair[p].hist = &hist[p];
            pair[p].cycles = len - 1;
            pair[p].converged = p % 2 == 0;
            pair[p].fine_updates = 10.0 * p;
        }
        std::vector<double> lambda(nev, -3.0), history((size_t)nev * cap, -7.0), vec(nev);
        std::vector<mgx_stats> stats(nev);
        for (int r = 0; r < nev; ++r) { vec[r] = -1.0 - r; stats[r].history_len = -5; stats[r].cycles = -5; }
        const int rc = em::scatter(nev, done, pair.data(), 1.5, lambda.data(), stats.data(), cap ? history.data() : nullptr, cap,
                                   [&](int p, int slot) { vec.at(slot) = p; return MGX_OK; });
        if (rc != MGX_OK) return 3;
        // the same call without stats and history writes the same lambdas and touches nothing else
        std::vector<double> lambda2(nev, -3.0);
        if (em::scatter(nev, done, pair.data(), 1.5, lambda2.data(), nullptr, nullptr, cap, [](int, int) { return MGX_OK; }) != MGX_OK || lambda2 != lambda)
            return 3;
        for (int r = 0; r < nev; ++r) {
            const mgx_stats& st = stats[r];
            const int p = (int)vec[r];
            if (r < done) {
                if (st.cycles != st.history_len - 1 || st.converged != (p % 2 == 0) || st.fine_updates != 10.0 * p || st.seconds != 1.5 ||
                    st.initial_residual != hist[p].front() || st.final_residual != hist[p].back())
                    return 4;
            } else if (st.cycles || st.converged || st.initial_residual != 0.0 || st.final_residual != 0.0 || st.seconds != 0.0 || st.fine_updates != 0.0)
                return 4;
        }
        for (int b = 0; b < nb; ++b) std::printf("%d ", size[b]);
        std::printf("\n");
        for (double v : vec) std::printf("%.17g ", v);
        std::printf("\n");
        for (double v : lambda) std::printf("%.17g ", v);
        std::printf("\n");
        for (const mgx_stats& st : stats) std::printf("%d ", st.history_len);
        std::printf("\n");
        for (double v : history) std::printf("%.17g ", v);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
