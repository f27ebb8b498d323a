// eig_dense_check.cpp - csrc/mgx_eig_dense.hpp on pencils read from a text file, for tests/test_eig_cpu.py (which builds this
// program with -fsanitize=address,undefined and runs it directly; no HIP, no device).
//   input:  the number of pencils, then per pencil: n nev, the n*n entries of G, the n*n entries of H (row-major)
//   output: per pencil "ok" and a line of nev theta and a line of n*nev entries of C (row-major), or "deficient index pivot"
#include "../csrc/mgx_eig_dense.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s pencils.txt\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    int count = 0;
    if (std::fscanf(f, "%d", &count) != 1) return 2;
    for (int p = 0; p < count; ++p) {
        int n = 0, nev = 0;
        if (std::fscanf(f, "%d %d", &n, &nev) != 2 || n < 1 || n > mgx_eig_dense::kMax || nev < 1 || nev > n) return 2;
        std::vector<double> G(n * n), H(n * n), theta(nev), C(n * nev);
        for (double& v : G) if (std::fscanf(f, "%lf", &v) != 1) return 2;
        for (double& v : H) if (std::fscanf(f, "%lf", &v) != 1) return 2;
        const mgx_eig_dense::Result r = mgx_eig_dense::rayleigh_ritz(n, nev, G.data(), H.data(), theta.data(), C.data());
        if (!r.ok) { std::printf("deficient %d %.17g\n", r.index, r.pivot); continue; }
        std::printf("ok\n");
        for (double v : theta) std::printf("%.17g ", v);
        std::printf("\n");
        for (double v : C) std::printf("%.17g ", v);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
