// ref_api_check.cpp — runs every function of include/mgx_reference_api.hpp once on the device, the way
// Poissons_SYCL.cpp calls them (PS:575-650, 725-727), and leaves what each returned in files, so that
// tests/test_gpu_ref_api.py can hold the vectors to the oracle bit for bit and the documented conventions
// (jacobirelaxation mutates v and returns it, PS:146; vcyclemultigrid clobbers vec_h, PS:581; levels are
// inferred from vector lengths, PS:583) to what the header says.  Plain C++ on the header alone.
//
//   ref_api_check <input dir> <output dir>
//
// Input: raw little-endian float32 files v8, f8, u8, b8 (255^2 values each) and e6 (63^2).  Output: one raw
// file per result (float32; fmg_f64 and solve_hist as float64) and status.txt.  Real = float on levels 8..6
// with mu0 1, mu1 3, mu2 2; one Real = double call at the end so that both instantiations run.
#include "mgx_reference_api.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>

using namespace mgxref;

template <typename T> static std::vector<T> read_raw(const std::string& path, std::size_t count)
{
    std::vector<T> v(count);
    std::ifstream in(path, std::ios::binary);
    in.read(reinterpret_cast<char*>(v.data()), std::streamsize(count * sizeof(T)));
    if (!in || in.gcount() != std::streamsize(count * sizeof(T)) || in.peek() != std::ifstream::traits_type::eof())
        throw std::runtime_error("cannot read " + std::to_string(count) + " values from " + path);
    return v;
}

template <typename T> static void write_raw(const std::string& path, const std::vector<T>& v)
{
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char*>(v.data()), std::streamsize(v.size() * sizeof(T)));
    out.close();
    if (!out) throw std::runtime_error("cannot write " + path);
}

static int run(const std::string& in, const std::string& out)
{
    parameters prm;
    prm.finest_level = 8;
    prm.coarsest_level = 6;
    prm.mu0 = 1; prm.mu1 = 3; prm.mu2 = 2;
    const std::size_t n8 = 255 * 255, n6 = 63 * 63;
    std::vector<float> v = read_raw<float>(in + "/v8", n8), f = read_raw<float>(in + "/f8", n8);
    std::vector<float> vec_h = read_raw<float>(in + "/u8", n8), f_h = read_raw<float>(in + "/b8", n8);
    std::vector<float> e = read_raw<float>(in + "/e6", n6);
    std::ofstream status(out + "/status.txt");

    queue q;                                                                            // PS:659
    // 1. the per-level loop of main() (PS:661-690)
    std::vector<matrix_elements_for_jacobi>& jacobi_matrices = build_hierarchy<float>(prm);
    status << "entries " << jacobi_matrices.size() << "\n";
    for (const matrix_elements_for_jacobi& a : jacobi_matrices) status << "size " << a.size << " level " << a.level << "\n";
    matrix_elements_for_jacobi& a_h = jacobi_matrices[jacobi_matrices.size() - 1];

    // 2. the six-argument form, as PS:581 calls it
    write_raw(out + "/jacobi_ret", jacobirelaxation(q, a_h.a_lu_handle, a_h.size, v, f, prm.mu1));
    write_raw(out + "/jacobi_v", v);

    // 3. the transfers (PS:611, 620): levels from the vector lengths
    write_raw(out + "/restrict", restriction2d(f));
    write_raw(out + "/interp", interpolation2d(e));

    // 4. PS:575
    write_raw(out + "/vcycle_ret", vcyclemultigrid(q, a_h, vec_h, f_h));
    write_raw(out + "/vcycle_vec_h", vec_h);

    // 5. PS:727, 725
    write_raw(out + "/fmg", fullmultigrid(q, a_h, f_h));
    write_raw(out + "/force", globalforcefunction<float>());

    // 6. MF:193
    mgx_stats stats{};
    std::vector<double> history;
    write_raw(out + "/solve_u", multigrid_solver(f_h, 0.0, 3, &stats, &history));
    write_raw(out + "/solve_hist", history);
    status << "cycles " << stats.cycles << "\n";

    // 7. a_size that is not the level's: the header's one check of it
    try {
        jacobirelaxation(q, a_h.a_lu_handle, a_h.size - 1, v, f, prm.mu1);
        status << "wrong a_size: no error\n";
    } catch (const std::runtime_error&) {
        status << "wrong a_size: caught\n";
    }

    // Real = double: MF's precision
    std::vector<matrix_elements_for_jacobi>& jm64 = build_hierarchy<double>(prm);
    std::vector<double> f64(f_h.begin(), f_h.end());
    write_raw(out + "/fmg_f64", fullmultigrid(q, jm64[jm64.size() - 1], f64));
    status << "double entries " << jm64.size() << "\n";
    status.close();
    if (!status) throw std::runtime_error("cannot write " + out + "/status.txt");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: ref_api_check <input dir> <output dir>\n");
        return 2;
    }
    try {
        return run(argv[1], argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_api_check: %s\n", e.what());
        return 1;
    }
}
