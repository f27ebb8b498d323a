"""CPU checks of the drop-in boundary: libmgx.so loads, exports every symbol
include/mgx.h declares, and refuses to run without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, have_gpu


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    return sorted(set(re.findall(r"MGX_API\s+[\w\s\*]+?\b(mgx_\w+)\s*\(", text)))


def test_header_and_binding_agree(pkg):
    declared = _declared_symbols()
    assert declared, "no MGX_API declarations found"
    assert sorted(pkg.EXPORTS) == declared


def test_library_exports_every_declared_symbol(pkg):
    L = pkg.lib()
    for name in _declared_symbols():
        assert hasattr(L, name), f"libmgx.so does not export {name}"


def test_only_the_c_abi_is_exported(pkg):
    # -fvisibility=hidden: nothing but the mgx_* C symbols leaves the library
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if " T " in ln]
    assert names and all(n.startswith("mgx_") for n in names), names


def test_struct_layouts_match_the_header(pkg, tmp_path):
    # ask the C compiler what include/mgx.h lays out and compare with ctypes
    import subprocess

    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mgx_config), offsetof(mgx_config, omega),'
        ' offsetof(mgx_config, profile), sizeof(mgx_stats), offsetof(mgx_stats, fine_updates),'
        ' sizeof(mgx_profile), sizeof(mgx_slab)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    from multigrid_nikhil_c_amd import binding as B

    assert got == [C.sizeof(B.Config), B.Config.omega.offset, B.Config.profile.offset, C.sizeof(B.Stats),
                   B.Stats.fine_updates.offset, C.sizeof(B.Profile), C.sizeof(B.Slab)]


def test_defaults_are_the_reference_globals(pkg):
    c = pkg.default_config()
    # PS:17-22, PS:127
    assert (c.finest_level, c.coarsest_level, c.mu0, c.mu1, c.mu2) == (10, 7, 30, 10, 10)
    assert c.omega == 2.0 / 3.0
    assert c.schedule == pkg.SCHEDULE_FMG and c.smoother == pkg.SMOOTHER_JACOBI


def test_geometry_helpers(pkg):
    L = pkg.lib()
    assert L.mgx_level_n(10) == 1023 and L.mgx_level_n(7) == 127     # PS:662-664
    # rows are 256-byte multiples and hold columns 0..N
    for lvl in (2, 5, 7, 13):
        for dt, es in ((pkg.DTYPE_F32, 4), (pkg.DTYPE_F64, 8)):
            p = L.mgx_level_pitch(lvl, dt)
            assert p >= (1 << lvl) + 1 and (p * es) % 256 == 0
    assert L.mgx_level_pitch(0, pkg.DTYPE_F64) == -1


def test_invalid_configs_are_rejected(pkg):
    for bad in (dict(finest_level=5, coarsest_level=6), dict(coarsest_level=1), dict(omega=0.0),
                dict(dtype=7), dict(finest_level=12, coarsest_level=9)):
        with pytest.raises(pkg.MgxError):
            pkg.Multigrid(**bad)


@pytest.mark.skipif(have_gpu(), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    with pytest.raises(pkg.MgxError, match="no usable HIP device"):
        pkg.Multigrid()
    # slab operators validate their arguments before touching the device
    s = pkg.Slab(level=1, dtype=pkg.DTYPE_F64, rows=4, row0=0)
    assert pkg.lib().mgx_slab_scratch_doubles(C.byref(s)) == -1


def test_no_kernel_uses_scratch():
    """Register-resident row windows are the whole point of the fused kernels: a
    spill (scratch) silently costs 30-60 %.  Every compile of the library leaves its kernels'
    resource usage in csrc/build/*.remarks (-Rpass-analysis=kernel-resource-usage): bring the build
    up to date and check every kernel's ScratchSize (this caught a run-time-indexed state array)."""
    import glob
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "multigrid_nikhil_c-_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    txt = "".join(open(f).read() for f in glob.glob(os.path.join(csrc, "build", "*.remarks")))
    sizes = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(sizes) > 300, "resource-usage remarks missing"
    assert max(sizes) == 0, f"{sum(1 for x in sizes if x)} kernels use scratch (max {max(sizes)} B/lane)"


def test_reference_signatures_compile_as_the_reference_calls_them(tmp_path):
    """include/mgx_reference_api.hpp: the free functions with the reference's own argument lists -
    jacobirelaxation in its six-argument form exactly as PS:581 calls it, vcyclemultigrid /
    fullmultigrid / restriction2d / interpolation2d as PS:617-645, 727 do (compile only: no GPU)."""
    import subprocess

    src = tmp_path / "calls.cpp"
    src.write_text(
        '#include "mgx_reference_api.hpp"\n'
        'using namespace mgxref;\n'
        'std::vector<float> like_ps(queue& q, matrix_elements_for_jacobi& a_h, std::vector<float>& vec_h, std::vector<float>& f_h) {\n'
        '    const int mu1 = 10;\n'
        '    vec_h = jacobirelaxation(q, a_h.a_lu_handle, a_h.size, vec_h, f_h, mu1);   // PS:581\n'
        '    std::vector<float> r = restriction2d(f_h);                                 // PS:611, 641\n'
        '    std::vector<float> p = interpolation2d(r);                                 // PS:620, 645\n'
        '    std::vector<float> v = vcyclemultigrid(q, a_h, vec_h, f_h);                // PS:617\n'
        '    return fullmultigrid(q, a_h, f_h);                                         // PS:727\n'
        '}\n'
        'static_assert(sizeof(matrix_handle_t) > 0, "");\n'
        'int main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_reference_level_inference_from_vector_lengths(pkg, tmp_path):
    """mgxref::level_of_size: the reference infers a vector's level as int(log2(sqrt(size) + 1)) in floating
    point (PS:583, 616, 634); for n = 2^L - 1 the argument of log2 is exactly 2^L only if sqrt and log2 are
    exact there - every level the library accepts (2..15) must come out as L, not L - 1"""
    import subprocess

    src = tmp_path / "levels.cpp"
    src.write_text(
        '#include "mgx_reference_api.hpp"\n'
        '#include <cstdio>\n'
        'int main() {\n'
        '    int bad = 0;\n'
        '    for (int L = 2; L <= 15; ++L) {\n'
        '        const std::size_t n = (std::size_t(1) << L) - 1;\n'
        '        const int got = mgxref::level_of_size(n * n);\n'
        '        std::printf("%d %d\\n", L, got);\n'
        '        bad += got != L;\n'
        '    }\n'
        '    return bad;\n'
        '}\n')
    exe = tmp_path / "levels"
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "undefined reference" in r.stderr:
        # a compiler that emits the header's unused inline wrappers wants the library they call
        libdir = os.path.dirname(pkg.LIB_PATH)
        r = subprocess.run(cmd + ["-L", libdir, "-lmgx", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    assert [ln.split() for ln in out.stdout.splitlines()] == [[str(L), str(L)] for L in range(2, 16)]
