"""CPU checks of mgx_solve_multi_refine_gcr and mgx_time_multi_refine_direction (include/mgx.h): the two entry points in
the header with their argument counts, in the library and in the binding; a NULL handle is an invalid argument without a
GPU; and the build's resource remarks hold the eight instances of k_refine_direction, none with scratch (DESIGN.md
5.8 tables their registers).  What the call computes is held to mgx_solve_refine_gcr on the GPU
(tests/test_gpu_multi_refine_gcr.py); that the refinement loop commutes with powers of two is tests/test_refine_gcr_cpu.py's."""
import ctypes as C
import glob
import os
import re

from conftest import ROOT

NAMES = ("mgx_solve_multi_refine_gcr", "mgx_time_multi_refine_direction")


def test_header_library_and_binding_have_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"MGX_API\s+int\s+(mgx_\w+)\s*\(([^;]*)\);", text)}
    solve, time = (decl[n] for n in NAMES)
    assert solve.count(",") == 9 and "mgx_stats" in solve and "int nrhs" in solve and "int restart" in solve
    assert time.count(",") == 3 and "mgx_handle" in time and "int nrhs" in time
    # declared after mgx_solve_multi_gcr, with its argument list
    assert text.index("mgx_solve_multi_gcr(mgx_handle") < text.index("mgx_solve_multi_refine_gcr(mgx_handle")
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(solve) == norm(decl["mgx_solve_multi_gcr"])
    L = C.CDLL(pkg.LIB_PATH)
    assert all(hasattr(L, n) for n in NAMES)
    assert set(NAMES) <= set(pkg.EXPORTS)
    assert len(pkg.lib().mgx_solve_multi_refine_gcr.argtypes) == 10 and len(pkg.lib().mgx_time_multi_refine_direction.argtypes) == 4
    assert callable(getattr(pkg.Multigrid, "solve_multi_refine_gcr", None))
    assert callable(getattr(pkg.Multigrid, "time_multi_refine_direction", None))


def test_a_null_handle_is_an_invalid_argument(pkg):
    """not a crash, and no GPU is touched"""
    assert pkg.lib().mgx_solve_multi_refine_gcr(None, 1, None, None, 1e-8, 1, 4, None, None, 0) == 1
    assert pkg.lib().mgx_time_multi_refine_direction(None, 1, 1, None) == 1


def test_no_instance_of_the_direction_kernel_uses_scratch(pkg):
    """the build leaves every kernel's resource usage in csrc/build/*.remarks: NQ = 5, 9 and K = 1, 2, 3, 4 are there (K = 1 is
    mgx_solve_refine_gcr's own pass), each without scratch and without spilled registers (four nine-point columns are one launch, not two of two)"""
    txt = "".join(open(f).read() for f in glob.glob(os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "build", "*.remarks")))
    seen = {}
    for m in re.finditer(r"Function Name: \S*k_refine_directionILi(\d)ELi(\d)E\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)",
                         txt, re.S):
        seen[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)))
    assert set(seen) == {(nq, k) for nq in (5, 9) for k in (1, 2, 3, 4)}, sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
