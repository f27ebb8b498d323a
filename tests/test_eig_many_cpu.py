"""CPU checks of mgx_eigs_many's pieces that need no device: the numpy statement of the deflated iteration
(tests/eig_many_ref.py) against the closed forms and numpy.linalg.eigvalsh, the header / exports / binding, the resource
remarks of the two projection kernels, and csrc/mgx_eig_many_plan.hpp through a stand-alone C++ program
(host/eig_many_check.cpp) built with -fsanitize=address,undefined and run directly."""
import functools
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eig_many_ref as em
import eig_ref as er
import galerkin_ref as gr
import nine_ref as nr
from conftest import ROOT
from pcg_ref import contrast_coefficient

EPS = np.finfo(np.float64).eps
TOL = 1e-8


def fine_stencil(kind, L):
    if kind.startswith("const"):
        return gr.nine(er.constant_stencil(L, float(kind[5:])))
    if kind.startswith("contrast"):
        return er.coefficient_stencil(contrast_coefficient(L, float(kind[8:])))
    return nr.tensor9(*nr.rotated_tensor(L, 45.0, 0.5))


@functools.lru_cache(maxsize=None)
def exact_values(kind, L, count):
    if kind.startswith("const"):
        return er.constant_eigenvalues(L, float(kind[5:]), count)
    assert L <= 5
    return np.linalg.eigvalsh(gr.dense(fine_stencil(kind, L)))[:count]


def operators(op, kind, L, Lc, transfer=0, cycle=0):
    fine = [np.asarray(a, dtype=np.float64) for a in fine_stencil(kind, L)]
    st = (lambda lv: er.constant_stencil(lv, float(kind[5:]))) if op == "s5" else fine
    h = er.hierarchy(op, st, L, Lc, transfer, cycle)
    return fine, (lambda v: er.apply(fine, v)), er.preconditioner(h)


def check_pairs(fine, res, exact, tol=TOL):
    """the two inequalities of tests/test_gpu_eig.py on every pair, the residual recomputed from the returned pair"""
    lmax = er.lambda_max_bound(fine)
    assert not res.reason and all(res.converged) and res.computed == len(exact)
    assert np.all(np.diff(res.theta) >= 0)
    for j, (th, x) in enumerate(zip(res.theta, res.X)):
        r = np.linalg.norm(er.apply(fine, x) - th * x)
        assert abs(r - res.hist[j][-1]) <= 1e-12 and r <= tol * th
        assert abs(th - exact[j]) <= r + 64 * EPS * lmax, (j, th, exact[j], r)
        assert th >= exact[j] - 64 * EPS * lmax, (j, th, exact[j])
    return er.orthonormality_defect(res.X)


# the issue's numpy experiment at levels 5 and 6: (op, kind, finest, coarsest, nev, transfer, cycle)
CASES = [("gal", "const1.0", 5, 2, 12, 0, 0), ("gal", "const0.5", 5, 2, 10, 0, 0), ("gal", "const1.0", 6, 3, 16, 0, 0),
         ("s5", "const0.5", 6, 3, 9, 0, 0), ("s5", "const1.0", 5, 2, 5, 0, 0), ("gal", "contrast10", 5, 2, 12, 0, 0),
         ("gal", "contrast10", 5, 2, 12, 1, 0), ("gal", "contrast100", 5, 2, 10, 1, 0), ("gal", "rot45", 5, 2, 12, 1, 0),
         ("gal", "rot45", 5, 2, 12, 1, 1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_reference_finds_the_nev_smallest_eigenvalues(case):
    op, kind, L, Lc, nev, transfer, cycle = case
    fine, A, M = operators(op, kind, L, Lc, transfer, cycle)
    res = em.eigs_many(A, M, er.guesses(L, nev), TOL, 200)
    defect = check_pairs(fine, res, exact_values(kind, L, nev))
    print(f"{case}: iterations per block {res.block_iterations}, |X^T X - I| {defect:.2e}")
    assert len(res.block_iterations) == len(em.partition(nev)) and max(res.block_iterations) <= 60
    assert defect <= 1e-12


def test_reference_cuts_a_degenerate_pair():
    """Poisson at level 5: eigenvalues 12 and 13 (counted from one) are equal, and nev = 12 asks for one of them"""
    exact = exact_values("const1.0", 5, 13)
    assert exact[11] == pytest.approx(exact[12], rel=1e-12)


@pytest.mark.parametrize("nev", [1, 2, 3, 4])
def test_one_block_is_eig_ref(nev):
    fine, A, M = operators("gal", "contrast10", 5, 2, 1)
    g = er.guesses(5, nev)
    want, got = er.lobpcg(A, M, g, TOL, 200), em.eigs_many(A, M, g, TOL, 200)
    assert all(want.converged) and got.block_iterations == [want.iterations]
    assert np.array_equal(got.theta, want.theta) and np.array_equal(got.X, want.X)
    assert all(np.array_equal(a, b) for a, b in zip(got.hist, want.hist)) and got.cycles == want.cycles and got.converged == want.converged


def test_reference_stops_at_a_block_that_does_not_converge():
    fine, A, M = operators("gal", "const0.5", 5, 2)
    res = em.eigs_many(A, M, er.guesses(5, 10), TOL, 1)
    assert res.computed == 4 and res.block_iterations == [1] and res.reason.startswith("block 0") and not any(res.converged)
    assert [len(h) for h in res.hist] == [2] * 4 and np.all(np.diff(res.theta) >= 0)


def test_partition_and_order():
    assert [em.partition(n) for n in (1, 4, 5, 9, 16)] == [[1], [4], [4, 1], [4, 4, 1], [4, 4, 4, 4]]
    assert em.stable_order([3.0, 1.0, 3.0, 2.0, 1.0]) == [1, 4, 3, 0, 2]


# ---- header, library and binding -----------------------------------------------------------------------------------------
def test_header_library_and_binding_have_eigs_many(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "#define MGX_EIGS_MAX 16" in text
    assert "MGX_API int mgx_eigs_many(mgx_handle h, int nev, void* x, double* lambda, double tol, int max_iters," in text
    assert "MGX_API int mgx_time_eig_project(mgx_handle h, int pass, int m, int k, int repeats, double* ms);" in text
    assert "enum { MGX_EIG_PROJECT_DOTS = 0, MGX_EIG_PROJECT_SUB = 1 };" in text
    assert {"mgx_eigs_many", "mgx_time_eig_project"} <= set(pkg.EXPORTS)
    assert hasattr(pkg.lib(), "mgx_eigs_many") and hasattr(pkg.lib(), "mgx_time_eig_project")
    assert callable(pkg.Multigrid.eigs_many) and callable(pkg.Multigrid.time_eig_project)
    assert pkg.EIGS_MAX == 16 and (pkg.EIG_PROJECT_DOTS, pkg.EIG_PROJECT_SUB) == (0, 1)
    assert pkg.lib().mgx_eigs_many(None, 1, None, None, 1e-8, 10, None, None, 0) == 1       # MGX_ERR_INVALID: no handle
    assert pkg.lib().mgx_time_eig_project(None, 0, 1, 1, 1, None) == 1


def kernel_counts(pkg, pattern, names):
    txt = "".join(open(f).read() for f in glob.glob(os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "build", pattern)))
    assert txt, "no resource remarks next to the library: build it with __graft_entry__.build()"
    seen = {}
    for b in re.split(r"Function Name: ", txt)[1:]:
        m = re.match(r"_ZN3mgx\d+(" + "|".join(names) + ")I", b)
        if m:
            seen[m.group(1)] = seen.get(m.group(1), 0) + 1
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.splitlines()[0]
    return seen


def test_the_build_has_every_projection_instance_without_scratch(pkg):
    """both types: dots 8 chunk sizes x 4 column counts, subtract 4 column counts; and the four families of mgx_eigs keep
    the counts tests/test_eig_cpu.py pins, in their own compilation"""
    assert kernel_counts(pkg, "inst_12_*.remarks", ["k_eig_project_dots", "k_eig_project_sub"]) == {"k_eig_project_dots": 64, "k_eig_project_sub": 8}
    old = ["k_eig_gram", "k_eig_combine", "k_eig_residual", "k_apply_var_multi"]
    assert kernel_counts(pkg, "inst_11_*.remarks", old) == {"k_eig_gram": 40, "k_eig_combine": 96, "k_eig_residual": 8, "k_apply_var_multi": 16}
    assert kernel_counts(pkg, "inst_12_*.remarks", old) == {}


# ---- csrc/mgx_eig_many_plan.hpp ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("eig_many") / "eig_many_check"
    src = os.path.join(ROOT, "multigrid_nikhil_c-_amd", "host", "eig_many_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), src],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def plan_cases():
    """(nev, computed, history_cap, lambdas, history lengths): every nev, calls that stop after each block, ties in lambda
    inside and across blocks, a history_cap shorter than, equal to and longer than the histories, and cap 0"""
    rng = np.random.default_rng(5)
    out = []
    for nev in range(1, 17):
        sizes = em.partition(nev)
        for stop in range(1, len(sizes) + 1):
            done = sum(sizes[:stop])
            lam = []
            for kb in sizes[:stop]:
                lam += sorted(rng.integers(1, 6, kb).astype(float) if (nev + stop) % 2 else rng.uniform(0.1, 4.0, kb))
            lens = [int(v) for v in rng.integers(1, 9, done)]
            for cap in (0, 3, 8, 11):
                out.append((nev, done, cap, lam, lens))
    return out


def test_plan_header_under_the_sanitizers(plan_program, tmp_path):
    cases = plan_cases()
    assert {c[0] for c in cases} == set(range(1, 17)) and any(c[1] < c[0] for c in cases) and any(len(set(c[3])) < len(c[3]) for c in cases)
    assert any(c[2] < max(c[4]) for c in cases)
    path = tmp_path / "plans.txt"
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for nev, done, cap, lam, lens in cases:
            f.write(f"{nev} {done} {cap}\n" + " ".join(repr(float(v)) for v in lam) + "\n" + " ".join(str(v) for v in lens) + "\n")
    r = subprocess.run([str(plan_program), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 5 * len(cases)
    for i, (nev, done, cap, lam, lens) in enumerate(cases):
        sizes, order, lam_out, hl, hist = (np.array(lines[5 * i + q].split(), dtype=float) for q in range(5))
        assert list(sizes) == em.partition(nev)
        want = em.stable_order(lam)
        # the vectors: slot r holds pair want[r]; the slots behind the computed ones still hold the guesses (-1 - slot)
        assert list(order) == want + [-1 - r for r in range(done, nev)]
        assert list(lam_out) == [lam[p] for p in want] + [0.0] * (nev - done)
        assert list(hl) == [lens[p] for p in want] + [0] * (nev - done)
        # pair p's history is p + 0.001 k; what the slot did not receive is still -7
        exp = np.full((nev, cap), -7.0)
        for r, p in enumerate(want):
            k = min(cap, lens[p])
            exp[r, :k] = p + 0.001 * np.arange(k)
        assert np.array_equal(hist, exp.ravel()), (nev, done, cap)
