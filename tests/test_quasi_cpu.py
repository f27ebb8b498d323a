"""tests/quasi_ref.py, the numpy statement of mgx_quasi, held to scalar arithmetic, to mgx_set_coefficient's discretisation,
to difference quotients and to the convergence the method promises - and the entry points' NULL refusals through libmgx.so
(no device needed)."""
import ctypes as C

import numpy as np
import pytest

import galerkin_ref as gr
import nine_ref as nr
import pcg_ref
import quasi_ref as qr

INVALID = 1
K = (1.0, 0.0, 1.0)


def random_input(L, dtype, seed=3):
    N = 1 << L
    n = N - 1
    rng = np.random.default_rng(seed)
    a = rng.uniform(1.0, 10.0, (N + 1, N + 1))
    u, de, f = (rng.uniform(-1.0, 1.0, (n, n)).astype(dtype) for _ in range(3))
    return a, u, de, f


def scalar_pass(a, k, f, u, de, lam, method):
    """the pass one point at a time with scalars of the working type (coefficients: float64 scalars, rounded once)"""
    dt = u.dtype.type
    d = np.float64
    N = a.shape[0] - 1
    k0, k1, k2 = (d(x) for x in k)
    kk2 = d(2.0 * float(k[2]))
    half = d(0.5)
    v = np.zeros((N + 1, N + 1), dtype=u.dtype)
    for i in range(1, N):
        for j in range(1, N):
            v[i, j] = u[i - 1, j - 1] if de is None else dt(u[i - 1, j - 1] + dt(dt(lam) * de[i - 1, j - 1]))
    kap = lambda i, j: d(a[i, j]) * ((k2 * d(v[i, j]) + k1) * d(v[i, j]) + k0)
    dk = lambda i, j: d(a[i, j]) * (kk2 * d(v[i, j]) + k1)
    b = np.zeros_like(u)
    out = [np.zeros_like(u) for _ in range(5)]
    for i in range(1, N):
        for j in range(1, N):
            nb = ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1))                # n, s, w, e
            fn, fs, fw, fe = (half * (kap(i, j) + kap(*x)) for x in nb)
            ctr = ((fn + fw) + fe) + fs
            cP, nP, sP, wP, eP = dt(ctr), dt(-fn), dt(-fs), dt(-fw), dt(-fe)
            # CSR order N, W, C, E, S, the first term starting the sum
            q = dt(nP * v[i - 1, j])
            q = dt(q + dt(wP * v[i, j - 1]))
            q = dt(q + dt(cP * v[i, j]))
            q = dt(q + dt(eP * v[i, j + 1]))
            q = dt(q + dt(sP * v[i + 1, j]))
            b[i - 1, j - 1] = dt(f[i - 1, j - 1] - q)
            if method == qr.PICARD:
                vals = (cP, nP, sP, wP, eP)
            else:
                gN, gS, gW, gE = (d(v[i, j]) - d(v[x]) for x in nb)
                sg = ((gN + gW) + gE) + gS
                vals = (dt(ctr + (half * dk(i, j)) * sg), dt((half * dk(*nb[0])) * gN - fn), dt((half * dk(*nb[1])) * gS - fs),
                        dt((half * dk(*nb[2])) * gW - fw), dt((half * dk(*nb[3])) * gE - fe))
            for o, x in zip(out, vals):
                o[i - 1, j - 1] = x
    return v[1:N, 1:N], b, out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", [qr.PICARD, qr.NEWTON])
def test_the_pass_point_by_point_against_scalars(dtype, method):
    """first evaluation and a trial (lam = 1/2), random a in [1, 10] and random u, L = 4: v, b and the five grids bit for bit"""
    a, u, de, f = random_input(4, dtype)
    k = (1.25, -0.5, 0.75)
    for d_, lam in ((None, None), (de, 0.5)):
        v, b, coefs, _ = qr.quasi_pass(a, k, f, u, d_, lam, method)
        sv, sb, scoefs = scalar_pass(a, k, f, u, d_, lam, method)
        assert v.dtype == b.dtype == np.dtype(dtype) and all(c.dtype == np.dtype(dtype) for c in coefs)
        assert np.array_equal(v, sv) and np.array_equal(b, sb)
        for c, sc in zip(coefs, scoefs):
            assert np.array_equal(c, sc)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_constant_k_is_set_coefficient_and_one_linear_solve(dtype):
    """k1 = k2 = 0: the Picard grids are mgx_set_coefficient's for k0 a bit for bit, the Newton grids equal them, and the
    loop is one linear solve with lam = 1"""
    a, u, de, f = random_input(4, dtype, seed=5)
    k = (2.5, 0.0, 0.0)
    want = nr.tensor9(k[0] * a, np.zeros_like(a), k[0] * a, dtype)[:5]
    for d_, lam in ((None, None), (de, 0.25)):
        _, bp, pic, _ = qr.quasi_pass(a, k, f, u, d_, lam, qr.PICARD)
        _, bn, new, _ = qr.quasi_pass(a, k, f, u, d_, lam, qr.NEWTON)
        for w, p, q in zip(want, pic, new):
            assert np.array_equal(np.asarray(w), p) and np.array_equal(p, q)
        assert np.array_equal(bp, bn)
    for method in (qr.PICARD, qr.NEWTON):
        a64, u64, _, f64 = random_input(4, np.float64, seed=5)
        r = qr.quasi(a64, k, f64, u64, qr.dense_solve, 1e-10, 10, 4, method=method)
        assert r["converged"] and len(r["hist"]) == 2 and list(r["lam"]) == [1.0] and r["backtracks"] == 0


def jacobian_error():
    a, u, _, f = random_input(4, np.float64, seed=7)
    n = u.shape[0]
    J = gr.dense(gr.nine(qr.quasi_pass(a, K, f, u, method=qr.NEWTON)[2]))
    eps = 1e-4
    D = np.zeros_like(J)
    for j in range(n * n):
        e = np.zeros(n * n)
        e[j] = eps
        e = e.reshape(n, n)
        D[:, j] = (qr.residual(a, K, f, u - e) - qr.residual(a, K, f, u + e)).ravel() / (2.0 * eps)      # F = -residual
    return float(np.abs(D - J).max() / np.abs(J).max())


def test_the_newton_grids_are_the_jacobian_of_F():
    """the matrix assembled from the Newton pass against central differences of F, eps = 1e-4, float64, L = 4, random a in
    [1, 10], random u in [-1, 1], k = (1, 0, 1): max |D - J| / max |J| measured 2.32e-9 on the CPU (deterministic: the
    cubic's third derivative times eps^2 / 6); bound 2.32e-8, ten times that"""
    err = jacobian_error()
    print("jacobian error", err)
    assert err <= 2.32e-8


def contrast_problem(L, fscale):
    N = 1 << L
    n = N - 1
    return pcg_ref.contrast_coefficient(L, 10), np.full((n, n), fscale / N ** 2), np.zeros((n, n))


def test_convergence_with_dense_solves():
    """contrast 10, k = (1, 0, 1), f = 100 / N^2, zero guess, tol 1e-10, L = 4, dense float64 solves.  Newton: 5 iterations,
    all lam = 1, ratios 2.1e-1, 5.6e-2, 2.8e-3, 6.3e-6, 3.6e-5 (the last at rounding level).  Picard: 11 iterations, all
    lam = 1, ratios 0.214, 0.153, 0.125, 0.103, 0.092, 0.084, 0.080, 0.076, 0.074, 0.072, 0.071"""
    a, f, u0 = contrast_problem(4, 100.0)
    nw = qr.quasi(a, K, f, u0, qr.dense_solve, 1e-10, 40, 8, method=qr.NEWTON)
    pc = qr.quasi(a, K, f, u0, qr.dense_solve, 1e-10, 40, 8, method=qr.PICARD)
    for r, its in ((nw, 5), (pc, 11)):
        print(r["hist"][1:] / r["hist"][:-1])
        assert r["converged"] and not r["failed"] and len(r["hist"]) == its + 1 and (r["lam"] == 1.0).all() and r["backtracks"] == 0
    ratios = nw["hist"][1:] / nw["hist"][:-1]
    assert ratios[3] < 1e-3 * ratios[0]                       # quadratic: the contraction itself contracts
    ratios = pc["hist"][1:] / pc["hist"][:-1]
    assert 0.05 < ratios[-1] < 0.1                            # linear: the contraction settles
    assert np.abs(nw["u"] - pc["u"]).max() <= 1e-8 * np.abs(nw["u"]).max()


def test_the_backtracking_input():
    """the same problem with f = 2000 / N^2 at L = 5: Newton's step lengths are 1/16, 1/8, 1/2, then 1 (8 rejected trials);
    Picard stays at 1/16 for its first seven steps; with max_backtracks = 2 the first line search fails after three
    rejected trials and the iterate is the guess"""
    a, f, u0 = contrast_problem(5, 2000.0)
    nw = qr.quasi(a, K, f, u0, qr.dense_solve, 1e-10, 40, 8, method=qr.NEWTON)
    assert nw["converged"] and list(nw["lam"]) == [1 / 16, 1 / 8, 1 / 2, 1, 1, 1, 1] and nw["backtracks"] == 8
    pc = qr.quasi(a, K, f, u0, qr.dense_solve, 1e-10, 8, 8, method=qr.PICARD)
    assert list(pc["lam"][:7]) == [1 / 16] * 7 and not pc["failed"]
    for method in (qr.NEWTON, qr.PICARD):
        short = qr.quasi(a, K, f, u0, qr.dense_solve, 1e-10, 40, 2, method=method)
        assert short["failed"] and not short["converged"] and short["backtracks"] == 3 and len(short["hist"]) == 1
        assert np.array_equal(short["u"], u0)


def test_null_handles_are_refused_without_a_device(pkg):
    """NULL handle (with and without opt) from both entry points: MGX_ERR_INVALID, every output left alone"""
    lib = pkg.lib()
    B = pkg.binding
    opt = B.QuasiOpts(1.0, 0.0, 1.0, pkg.QUASI_NEWTON, pkg.TRANSFER_BILINEAR, pkg.STEP_SOLVE, 1e-8, 10, 4, 1e-10, 5, 4)
    a = np.ones(25)
    ns = B.NewtonStats(iterations=-7, converged=-7, history_len=-7)
    st = (B.Stats * 5)()
    for s in st:
        s.cycles = -7
    lam, hist = np.full(5, -1.0), np.full(6, -1.0)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    for o in (C.byref(opt), None):
        assert lib.mgx_quasi(None, o, a.ctypes.data, a.size, C.byref(ns), st, dp(lam), dp(hist), 6) == INVALID
    assert (ns.iterations, ns.converged, ns.history_len) == (-7, -7, -7)
    assert all(s.cycles == -7 for s in st) and (lam == -1.0).all() and (hist == -1.0).all()
    ms = C.c_double(-1.0)
    for step in (0, 1):
        for method in (pkg.QUASI_PICARD, pkg.QUASI_NEWTON):
            assert lib.mgx_time_quasi_pass(None, step, method, 1, C.byref(ms)) == INVALID and ms.value == -1.0


def test_the_options_struct_is_laid_out_as_the_header_says(pkg, tmp_path):
    """sizeof and the offsets of mgx_quasi_opts from the C compiler against the ctypes structure"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [name for name, _ in pkg.binding.QuasiOpts._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mgx.h"\nint main(void){printf("%zu", sizeof(mgx_quasi_opts));\n'
                   + "".join(f'printf(" %zu", offsetof(mgx_quasi_opts, {name}));\n' for name in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Q = pkg.binding.QuasiOpts
    assert got == [C.sizeof(Q)] + [getattr(Q, name).offset for name in fields]
