"""numpy statement of mgx_solve_refine (include/mgx.h): fp64 defect correction around an fp32 cycle,

    u += s_k * M32( (b - A u) / s_k ),   s_k = pow2_floor( hist[max(k - 1, 0)] / n ),   n = 2^finest_level - 1,

with the residual and the iterate in float64, M32 one cycle from zero in float32 and every s_k a power of two, so
that the scaling is exact.  The operator and the cycle are callables: the CPU tests give it tests/galerkin_ref.py's
hierarchies, the GPU tests the public pieces of independent handles."""
import math

import numpy as np


def pow2_floor(x):
    """the largest power of two <= x (x > 0 and finite): pow2_floor() of csrc/mgx.hip"""
    _, e = math.frexp(x)
    return math.ldexp(1.0, e - 1)


def scale(hist, k, n):
    """s_k, the scale of the residual that cycle k is given and of the correction it returns"""
    return pow2_floor(hist[max(k - 1, 0)] / n)


def norm2(r):
    return float(np.sqrt(np.sum(np.asarray(r, dtype=np.float64) ** 2)))


def refine(residual, cycle, b, u0, tol=0.0, max_cycles=50, history=None, norm=norm2, scales=None):
    """(u, history of ||b - A u||).  residual(u, b) -> float64 array; cycle(r32) -> float32 array, the correction of one
    cycle from zero for the float32 right-hand side r32.  history = None: the scales come from this loop's own norms
    and it stops at hist[k] <= tol * hist[0] or after max_cycles cycles; history given (len = cycles + 1): that many
    cycles with the scales derived from IT, as a device that reported it has used them.  scales (a history, with
    history = None): the loop stops by its own norms, and s_k is derived from scales[max(k - 1, 0)] where that entry
    exists, from its own history where it does not."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    u = np.array(u0, dtype=np.float64, order="C")
    n = b.shape[0]
    r = residual(u, b)
    hist = [norm(r)]
    given = None if history is None else [float(x) for x in history]
    cycles = max_cycles if given is None else len(given) - 1
    for k in range(cycles):
        if given is None and hist[k] <= tol * hist[0]:
            break
        src = hist if given is None else given
        if given is None and scales is not None and max(k - 1, 0) < len(scales):
            src = scales
        s = scale(src, k, n)
        r32 = (r / s).astype(np.float32)
        e = np.asarray(cycle(r32))
        assert e.dtype == np.float32
        u = u + s * e.astype(np.float64)
        r = residual(u, b)
        hist.append(norm(r))
    return u, np.array(hist)
