"""numpy statement of mgx_solve_refine_gcr (include/mgx.h): tests/gcr_ref.py's loop - restarted GCR with right
preconditioning in float64 - with M replaced by the scaled float32 cycle of tests/refine_ref.py:

    r = b - A x;  hist[0] = ||r||;  n = the side of the grid
    iteration k, j = k mod restart (the basis is emptied at j = 0):
      s_k = pow2_floor(hist[max(k - 1, 0)] / n)
      z = s_k * float64( M32( float32(r / s_k) ) );  q = A z
      h_i = (q.Q_i) / s_i, i < j;  q' = ((q - h_0 Q_0) - h_1 Q_1) - ..., z' likewise
      s_j = q'.q';  rho = r.q';  breakdown unless s_j > 0 and finite;  alpha = rho / s_j
      x += alpha z';  r -= alpha q';  hist[k + 1] = ||r||;  Z_j = z', Q_j = q'

Vectors, dots and scalars are float64; the scaling by a power of two is exact.  The operator and the cycle are callables:
the CPU tests give it tests/galerkin_ref.py's hierarchies, the GPU tests the public pieces of independent handles."""
import numpy as np

from pcg_ref import dot
from refine_ref import scale


def device_dot(a, b, rows_per_chunk=0):
    """a.b of two fp64 fine-level vectors (interior points, n x n) summed in the order of the device's Krylov passes
    (csrc/mgx_krylov.hpp, csrc/mgx_kernels.hpp: make_launch, wave_tile, lane_cols<2>, block_reduce, pcg_reduce_sum), every
    product and sum rounded on its own:
      a lane holds the columns (2 v, 2 v + 1) of its vector v (column 0 is the ring: zero) and adds p.x q.x + p.y q.y row by
      row down the R rows of its chunk; 62 storing lanes (1 .. 62 of 64) per wave, one wave per (chunk, strip), strips
      fastest; a wave is summed by shuffles (32, 16, .. 1), the four waves of a workgroup in order from zero; workgroup i
      works on the tiles of block xcd * per_xcd + (nth or per_xcd - 1 - nth) (xcd = i & 7, nth = i >> 3, backwards on the
      upper four); the per-workgroup sums are added by 1024 threads with four strided accumulators each, the threads by
      shuffles per wave, the sixteen waves in order.
    With this dot tests/test_gpu_refine_gcr.py's reference performs the device's operations in the device's order."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n = a.shape[0]
    N = n + 1
    strips = max(1, (N // 2 + 61) // 62)
    R = rows_per_chunk if rows_per_chunk > 0 else min(8, max(4, n // 128))
    chunks = max(1, (n + R - 1) // R)
    blocks = ((strips * chunks + 3) // 4 + 7) // 8 * 8
    fa = np.zeros((chunks * R, strips * 124))
    fb = np.zeros_like(fa)
    fa[:n, 1:N] = a
    fb[:n, 1:N] = b
    pair = fa[:, 0::2] * fb[:, 0::2] + fa[:, 1::2] * fb[:, 1::2]          # (rows, vectors)
    pair = pair.reshape(chunks, R, strips, 62)
    lanes = np.zeros((chunks, strips, 64))
    for t in range(R):                                                    # (rows past the grid add zeros: exact)
        lanes[:, :, 1:63] = lanes[:, :, 1:63] + pair[:, t]
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes[..., :off] + lanes[..., off:2 * off]
    waves = np.zeros(blocks * 4)
    waves[:chunks * strips] = lanes.reshape(-1)
    waves = waves.reshape(blocks, 4)
    bsum = np.zeros(blocks)
    for w in range(4):
        bsum = bsum + waves[:, w]
    i = np.arange(blocks)
    per_xcd, xcd, nth = blocks >> 3, i & 7, i >> 3
    part = bsum[xcd * per_xcd + np.where(xcd >= 4, per_xcd - 1 - nth, nth)]
    T = 1024
    acc = np.zeros((4, T))
    at = np.arange(T)
    while True:
        m = at + 3 * T < blocks
        if not m.any():
            break
        for q in range(4):
            acc[q, m] = acc[q, m] + part[at[m] + q * T]
        at[m] += 4 * T
    while True:
        m = at < blocks
        if not m.any():
            break
        acc[0, m] = acc[0, m] + part[at[m]]
        at[m] += T
    v = ((acc[0] + acc[1]) + (acc[2] + acc[3])).reshape(16, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:, :off] + v[:, off:2 * off]
    s = 0.0
    for w in range(16):
        s = s + v[w, 0]
    return float(s)


def refine_gcr(A, cycle, b, x0, tol=1e-8, max_iters=100, restart=4, history=None, dot=dot):
    """A: callable u -> A u (float64);  cycle(r32) -> float32 array, the correction of one cycle from zero for the float32
    right-hand side r32;  dot: the inner product (float64 result).  history = None: the scales come from this loop's own
    norms; history given (a device's reported history): s_k is derived from IT wherever the entry exists, as a device
    that reported it has used them - the loop still stops by its own norms and max_iters.
    Returns (x, history, converged, breakdown)."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64, order="C")
    n = b.shape[0]
    r = b - A(x)
    h0 = np.sqrt(dot(r, r))
    hist = [h0]
    if h0 <= tol * h0 or max_iters == 0:
        return x, np.array(hist), h0 <= tol * h0, False
    given = None if history is None else [float(v) for v in history]
    Z, Q, S = [], [], []
    for k in range(max_iters):
        j = k % restart
        if j == 0:
            Z, Q, S = [], [], []
        src = given if given is not None and max(k - 1, 0) < len(given) else hist
        s = scale(src, k, n)
        e = np.asarray(cycle((r * (1.0 / s)).astype(np.float32)))
        assert e.dtype == np.float32
        z = s * e.astype(np.float64)
        q = A(z)
        h = [dot(q, Q[i]) / S[i] for i in range(j)]
        for i in range(j):
            q = q - h[i] * Q[i]
            z = z - h[i] * Z[i]
        sj = dot(q, q)
        rho = dot(r, q)
        if not (sj > 0) or not np.isfinite(sj):
            return x, np.array(hist), False, True
        alpha = rho / sj
        x = x + alpha * z
        r = r - alpha * q
        rn = np.sqrt(dot(r, r))
        hist.append(rn)
        Z.append(z), Q.append(q), S.append(sj)
        if rn <= tol * h0:
            return x, np.array(hist), True, False
    return x, np.array(hist), False, False
