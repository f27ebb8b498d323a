"""include/mgx_reference_api.hpp on the device: host/ref_api_check calls every function of the drop-in header once,
with the reference's names and std::vector signatures, and writes what each returned.  The float vectors must be
the oracle's bit for bit (the interpolation: the reference's own recorded output, tests/golden/ref_ps.npz), and
the conventions the header documents must hold: jacobirelaxation mutates v and returns it (PS:146),
vcyclemultigrid clobbers vec_h (PS:581), levels are inferred from vector lengths (PS:583), a wrong a_size throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_solve import hist_close

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = dict(finest_level=8, coarsest_level=6, mu0=1, mu1=3, mu2=2)
N8, N7, N6 = 255, 127, 63


@pytest.fixture(scope="module")
def run(pkg, po, tmp_path_factory):
    """the inputs, and everything the program wrote, from ONE run of it"""
    exe = os.path.join(ROOT, "multigrid_nikhil_c-_amd", "host", "ref_api_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True)
    rng = np.random.default_rng(808)
    inp = {
        "v8": rng.uniform(-1, 1, (N8, N8)).astype(np.float32),
        "f8": rng.uniform(-1, 1, (N8, N8)).astype(np.float32),
        "u8": po.fill_uniform((N8, N8), 808).astype(np.float32),
        "b8": po.rhs_sine(8).astype(np.float32),
        "e6": np.load(os.path.join(GOLD, "ref_ps.npz"))["interp_in_63"].astype(np.float32),
    }
    din, dout = tmp_path_factory.mktemp("ref_api_in"), tmp_path_factory.mktemp("ref_api_out")
    for name, a in inp.items():
        a.astype("<f4").tofile(str(din / name))
    r = subprocess.run([exe, str(din), str(dout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {}
    for name, n in (("jacobi_ret", N8), ("jacobi_v", N8), ("restrict", N7), ("interp", N7), ("vcycle_ret", N8),
                    ("vcycle_vec_h", N8), ("fmg", N8), ("force", N8), ("solve_u", N8)):
        a = np.fromfile(str(dout / name), dtype="<f4")
        assert a.size == n * n, (name, a.size)
        out[name] = a.reshape(n, n).astype(np.float32)
    out["fmg_f64"] = np.fromfile(str(dout / "fmg_f64"), dtype="<f8").reshape(N8, N8)
    out["solve_hist"] = np.fromfile(str(dout / "solve_hist"), dtype="<f8")
    out["status"] = (dout / "status.txt").read_text().splitlines()
    for a in inp.values():
        a.setflags(write=False)
    return inp, out


@pytest.fixture(scope="module")
def ref32(po):
    return po.Solver(**CFG, dtype=po.DTYPE_F32, schedule=po.SCHEDULE_FMG, bottom=po.BOTTOM_DST)


def test_hierarchy_entries_cycle_count_and_the_a_size_check(run):
    _, out = run
    assert out["status"] == ["entries 3", f"size {N6 * N6} level 6", f"size {N7 * N7} level 7", f"size {N8 * N8} level 8",
                             "cycles 3", "wrong a_size: caught", "double entries 3"]


def test_jacobirelaxation_returns_the_oracle_bits_and_mutates_v(run, po):
    inp, out = run
    assert np.array_equal(out["jacobi_ret"], po.jacobi(inp["v8"], inp["f8"], 3))
    assert not np.array_equal(out["jacobi_ret"], inp["v8"])
    assert np.array_equal(out["jacobi_v"], out["jacobi_ret"])                       # PS:146


def test_transfers_infer_their_level_from_the_vector_length(run, po):
    inp, out = run
    assert np.array_equal(out["restrict"], po.restrict(inp["f8"]))                  # PS:531: 255^2 -> 127^2
    # the reference's own interpolation2d output (PS:337) for this input
    want = np.load(os.path.join(GOLD, "ref_ps.npz"))["interp_out_63"]
    assert want.dtype == np.float32 and np.any(want != 0)
    assert np.array_equal(out["interp"], want)


def test_vcyclemultigrid_and_fullmultigrid_return_the_oracle_bits(run, ref32):
    inp, out = run
    v_ref = ref32.vcycle(8, inp["u8"], inp["b8"])
    assert v_ref.dtype == np.float32 and np.any(v_ref != 0)
    assert np.array_equal(out["vcycle_ret"], v_ref)
    assert np.array_equal(out["vcycle_vec_h"], out["vcycle_ret"])                   # PS:581: vec_h is clobbered
    assert not np.array_equal(out["vcycle_vec_h"], inp["u8"])
    w_ref = ref32.fmg(8, inp["b8"])
    assert w_ref.dtype == np.float32 and np.any(w_ref != 0)
    assert np.array_equal(out["fmg"], w_ref)


def test_globalforcefunction_is_the_reference_load_vector_with_the_spd_sign(run):
    _, out = run
    want = np.load(os.path.join(GOLD, "ref_ps.npz"))["force_L8"]                     # PS:283-335, recorded
    assert want.dtype == np.float32 and np.all(want < 0)
    assert np.array_equal(out["force"], -want)                                      # D1


def test_multigrid_solver_returns_the_oracle_solve(run, ref32):
    inp, out = run
    u_ref, h_ref = ref32.solve(inp["b8"], None, tol=0.0, max_cycles=3)
    assert len(out["solve_hist"]) == len(h_ref) == 4
    assert hist_close(out["solve_hist"], h_ref), (out["solve_hist"], h_ref)
    assert np.array_equal(out["solve_u"].astype(np.float64), u_ref)


def test_the_double_instantiation_tracks_the_fp64_oracle(run, po):
    inp, out = run
    w_ref = po.Solver(**CFG, dtype=po.DTYPE_F64).fmg(8, inp["b8"].astype(np.float64))
    assert np.max(np.abs(out["fmg_f64"] - w_ref)) <= 1e-12 * np.max(np.abs(out["fmg_f64"]))
