"""bench.py's options: a plain run times exactly --steps steps and reports them, --dump-outputs writes what
those steps computed, --full adds the legs that take runs of their own.  The GPU cases start bench.py as a
child process at a small grid and redo its timed path in this process to check the dumped arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_KEYS = ("vcycles_to_1e-8", "ms_per_step_first_5_cycles_from_a_random_guess", "profiling_off",
             "roofline_single_sweep", "reference_problem_fmg")


def run_bench(*args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout)
    return r


def result_line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dump_outputs_is_refused_on_several_gpus(tmp_path):
    r = run_bench("--gpus", "2", "--dump-outputs", str(tmp_path / "out"), timeout=120)
    assert r.returncode == 2 and "--gpus 1 only" in r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("flags", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_checked(flags):
    r = run_bench(*flags, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_what_its_timed_steps_computed(pkg, tmp_path):
    level, steps, warmup = 10, 3, 1
    out = tmp_path / "out"
    d = result_line(run_bench("--level", str(level), "--steps", str(steps), "--warmup", str(warmup),
                              "--dump-outputs", str(out)))
    assert d["metric"] == "fine_grid_stencil_updates_per_sec" and d["unit"] == "updates/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0 and d["value"] > 0
    assert not any(k in d for k in FULL_KEYS + ("cpu_baseline",))
    hist = np.load(out / "residual_history.npy")
    u = np.load(out / "solution_sample.npy")
    assert hist.dtype == np.float64 and hist.shape == (steps + 1,)
    n = (1 << level) - 1
    assert u.dtype == np.float64 and u.shape == (n * n,)                 # n^2 <= 2^22: every point
    # the timed path of bench.py, redone here: same configuration, same device-generated inputs
    cfg = dict(finest_level=level, coarsest_level=7, mu0=0, mu1=10, mu2=10, omega=2.0 / 3.0, smoother=0,
               dtype=pkg.DTYPE_F64, schedule=pkg.SCHEDULE_V, profile=2, arith=pkg.ARITH_FMA)
    with pkg.Multigrid(**cfg) as mg:
        mg.fill_rhs(1, 0.0)
        mg.fill_guess_random(12345)
        mg.solve(tol=0.0, max_cycles=1)
        mg.fill_guess_random(12345)
        mg.solve(tol=0.0, max_cycles=warmup)
        _, h_ref = mg.solve(tol=0.0, max_cycles=steps)
        u_ref = mg.get_solution().reshape(-1)
    assert np.allclose(hist, h_ref, rtol=1e-12, atol=0)
    assert np.max(np.abs(u - u_ref)) <= 1e-12 * np.max(np.abs(u_ref))


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(pkg):
    d = result_line(run_bench("--full", "--no-cpu-baseline", "--level", "10", "--steps", "2", "--warmup", "1"))
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    for k in FULL_KEYS:
        assert k in d, k
        assert not (isinstance(d[k], dict) and "error" in d[k]), (k, d[k])
    assert "cpu_baseline" not in d
