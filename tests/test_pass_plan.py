"""Pass planner (csrc/mgx_pass_plan.hpp) checked on the CPU: fold_plan, the one function that splits a smoothing block into
launches for whole levels and slabs, compiled with g++ into tests/pass_plan_check.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_nikhil_c-_amd", "csrc")

# the knob sets of the pinned table (its first column), as the GPU tests switch them
KNOB_SETS = [
    {},
    {"MGX_FUSE": "1"},
    {"MGX_FUSE": "2", "MGX_FUSE_MIN_N": "128"},
    {"MGX_TILE_MAX_N": "0"},
    {"MGX_PLAN_PRE": "8,2", "MGX_PLAN_POST": "6,4", "MGX_PLAN_MIN_N": "1024"},
    {"MGX_FOLD_KMAX": "5"},
    {"MGX_ROWS": "8"},
]


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "pass_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "pass_plan_check.cpp")], check=True)
    return exe


def _env(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MGX_")}
    return {**env, **knobs}


@pytest.mark.parametrize("set_id", range(len(KNOB_SETS)))
def test_plans_match_the_pinned_table(plan_check, set_id):
    r = subprocess.run([plan_check, "pinned", str(set_id)], env=_env(KNOB_SETS[set_id]), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.mark.parametrize("knobs", KNOB_SETS + [{"MGX_TILE_K": "4", "MGX_TILE_WIDE": "2"}, {"MGX_FUSE_ROWS": "24"}])
def test_fuzzed_plans_keep_the_invariants(plan_check, knobs):
    r = subprocess.run([plan_check, "fuzz", "20000"], env=_env(knobs), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
