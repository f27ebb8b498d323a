"""CPU check of k_tile_wide's tile map (csrc/mgx_geom.hpp tile_wide_geom), compiled with g++ into
tests/tile_wide_check.cpp: every output node covered exactly once, inside the valid region of its tile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigrid_nikhil_c-_amd", "csrc")


def test_wide_tiles_cover_every_node_exactly_once(tmp_path):
    exe = str(tmp_path / "tile_wide_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "tile_wide_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
