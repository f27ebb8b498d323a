"""tests/bench_cfg.py turns tools/run_configs.py rows into bench.py's solver configuration (no GPU needed: the
package's constants are read without loading libmgx)."""
import pytest

import __graft_entry__ as ge
import bench_cfg


@pytest.fixture(scope="module")
def mgx():
    return ge.load_package()


def test_every_row_parses(mgx):
    rows = bench_cfg.rows()
    assert len(rows) >= 13
    for name, flags in rows:
        cfg = bench_cfg.config(mgx, flags)
        assert cfg["profile"] == 2 and cfg["mu0"] == 0 and cfg["schedule"] == mgx.SCHEDULE_V, name
        assert 2 <= cfg["coarsest_level"] <= cfg["finest_level"] <= 15, name


@pytest.mark.parametrize("flags", ["--gpus 2", "--level 12 --full", "--lev 12", "--smoother sor", "--dtype f16", "--mu1"])
def test_an_unknown_flag_raises(mgx, flags):
    with pytest.raises(ValueError):
        bench_cfg.config(mgx, flags)


def test_the_metric_grid_row_is_the_bench_default(mgx):
    # the configuration tests/test_bench_cli.py rebuilds for bench.py's timed path, at the metric grid
    expect = dict(finest_level=13, coarsest_level=7, mu0=0, mu1=10, mu2=10, omega=2.0 / 3.0, smoother=0,
                  dtype=mgx.DTYPE_F64, schedule=mgx.SCHEDULE_V, profile=2, arith=mgx.ARITH_FMA)
    flags = dict(bench_cfg.rows())["metric grid, the reference's V(10,10) (bench default)"]
    assert bench_cfg.config(mgx, flags) == expect
    assert bench_cfg.config(mgx, "") == expect
    # --steps / --warmup do not change the configuration; --arith and the override do
    assert bench_cfg.config(mgx, flags + " --steps 50 --warmup 5") == expect
    assert bench_cfg.config(mgx, flags + " --arith separate")["arith"] == mgx.ARITH_SEPARATE
    assert bench_cfg.config(mgx, flags, arith="separate")["arith"] == mgx.ARITH_SEPARATE


def test_rows_map_to_the_published_configurations(mgx):
    cfgs = {flags: bench_cfg.config(mgx, flags) for _, flags in bench_cfg.rows()}
    c = cfgs["--level 13 --dtype mixed --mu1 2 --mu2 1"]
    assert (c["dtype"], c["mu1"], c["mu2"], c["finest_level"]) == (mgx.DTYPE_MIXED, 2, 1, 13)
    c = cfgs["--level 14 --smoother rbgs --mu1 2 --mu2 1"]
    assert (c["smoother"], c["finest_level"], c["coarsest_level"]) == (mgx.SMOOTHER_RBGS, 14, 7)
    c = cfgs["--level 8 --coarsest 6 --mu1 10 --mu2 10"]
    assert (c["finest_level"], c["coarsest_level"]) == (8, 6)
