"""The single-GPU solver configuration bench.py builds from its flags, for the parity tests of the benchmarked rows
(tools/run_configs.py ROWS).  bench.py itself is not imported: it redirects fd 1 at import.  The defaults and the
construction mirror bench.py's parse() and run_single(); --steps / --warmup are accepted and ignored, any other flag
raises ValueError."""
import argparse
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f32": 0, "f64": 1, "mixed": 2}


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        raise ValueError(message)


def _parser():
    p = _Parser(add_help=False, allow_abbrev=False)
    p.add_argument("--level", type=int, default=13)            # one GPU: the metric grid
    p.add_argument("--coarsest", type=int, default=7)
    p.add_argument("--mu1", type=int, default=10)
    p.add_argument("--mu2", type=int, default=10)
    p.add_argument("--omega", type=float, default=2.0 / 3.0)
    p.add_argument("--smoother", choices=["jacobi", "rbgs"], default="jacobi")
    p.add_argument("--dtype", choices=["f64", "f32", "mixed"], default="f64")
    p.add_argument("--arith", choices=["fma", "separate"], default="fma")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    return p


def parse(flags):
    """the parsed flags of one row (a string or a list); ValueError on a flag bench.py's single-GPU run has not"""
    argv = flags.split() if isinstance(flags, str) else list(flags)
    args, extra = _parser().parse_known_args(argv)
    if extra:
        raise ValueError(f"unknown bench flags: {extra}")
    return args


def config(pkg, flags, arith=None):
    """mgx_config keywords of bench.py's timed handle (bench.py run_single); `arith` ("fma" / "separate") overrides
    the row's rounding mode"""
    a = parse(flags)
    ar = a.arith if arith is None else arith
    return dict(finest_level=a.level, coarsest_level=min(a.coarsest, a.level), mu0=0, mu1=a.mu1, mu2=a.mu2,
                omega=a.omega, smoother=1 if a.smoother == "rbgs" else 0, dtype=DT[a.dtype],
                schedule=pkg.SCHEDULE_V, profile=2, arith=pkg.ARITH_FMA if ar == "fma" else pkg.ARITH_SEPARATE)


def rows():
    """tools/run_configs.py ROWS: (name, flags) of every configuration whose numbers the project publishes"""
    path = os.path.join(ROOT, "tools", "run_configs.py")
    spec = importlib.util.spec_from_file_location("run_configs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.ROWS)
