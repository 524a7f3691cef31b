"""Host side of Milstein on the neural-SDE kernel (`tsde_trajectory_mlp_general`, diagonal and scalar noise): the method codes
of the C ABI, which code a `_Milstein` solver asks the kernel for, and the benchmark workloads. (No GPU: the kernel itself is
tests/test_gpu_neural_milstein.py.)"""
import importlib
import os
import re
import sys

import pytest

from workloads import configs, problems
from torchsde_amd import _native, solvers
from torchsde_amd.brownian import BrownianInterval
from torchsde_amd.sde import ForwardSDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_method_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "torchsde_amd.h")).read()
    header = {name: int(value) for name, value in re.findall(r"#define TSDE_(TRAJ_[A-Z_]+) (\d+)", text)}
    for name in ("TRAJ_EULER", "TRAJ_MILSTEIN_ITO", "TRAJ_MILSTEIN_STRAT", "TRAJ_MIDPOINT", "TRAJ_SRK", "TRAJ_HEUN",
                 "TRAJ_EULER_HEUN", "TRAJ_REVERSIBLE_HEUN", "TRAJ_MILSTEIN_ITO_GF", "TRAJ_MILSTEIN_STRAT_GF"):
        assert getattr(_native, name) == header[name], name
    assert (header["TRAJ_MILSTEIN_ITO_GF"], header["TRAJ_MILSTEIN_STRAT_GF"]) == (8, 9)
    codes = [v for k, v in header.items() if k != "TRAJ_SENS"]
    assert len(set(codes)) == len(codes)


OPT_IN = {"neural_milstein_kernel": True}      # (the route is off by default: its timings are not on file)


def _solver(problem, sde_type, grad_free, options=OPT_IN, **kw):
    sde = ForwardSDE(problems.make(f"{problem}_{'ito' if sde_type == 'ito' else 'strat'}", **kw))
    m = {"netdiag": 4, "netscalar": 1}.get(problem, kw.get("m", 3))
    bm = BrownianInterval(0.0, 1.0, size=(3, m))
    cls = solvers.select("milstein", sde_type)
    return cls(sde=sde, options=dict(options or {}, grad_free=grad_free), bm=bm, dt=0.1, adaptive=False, rtol=1e-5, atol=1e-4,
               dt_min=1e-5)


@pytest.mark.parametrize("problem", ["netdiag", "netscalar"])
@pytest.mark.parametrize("sde_type,grad_free,want", [
    ("ito", False, "TRAJ_MILSTEIN_ITO"), ("stratonovich", False, "TRAJ_MILSTEIN_STRAT"),
    ("ito", True, "TRAJ_MILSTEIN_ITO_GF"), ("stratonovich", True, "TRAJ_MILSTEIN_STRAT_GF")])
def test_neural_code_of_milstein(problem, sde_type, grad_free, want):
    solver = _solver(problem, sde_type, grad_free)
    assert solver._neural_code() == getattr(_native, want)
    assert solver._deep_code() is None                  # (deeper nets, LipSwish, a closing tanh: stepwise under Milstein)
    assert solver.stage_fracs == solvers.Euler.stage_fracs      # one stage time, t_k, like Euler
    assert _solver(problem, sde_type, grad_free, options=None)._neural_code() is None        # (off by default)


@pytest.mark.parametrize("sde_type", ["ito", "stratonovich"])
@pytest.mark.parametrize("grad_free", [False, True])
def test_general_noise_milstein_has_no_neural_code(sde_type, grad_free):
    """(Holds before the feature too -- the base class answers None: a guard that the opt-in general-noise Milstein is not
    routed to a kernel that has no such scheme; beside it, the same solver class does answer for diagonal noise.)"""
    solver = _solver("general", sde_type, grad_free, options=dict(OPT_IN, general_noise=True))
    assert solver._neural_code() is None
    assert type(solver) is type(_solver("netdiag", sde_type, grad_free)) and _solver("netdiag", sde_type, grad_free)._neural_code()


def test_the_workloads():
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    pairs = {"c2_milstein_netdiag_default_route_b65536_d64_s1000": "c2_milstein_netdiag_b65536_d64_s1000",
             "c2_milstein_gradfree_netdiag_default_route_b65536_d64_s1000": "c2_milstein_gradfree_netdiag_b65536_d64_s1000"}
    for route, twin in pairs.items():
        assert route in bench.WORKLOADS and twin in bench.WORKLOADS
        assert route not in bench.ALSO and twin not in bench.ALSO
        r, t = configs.WORKLOADS[route], configs.WORKLOADS[twin]
        assert r["stepwise"] == twin and r["recognised"] and r["trajectory"] and not t.get("trajectory")
        assert r["mfma_flops_per_traj_step"] == 6 * 2 * 64 * 64
        same = ("problem", "method", "levy", "B", "d", "m", "nsteps", "dt")
        assert [r[k] for k in same] == [t[k] for k in same] == ["netdiag_big", "milstein", "none", 65536, 64, 64, 1000, 2.0 ** -10]
        form = {"grad_free": True} if "gradfree" in route else {}
        assert (t.get("options") or {}) == form and r["options"] == dict(form, **OPT_IN)
