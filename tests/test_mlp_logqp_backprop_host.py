"""Host side of ``sdeint(..., logqp=True)`` on the KL perceptron kernels (no GPU): the new export, the planner's refusals, and
the oracle criterion's power to tell the step equations of ``tsde_trajectory_mlp_diag_logqp_backward`` from a wrong set."""
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers
from tests import helpers_logqp as L
from tests import helpers_logqp_backprop as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "tsde_trajectory_mlp_diag_logqp_backward"


def test_the_export_is_in_the_header_the_library_and_the_signatures():
    from torchsde_amd import _native
    text = open(os.path.join(ROOT, "include", "torchsde_amd.h")).read()
    declaration = re.search(r"int\s+" + SYMBOL + r"\s*\(([^;]*)\);", text)
    assert declaration, "not declared in include/torchsde_amd.h"
    arguments = [a.strip() for a in declaration.group(1).split(",")]
    for name in ("a_l", "grad_logqp", "b2", "prior_rate", "prior_shift", "row_prior_rate", "row_prior_shift", "bm_stride"):
        assert any(re.search(r"\b" + name + r"$", a) for a in arguments), name
    assert SYMBOL in _native.SIGNATURES and len(_native.SIGNATURES[SYMBOL][1]) == len(arguments)
    lib = _native.load()
    assert hasattr(lib, SYMBOL)
    assert lib.tsde_abi_version() == 2                   # an additive change


def _wrapped(module):
    from torchsde_amd.sde import ForwardSDE, SDELogqp
    return ForwardSDE(SDELogqp(module))


@pytest.mark.parametrize("what", ("adaptive", "extra", "extra_solver_state", "srk", "trajectory_kernel off", "hip_graph",
                                  "TSDE_RECOGNISE=0", "no solver", "stratonovich", "foreign brownian motion"))
def test_the_planner_declines_without_touching_the_gpu(what, monkeypatch):
    from torchsde_amd import mlp_adjoint, recognise
    case = L.Case(70, (16, 4, 16), P.SCHEMES[0], "tanh")
    module = case.module(sde_type="stratonovich" if what == "stratonovich" else "ito")
    monkeypatch.setattr(torch.Tensor, "cuda", lambda *a, **k: pytest.fail("the planner moved a tensor to the GPU"))
    monkeypatch.setattr(recognise, "recognise", lambda *a, **k: pytest.fail("the planner interpreted the module"))
    if what == "TSDE_RECOGNISE=0":
        monkeypatch.setattr(recognise, "ENABLED", False)
    y0 = torch.cat((case.y0(), torch.zeros(case.B, 1)), dim=1)
    ts = torch.tensor(case.ts())
    options = {"trajectory_kernel off": {"trajectory_kernel": False}, "hip_graph": {"hip_graph": True}}.get(what, {})

    class Solver:                                        # (what trust.open_book would ask of it is never reached)
        options = {}

    plan = mlp_adjoint.plan_logqp_sdeint(
        _wrapped(module), y0, ts, object(), "srk" if what == "srk" else "euler", P.DT, what == "adaptive", options,
        what == "extra", () if what == "extra_solver_state" else None, None if what == "no solver" else Solver())
    assert plan is None


def test_the_oracle_criterion_tells_the_step_equations_from_a_mutant():
    """The reverse step of include/torchsde_amd.h, written out in torch on the CPU in float32, meets `compare` against autograd
    through the oracle's solver; the same with the w term dropped from the cotangent of the W2 product does not."""
    case = L.Case(P.FIRST_INDEX + 1, (37, 20, 36), P.SCHEMES[0], "softplus")
    ref = P.oracle(case)
    assert ref["min_g"] >= L.MIN_DIFFUSION
    module = case.module()
    edges = helpers.rheun_grid(case.ts(), P.DT).t_f64()
    bm = helpers.counter_rows_bm(np.arange(case.B), case.d + 1, case.entropy, edges, P.F32)
    dW = torch.stack([bm(float(edges[k]), float(edges[k + 1]))[:, :case.d] for k in range(P.STEPS)])
    outcomes = {}
    for drop_w in (False, True):
        got = {}
        for label, wy, wl in case.cotangents():
            cot = L.column_cotangent(wy, wl)
            every = torch.zeros(P.STEPS + 1, case.B, case.d + 1)
            every[list(P.OUTPUTS)] = cot
            grad_y0, grads = P.reverse_sweep(module, case.y0(), dW, P.DT, every[:, :, :-1], every[:, :, -1], drop_w=drop_w)
            got[label] = dict(grads, y0=grad_y0)
        records, failures = P.compare(got, ref)
        outcomes[drop_w] = failures
        print("mutant" if drop_w else "step equations", "worst ratio", max(r[3] for r in records))
    assert not outcomes[False], "\n".join(outcomes[False])
    assert any("lin2.weight" in f for f in outcomes[True]) and any("log_ratio only" in f for f in outcomes[True])
    assert not any(f.startswith("ys only") for f in outcomes[True])        # (without a column cotangent w is 0)
