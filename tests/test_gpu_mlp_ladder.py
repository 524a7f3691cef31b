"""Every rung of the launch ladder of the perceptron-drift kernels (csrc/tsde_launch.h: `mlp_ladder`; run with ``-m gpu``).

The ladder picks the tile sizes D in {32, 64, 128} and H in {32, 64, 128, 256} (H = 256 for D <= 64 only) that hold (d, hidden),
the activation, and the unpadded (FULL) instantiation where d == D and hidden == H; a wrong rung would pick a tile smaller than
the problem. The widths below sit on, just under and just over every tile edge, so that each (D, H) tile is taken padded and
FULL, with both activations. A rung that tests/test_gpu_mlp_trajectory.py, test_gpu_mlp_backward.py AND test_gpu_mlp_adjoint.py
already reach (sampling, training sweep and stochastic adjoint alike) is left out.

Per case: the sampling kernel's values and the training gradients (``sdeint`` under autograd: the forward pass IS the sampling
kernel) and the gradients of ``sdeint_adjoint``, each against the stepwise route of the same call, at the tolerances of
tests/test_gpu_mlp_backward.py. One case for ``logqp=True`` (the KL instantiations) at the tolerances of
tests/test_gpu_mlp_logqp_adjoint.py."""
import pytest
import torch

from tests import helpers_logqp as L
from tests.test_gpu_mlp_backward import _assert_gradients_close, _gradients, _sde

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, DT = 24, 2.0 ** -5                         # one full group of 16 rows and a partial one of 8
WIDTHS_D = (8, 32, 36, 64, 68, 128)
WIDTHS_H = (8, 32, 36, 64, 68, 128, 132, 256)


def _rung(d, hidden, activation):
    D = next(t for t in (32, 64, 128) if d <= t)
    H = next(t for t in (32, 64, 128, 256) if hidden <= t)
    return D, H, activation, d == D and hidden == H


# (D, H, activation, FULL) that all three existing suites reach: see their parametrisations
_REACHED = {(32, 32, "tanh", True), (64, 64, "softplus", True), (128, 128, "tanh", True), (128, 128, "softplus", True),
            (64, 256, "softplus", True), (32, 64, "tanh", False)}
CASES = [(d, hidden, activation) for d in WIDTHS_D for hidden in WIDTHS_H for activation in ("tanh", "softplus")
         if not (hidden > 128 and d > 64) and _rung(d, hidden, activation) not in _REACHED]


def test_the_cases_take_every_rung():
    rungs = {_rung(*case) for case in CASES} | _REACHED
    tiles = [(D, H) for D in (32, 64, 128) for H in (32, 64, 128, 256) if not (H == 256 and D == 128)]
    assert rungs == {(D, H, act, full) for D, H in tiles for act in ("tanh", "softplus") for full in (True, False)}


def _adjoint_gradients(sde, y0, ts, entropy, fast, weights):
    import torchsde_amd
    y = y0.clone().requires_grad_(True)
    bm = torchsde_amd.BrownianInterval(float(ts[0]), float(ts[-1]), size=tuple(y0.shape), dtype=y0.dtype, device=DEV,
                                       entropy=entropy)
    sde.zero_grad()
    ys = torchsde_amd.sdeint_adjoint(sde, y, ts, bm=bm, method="euler", adjoint_method="euler", dt=DT,
                                     adjoint_options={"trajectory_kernel": fast})
    assert type(ys.grad_fn).__name__.startswith("_MlpAdjointFn") == fast
    (ys * weights).sum().backward()
    named = {name: p.grad.clone() for name, p in sde.named_parameters()}
    named["y0"] = y.grad.clone()
    return ys.detach(), named


@pytest.mark.parametrize("d,hidden,activation", CASES)
def test_values_and_gradients_match_the_stepwise_route(d, hidden, activation):
    sde = _sde(d, hidden, activation)
    gen = torch.Generator().manual_seed(7)
    y0 = (0.5 * torch.randn(B, d, generator=gen)).to(DEV)
    ts = torch.tensor([0.0, DT, 3 * DT], device=DEV)         # 3 Euler steps, outputs on boundaries 1 and 3
    weights = torch.randn(3, B, d, generator=gen).to(DEV)
    ys_fast, fast = _gradients(sde, y0, ts, DT, 5, True, weights)
    ys_ref, ref = _gradients(sde, y0, ts, DT, 5, False, weights)
    torch.testing.assert_close(ys_fast, ys_ref, rtol=2e-4, atol=2e-5)
    _assert_gradients_close(fast, ref)
    ys_adj, adj = _adjoint_gradients(sde, y0, ts, 5, True, weights)
    ys_step, step = _adjoint_gradients(sde, y0, ts, 5, False, weights)
    torch.testing.assert_close(ys_adj, ys_step, rtol=2e-4, atol=2e-5)
    _assert_gradients_close(adj, step)


def test_logqp_on_a_padded_rung():
    """36 x 68: the padded (64, 128) tile of the two KL instantiations."""
    case = L.Case(70, (B, 36, 68), L.SCHEMES[0], "softplus")
    fast = L.solve(case, DEV, expect_route=True)
    stepwise = L.solve(case, DEV, fast=False, expect_route=False)
    for label in fast:
        for name, want in stepwise[label].items():
            got = fast[label][name]
            err, scale = (got.double() - want.double()).abs().max().item(), want.abs().max().item()
            tol = 5e-4 if name in ("ys", "log_ratio") else 2e-3
            assert err <= tol * scale + 1e-7, f"{label} {name}: max error {err:.3e} vs scale {scale:.3e}"
