"""The perceptron training kernels held to float32 rounding (run with ``-m gpu``): autograd through ``sdeint``
(``_MlpTrajectoryFn``: tsde_trajectory_mlp_diag_backward + tsde_gram_partials, and the chunk and re-run logic of
torchsde_amd/kernels.py) and ``sdeint_adjoint`` (``_MlpAdjointFn``: tsde_adjoint_mlp_diag, torchsde_amd/mlp_adjoint.py) on
``MLPDriftDiagonalSDE``, over the case table of tests/helpers.py (`mlp_grad_cases`: shapes at the edges of the tiles, a random
start, outputs on the first step, on consecutive boundaries, inside and at the end, a cotangent on all outputs and on single
ones).

Reference: the CPU oracle in float64 on the same counter path (`helpers.mlp_grad_oracle`). Criterion: the kernels may differ
from it by `MLP_GRAD_FACTOR` times what the oracle's own float32 run differs from it, plus `MLP_GRAD_FLOOR` of the quantity's
scale (`helpers.assert_within_reference_rounding`) -- for the outputs, dL/dy0 and each of the six parameter gradients, whole and
on the ragged last tiles on their own. tests/test_mlp_gradient_criterion.py shows on the CPU what this criterion rejects that
``2e-3 * max + 1e-6`` accepts. The factor is measured (tools/mlp_gradient_rounding_ratios.py ->
profiles/mlp_gradient_rounding_ratios.txt), never against the kernels' own earlier output."""
import functools

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
CASES = helpers.mlp_grad_cases()
SCALAR_CASES = helpers.mlp_grad_scalar_cases()
ALL_CASES = CASES + SCALAR_CASES
# the shapes that also run chunked, recomputed and without a gradient for y0
SMALL = [i for i, case in enumerate(CASES) if (case.B, case.d, case.hidden) in ((37, 20, 36), (129, 4, 16))]
GRADIENTS = helpers.MLP_GRAD_QUANTITIES[1:]


@functools.lru_cache(maxsize=None)
def _oracle(index):
    """Computed once per case, shared by every test of that case, never written to."""
    return helpers.mlp_grad_oracle(ALL_CASES[index])


def solve(case, y0_grad=True):
    """One solve of `case` on the kernels and one backward pass per cotangent: {label: {quantity: tensor}}."""
    import torchsde_amd
    dt, steps = helpers.MLP_GRAD_DT, helpers.MLP_GRAD_STEPS
    sde = case.module().to(DEV)
    y0 = case.y0().to(DEV).requires_grad_(y0_grad)
    ts = torch.tensor(case.ts(), device=DEV)
    bm = torchsde_amd.BrownianInterval(0.0, steps * dt, size=(case.B, case.d), dtype=F32, device=DEV, entropy=case.entropy,
                                       dt=dt, levy_area_approximation="space-time" if case.levy else "none")
    if case.route == "backprop":
        ys = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=case.method, dt=dt)
        assert type(ys.grad_fn).__name__.startswith("_MlpTrajectoryFn"), type(ys.grad_fn).__name__
    else:
        ys = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method=case.method, adjoint_method=case.adjoint_method, dt=dt)
        assert type(ys.grad_fn).__name__.startswith("_MlpAdjointFn"), type(ys.grad_fn).__name__
    names, params = zip(*sde.named_parameters())
    inputs = ([y0] if y0_grad else []) + list(params)
    out = {}
    for label, w in case.cotangents():
        grads = torch.autograd.grad(ys, inputs, grad_outputs=w.to(DEV), retain_graph=True)
        out[label] = dict(zip((["y0"] if y0_grad else []) + list(names), (g.detach().clone() for g in grads)))
        out[label]["ys"] = ys.detach()
    return out


def compare(case, got, ref):
    """Every quantity of `got` (and its ragged tiles) against the oracle: [(label, quantity, err_new, err_ref, ratio)] with
    ratio = (err_new - floor * scale) / err_ref -- the factor that quantity needs -- and the list of those the criterion
    refuses."""
    records, failures = [], []
    floor = helpers.MLP_GRAD_FLOOR
    for label, quantities in got.items():
        for name in helpers.MLP_GRAD_QUANTITIES:
            if name not in quantities:
                continue
            views = {"": ()}
            views.update(helpers.mlp_grad_ragged_slices(case, name))
            for where, index in views.items():
                new = quantities[name][index].double().cpu()
                r32, r64 = ref[F32][label][name][index].double(), ref[F64][label][name][index]
                assert new.shape == r64.shape and new.numel() > 0, (name, where, new.shape, r64.shape)
                scale = max(1.0, r64.abs().max().item())
                err_new, err_ref = (new - r64).abs().max().item(), (r32 - r64).abs().max().item()
                excess = err_new - floor * scale
                ratio = 0.0 if excess <= 0.0 else (excess / err_ref if err_ref > 0.0 else float("inf"))
                what = f"{label:6s} {name}{' [' + where + ']' if where else ''}"
                records.append((what, err_new, err_ref, ratio))
                try:
                    helpers.assert_within_reference_rounding(new, r32, r64, what, factor=helpers.MLP_GRAD_FACTOR, floor=floor)
                except AssertionError as e:
                    failures.append(str(e))
    return records, failures


def hold(case, got, ref, variant=""):
    records, failures = compare(case, got, ref)
    for what, err_new, err_ref, ratio in records:
        print(f"{case.id} {variant} {what}: err {err_new:.3e} ref {err_ref:.3e} ratio {ratio:.2f}")
    assert not failures, "\n".join(failures)


def _degenerate(case, got):
    """A cotangent on ys[0] alone: dL/dy0 is that cotangent bit for bit, no parameter is reached."""
    w = dict(case.cotangents())["first"][0]
    assert torch.equal(got["first"]["y0"].cpu(), w)
    for name in GRADIENTS[1:]:
        assert got["first"][name].abs().max().item() == 0.0, name


@pytest.mark.parametrize("index", range(len(CASES)), ids=[case.id for case in CASES])
def test_outputs_and_gradients_are_the_float64_oracles_to_float32_rounding(index):
    case = CASES[index]
    got = solve(case)
    assert set(got["all"]) == set(helpers.MLP_GRAD_QUANTITIES)
    hold(case, got, _oracle(index))
    _degenerate(case, got)


def _budgets(monkeypatch, case, steps_per_chunk=5, recompute=False):
    from torchsde_amd import kernels as K, mlp_adjoint
    B, d, hidden = case.B, case.d, case.hidden
    monkeypatch.setattr(K._MlpTrajectoryFn, "STASH_BYTES", steps_per_chunk * B * (d + 2 * hidden) * 4)
    monkeypatch.setattr(mlp_adjoint._MlpAdjointFn, "STASH_BYTES", steps_per_chunk * B * (2 * d + 2 * hidden) * 4)
    if recompute:
        monkeypatch.setattr(K._MlpTrajectoryFn, "STATE_BYTES", 1)


@pytest.mark.parametrize("index", SMALL, ids=[CASES[i].id for i in SMALL])
def test_a_stash_budget_of_five_steps_changes_no_state_gradient_and_stays_within_rounding(index, monkeypatch):
    """Five steps per chunk of sixteen: the outputs at steps 1 and 2 sit in the chunk processed last, step 9 inside a chunk,
    step 16 on a chunk edge. With no room for the states either, the backward pass of `sdeint` re-runs the sampling kernel
    per chunk."""
    case = CASES[index]
    whole = solve(case)
    variants = [("chunked", False)] + ([("recomputed", True)] if case.route == "backprop" else [])
    for variant, recompute in variants:
        with monkeypatch.context() as m:
            _budgets(m, case, recompute=recompute)
            got = solve(case)
        for label in whole:
            assert torch.equal(got[label]["ys"], whole[label]["ys"]), (variant, label)
            assert torch.equal(got[label]["y0"], whole[label]["y0"]), (variant, label)
        hold(case, got, _oracle(index), variant)
        _degenerate(case, got)


@pytest.mark.parametrize("index", SMALL, ids=[CASES[i].id for i in SMALL])
def test_a_start_without_a_gradient_leaves_the_parameter_gradients_unchanged(index):
    case = CASES[index]
    with_y0, without = solve(case), solve(case, y0_grad=False)
    for label in with_y0:
        assert "y0" not in without[label]
        for name in GRADIENTS[1:]:
            assert torch.equal(without[label][name], with_y0[label][name]), (label, name)
    # (and through `backward()`, as a training loop calls it: y0.grad stays None)
    import torchsde_amd
    sde = case.module().to(DEV)
    y0 = case.y0().to(DEV)
    bm = torchsde_amd.BrownianInterval(0.0, 16 * helpers.MLP_GRAD_DT, size=(case.B, case.d), dtype=F32, device=DEV,
                                       entropy=case.entropy, dt=helpers.MLP_GRAD_DT,
                                       levy_area_approximation="space-time" if case.levy else "none")
    ts = torch.tensor(case.ts(), device=DEV)
    if case.route == "backprop":
        ys = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=case.method, dt=helpers.MLP_GRAD_DT)
    else:
        ys = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method=case.method, adjoint_method=case.adjoint_method,
                                         dt=helpers.MLP_GRAD_DT)
    assert type(ys.grad_fn).__name__.startswith(("_MlpTrajectoryFn", "_MlpAdjointFn"))
    (ys * case.cotangents()[0][1].to(DEV)).sum().backward()
    assert y0.grad is None
    for name, p in sde.named_parameters():
        assert torch.equal(p.grad, with_y0["all"][name]), name


@pytest.mark.parametrize("k", range(len(SCALAR_CASES)), ids=[case.id for case in SCALAR_CASES])
def test_scalar_diffusion_parameters_receive_the_oracles_sums(k):
    case = SCALAR_CASES[k]
    got = solve(case)
    for label in got:
        assert got[label]["diff_rate"].shape == got[label]["diff_shift"].shape == ()
    hold(case, got, _oracle(len(CASES) + k))
    _degenerate(case, got)
