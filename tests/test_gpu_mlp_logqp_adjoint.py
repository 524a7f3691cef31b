"""``sdeint_adjoint(..., logqp=True)`` on the KL instantiations of the perceptron kernels (run with ``-m gpu``;
torchsde_amd/mlp_adjoint.py: plan_logqp, _MlpLogqpAdjointFn; csrc: tsde_trajectory_mlp_diag_logqp, tsde_adjoint_mlp_diag_logqp)
for an unchanged user module with a per-channel affine prior drift, against

(a) this package's stepwise stochastic adjoint of the same call (``adjoint_options={"trajectory_kernel": False}``), at the
    tolerances of tests/test_gpu_mlp_adjoint.py: 5e-4 of scale for values, 2e-3 for gradients;
(b) the oracle's restatement of the reference (`SDELogqp` under the stochastic adjoint) in float32 and float64 on the same
    counter path, through `helpers.assert_within_reference_rounding` with the measured factor of tests/helpers_logqp.py.

Cases, modules and the reference: tests/helpers_logqp.py. The KL column's row sum is an f32 sum in the kernel's own order, so
nothing here is bit-equal to the stepwise route; chunks and shards of the route itself are."""
import copy
import functools

import pytest
import torch

from tests import helpers_logqp as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = L.cases()
FN = "_MlpLogqpAdjointFn"


@functools.lru_cache(maxsize=None)
def _oracle(index):
    """Computed once per case, shared, never written to."""
    return L.oracle(CASES[index])


def _close(got, want, what, tol):
    err = (got.double().cpu() - want.double().cpu()).abs().max().item()
    scale = want.abs().max().item()
    print(f"{what}: max error {err:.3e} at scale {scale:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max error {err:.3e} vs scale {scale:.3e}"


def _against_stepwise(fast, stepwise, what=""):
    for label in fast:
        for name, want in stepwise[label].items():
            _close(fast[label][name], want, f"{what}{label} {name}", 5e-4 if name in ("ys", "log_ratio") else 2e-3)


# ---- 1. parity and route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.id for c in CASES])
def test_values_and_gradients_against_the_stepwise_route_and_the_oracle(index):
    case = CASES[index]
    ref = _oracle(index)
    assert ref["min_g"] >= L.MIN_DIFFUSION, f"the reference run meets |g| = {ref['min_g']:.3e}: an ill-conditioned case"
    fast = L.solve(case, DEV, expect_route=True)             # (the second solve of the form: the trusted one)
    stepwise = L.solve(case, DEV, fast=False, expect_route=False)
    assert set(fast) == {"all", "log_ratio only", "ys only"}
    assert set(fast["all"]) == set(L.quantities(case.module()))
    _against_stepwise(fast, stepwise)
    records, failures = L.compare(fast, ref)
    for what, err_new, err_ref, ratio in records:
        print(f"{case.id} {what}: err {err_new:.3e} ref {err_ref:.3e} ratio {ratio:.2f}")
    assert not failures, "\n".join(failures)


# ---- 2. chunking is invisible ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", (1, 5), ids=[CASES[i].id for i in (1, 5)])
def test_a_stash_budget_of_five_steps_changes_no_state_gradient(index, monkeypatch):
    from torchsde_amd import mlp_adjoint
    case = CASES[index]
    whole = L.solve(case, DEV, expect_route=True)
    monkeypatch.setattr(mlp_adjoint._MlpAdjointFn, "STASH_BYTES", 5 * case.B * (2 * case.d + 2 * case.hidden) * 4)
    chunked = L.solve(case, DEV, expect_route=True)
    for label in whole:
        for name in ("ys", "log_ratio", "y0"):
            assert torch.equal(chunked[label][name], whole[label][name]), (label, name)
        for name, want in whole[label].items():
            _close(chunked[label][name], want, f"chunked {label} {name}", 1e-4)


# ---- 3. sharding -----------------------------------------------------------------------------------------------------------------
def test_shards_equal_the_rows_of_the_whole():
    import torchsde_amd
    case = L.Case(50, (8, 20, 36), L.SCHEMES[0], "tanh")
    sde = case.module().to(DEV)
    ts = torch.tensor(case.ts(), device=DEV)
    y0_all = case.y0().to(DEV)

    def run(rows, offset):
        y0 = y0_all[offset:offset + rows].clone().requires_grad_(True)
        for _ in range(2):       # per batch size: the verifying solve, then the trusted one
            ys, log_ratio = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=L.brownian(case, DEV, rows=rows, row_offset=offset),
                                                        method=case.method, adjoint_method=case.adjoint_method, dt=L.DT,
                                                        logqp=True)
        assert L.graph_has(ys, FN)
        return ys.detach(), log_ratio.detach()

    ys, log_ratio = run(8, 0)
    for offset in (0, 4):
        ys_part, lr_part = run(4, offset)
        assert torch.equal(ys_part, ys[:, offset:offset + 4]), offset
        assert torch.equal(lr_part, log_ratio[:, offset:offset + 4]), offset


# ---- 4. prior forms and names= ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior, theta_elements, names", (
    ("mean_reverting", None, None),
    ("mean_reverting", 1, None),
    ("numbers", None, None),
    ("ou", None, {"prior_drift": "prior"}),
))
def test_prior_forms_take_the_route_and_their_parameters_get_the_stepwise_gradients(prior, theta_elements, names):
    case = L.Case(60, (37, 20, 36), L.SCHEMES[2], "softplus")
    kw = {} if theta_elements is None else {"theta_elements": theta_elements}
    module = case.module(prior=prior, named=names is not None, **kw)
    assert hasattr(module, "h") == (names is None)
    fast = L.solve(case, DEV, module=module, names=names, expect_route=True)
    stepwise = L.solve(case, DEV, module=module, names=names, fast=False, expect_route=False)
    expected = {"mean_reverting": {"theta", "mu"}, "numbers": set(), "ou": {"theta"}}[prior]
    assert expected <= set(fast["all"]) and not ({"theta", "mu"} - expected) & set(fast["all"])
    for name in expected:
        assert fast["log_ratio only"][name].abs().max().item() > 0.0, name
    _against_stepwise(fast, stepwise, what=f"{prior} ")


# ---- 5. what stays stepwise ------------------------------------------------------------------------------------------------------
def _stepwise_case():
    return L.Case(70, (16, 4, 16), L.SCHEMES[0], "tanh")


@pytest.mark.parametrize("what", ("tanh prior", "prior with t", "midpoint forward", "srk forward", "stratonovich",
                                  "adjoint_params subset", "trajectory_kernel off"))
def test_other_calls_stay_on_the_stepwise_route_with_unchanged_results(what):
    import torchsde_amd
    case = _stepwise_case()
    prior = {"tanh prior": "tanh", "prior with t": "times_t"}.get(what, "ou")
    strat = what in ("stratonovich", "midpoint forward")
    sde = case.module(prior=prior, sde_type="stratonovich" if strat else "ito").to(DEV)
    method = {"midpoint forward": "midpoint", "srk forward": "srk", "stratonovich": "milstein"}.get(what, "euler")
    adjoint_method = {"midpoint forward": "midpoint", "stratonovich": "milstein"}.get(what, "euler")
    ts = torch.tensor(case.ts(), device=DEV)
    params = [sde.lin1.weight] if what == "adjoint_params subset" else None

    def run(**kw):
        import torchsde_amd
        y0 = case.y0().to(DEV).requires_grad_(True)
        bm = torchsde_amd.BrownianInterval(0.0, L.STEPS * L.DT, size=(case.B, case.d + 1), dtype=torch.float32, device=DEV,
                                           entropy=case.entropy, dt=L.DT,
                                           levy_area_approximation="space-time" if method == "srk" else "none")
        out = None
        for _ in range(2):
            ys, log_ratio = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method=method, adjoint_method=adjoint_method,
                                                        dt=L.DT, logqp=True, adjoint_params=params, **kw)
            assert not L.graph_has(ys, FN), what
            wanted = [y0] + [p for p in (params or sde.parameters())]
            grads = torch.autograd.grad(ys.sum() + log_ratio.sum(), wanted, allow_unused=True)
            out = [ys.detach(), log_ratio.detach()] + [g for g in grads if g is not None]
        return out

    off = {"adjoint_options": {"trajectory_kernel": False}}
    got = run(**(off if what == "trajectory_kernel off" else {}))
    want = run(**off)                       # the parent's behaviour: the stepwise stochastic adjoint
    assert len(got) == len(want)
    for a, b in zip(got[:2], want[:2]):
        assert torch.equal(a, b), what
    for a, b in zip(got[2:], want[2:]):      # (sums over the batch: the same kernels, not necessarily the same order)
        _close(a, b, what, 1e-5)


def test_without_logqp_the_same_object_keeps_its_own_route_and_its_own_trust():
    import torchsde_amd
    from torchsde_amd import trust
    case = _stepwise_case()
    # (a prior without parameters of its own: `mlp_adjoint.route` takes a module whose parameters are the six tensors only)
    sde = case.module(prior="numbers").to(DEV)
    ts = torch.tensor(case.ts(), device=DEV)

    def run(logqp):
        y0 = case.y0().to(DEV).requires_grad_(True)
        width = case.d + 1 if logqp else case.d
        bm = torchsde_amd.BrownianInterval(0.0, L.STEPS * L.DT, size=(case.B, width), dtype=torch.float32, device=DEV,
                                           entropy=case.entropy, dt=L.DT)
        out = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method="euler", adjoint_method="euler", dt=L.DT, logqp=logqp)
        return out[0] if logqp else out

    for _ in range(2):
        ys_kl = run(True)
    assert L.graph_has(ys_kl, FN)
    ys = run(False)
    assert type(ys.grad_fn).__name__.startswith("_MlpAdjointFn")
    assert L.graph_has(run(True), FN)
    verdicts = trust.book_of(sde)["trusted"]
    assert all(v is True for v in verdicts.values())
    assert sum("logqp" in key for key in verdicts) == 1 and sum("logqp" not in key for key in verdicts) >= 1


# ---- 6. the guard works ----------------------------------------------------------------------------------------------------------
def test_a_wrong_column_cotangent_is_refused_and_the_caller_gets_the_stepwise_result(monkeypatch):
    from torchsde_amd import mlp_adjoint, trust
    import torchsde_amd
    case = L.Case(80, (37, 20, 36), L.SCHEMES[0], "softplus")
    sde = case.module().to(DEV)
    params = list(sde.parameters())
    ts = torch.tensor(case.ts(), device=DEV)
    _, wy, wl = case.cotangents()[0]
    honest = mlp_adjoint.adjoint_mlp_diag_logqp

    def wrong(y, a, a_l, *rest, **kw):
        return honest(y, a, a_l * 1.01, *rest, **kw)

    def call(**kw):
        y0 = case.y0().to(DEV).requires_grad_(True)
        ys, log_ratio = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=L.brownian(case, DEV), method=case.method,
                                                    adjoint_method=case.adjoint_method, dt=L.DT, logqp=True, **kw)
        grads = torch.autograd.grad([ys, log_ratio], [y0] + params, grad_outputs=[wy.to(DEV), wl.to(DEV)])
        return L.graph_has(ys, FN), [ys.detach(), log_ratio.detach()] + list(grads)

    monkeypatch.setattr(mlp_adjoint, "adjoint_mlp_diag_logqp", wrong)
    routed, got = call()                       # the verifying solve: both routes, the stepwise result returned
    assert not routed
    verdicts = [v for k, v in trust.book_of(sde)["trusted"].items() if "logqp" in k]
    assert len(verdicts) == 1 and verdicts[0] is not True and "gradient" in verdicts[0], verdicts
    assert not call()[0]                       # ... and the form stays stepwise from then on
    monkeypatch.undo()
    _, want = call(adjoint_options={"trajectory_kernel": False})
    for a, b in zip(got[:2], want[:2]):
        assert torch.equal(a, b)
    for a, b in zip(got[2:], want[2:]):
        _close(a, b, "gradient of the verifying solve", 1e-5)


# ---- 7. create_graph=True --------------------------------------------------------------------------------------------------------
def test_second_derivative_equals_the_stepwise_routes():
    """The first backward pass with a graph goes to the differentiable sweep (adjoint_double) on the wrapped SDE, as on the
    stepwise route: the two second derivatives come from the same torch program over forward states that agree to float32
    rounding -- compared at the tolerance of tests/test_gpu_double_backward.py's perceptron case, 2e-4 of scale + 1e-6."""
    import torchsde_amd
    case = _stepwise_case()
    sde = case.module().to(DEV)
    ts = torch.tensor(case.ts(), device=DEV)
    params = list(sde.parameters())

    def second(fast):
        for _ in range(2 if fast else 1):
            y0 = case.y0().to(DEV).requires_grad_(True)
            ys, log_ratio = torchsde_amd.sdeint_adjoint(
                sde, y0, ts, bm=L.brownian(case, DEV), method="euler", adjoint_method="euler", dt=L.DT, logqp=True,
                adjoint_options={} if fast else {"trajectory_kernel": False})
        assert L.graph_has(ys, FN) == fast
        first = torch.autograd.grad((ys[-1] ** 2).sum() + log_ratio.sum(), [y0] + params, create_graph=True)
        penalty = sum((g ** 2).sum() for g in first)
        return [g.detach() for g in first], torch.autograd.grad(penalty, [y0] + params, allow_unused=True)

    first_fast, second_fast = second(True)
    first_step, second_step = second(False)
    for a, b in zip(first_fast, first_step):
        _close(a, b, "first derivative with a graph", 2e-3)
    assert any(h is not None and float(h.abs().max()) > 0.0 for h in second_step)
    for a, b in zip(second_fast, second_step):
        assert (a is None) == (b is None)
        if a is not None:
            scale = float(b.abs().max())
            err = float((a - b).abs().max())
            print(f"second derivative: max error {err:.3e} at scale {scale:.3e}")
            assert err <= 2e-4 * scale + 1e-6
