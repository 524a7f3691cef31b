"""``sdeint(..., logqp=True)`` on the KL instantiations of the perceptron kernels (run with ``-m gpu``;
torchsde_amd/mlp_adjoint.py: plan_logqp_sdeint; torchsde_amd/kernels.py: _MlpLogqpTrajectoryFn; csrc:
tsde_trajectory_mlp_diag_logqp, tsde_trajectory_mlp_diag_logqp_backward) for an unchanged user module with a per-channel affine
prior drift, sampling and training, against

(a) the oracle: autograd through oracle.solvers_ref.integrate over `LogqpRef` in float32 and float64 on the same counter path,
    through `helpers.assert_within_reference_rounding` with the measured factor of tests/helpers_logqp_backprop.py;
(b) this package's stepwise route of the same call (``options={"trajectory_kernel": False}``), at the tolerances of
    tests/test_gpu_mlp_logqp_adjoint.py: 5e-4 of scale for values, 2e-3 for gradients.

Cases, reference and solves: tests/helpers_logqp_backprop.py (modules and comparison: tests/helpers_logqp.py). The KL column's
row sum is an f32 sum in the kernel's own order, so nothing here is bit-equal to the stepwise route; chunks, re-runs and shards
of the route itself are."""
import functools

import pytest
import torch

from tests import helpers
from tests import helpers_logqp as L
from tests import helpers_logqp_backprop as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = P.cases()
FN = P.FN


@functools.lru_cache(maxsize=None)
def _oracle(index):
    """Computed once per case, shared, never written to."""
    return P.oracle(CASES[index])


def _close(got, want, what, tol):
    err = (got.double().cpu() - want.double().cpu()).abs().max().item()
    scale = want.abs().max().item()
    print(f"{what}: max error {err:.3e} at scale {scale:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max error {err:.3e} vs scale {scale:.3e}"


def _against_stepwise(fast, stepwise, what=""):
    for label in fast:
        for name, want in stepwise[label].items():
            _close(fast[label][name], want, f"{what}{label} {name}", 5e-4 if name in ("ys", "log_ratio") else 2e-3)


# ---- 1. values and gradients; the route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.id for c in CASES])
def test_values_and_gradients_against_the_oracle_and_the_stepwise_route(index):
    case = CASES[index]
    ref = _oracle(index)
    assert ref["min_g"] >= L.MIN_DIFFUSION, f"the reference run meets |g| = {ref['min_g']:.3e}: an ill-conditioned case"
    fast = P.solve(case, DEV, expect_route=True)       # (the first solve must not, the second must go through the Function)
    stepwise = P.solve(case, DEV, fast=False, expect_route=False)
    assert set(fast) == {"all", "log_ratio only", "ys only"}
    assert set(fast["all"]) == set(L.quantities(case.module()))
    records, failures = P.compare(fast, ref)
    for what, err_new, err_ref, ratio in records:
        print(f"{case.id} {what}: err {err_new:.3e} ref {err_ref:.3e} ratio {ratio:.2f}")
    _against_stepwise(fast, stepwise)
    assert not failures, "\n".join(failures)


# ---- 2. sampling ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", (1, 5, 8), ids=[CASES[i].id for i in (1, 5, 8)])
def test_sampling_is_one_launch_interpolates_and_survives_reverification(index, monkeypatch):
    from torchsde_amd import mlp_adjoint, solvers, trust
    case = CASES[index]
    ts = [0.0, 2.5 * P.DT, 9 * P.DT, 16 * P.DT]
    ref = P.oracle(case, ts=ts, gradients=False)
    assert ref["min_g"] >= L.MIN_DIFFUSION
    sde = case.module().to(DEV)
    launches = []
    honest = mlp_adjoint.trajectory_mlp_diag_logqp
    monkeypatch.setattr(mlp_adjoint, "trajectory_mlp_diag_logqp", lambda *a, **k: (launches.append(1), honest(*a, **k))[1])

    def run():
        with torch.no_grad():
            ys, log_ratio, _ = P.call(case, sde, DEV, y0=case.y0().to(DEV), ts=ts)
        return ys, log_ratio

    untrusted = run()                                    # both routes, the stepwise result
    del launches[:]
    ys, log_ratio = run()
    assert len(launches) == 1 and ys.shape == (4, case.B, case.d) and log_ratio.shape == (3, case.B)
    records, failures = P.compare({"values": {"ys": ys, "log_ratio": log_ratio}}, ref)
    for what, err_new, err_ref, ratio in records:
        print(f"{case.id} sampling {what}: err {err_new:.3e} ref {err_ref:.3e} ratio {ratio:.2f}")
    assert not failures, "\n".join(failures)
    for got, want, name in zip((ys, log_ratio), untrusted, ("ys", "log_ratio")):
        _close(got, want, f"sampling against the stepwise route, {name}", 5e-4)
    keys = [k for k, v in trust.book_of(sde)["trusted"].items() if "sampling" in k]
    assert len(keys) == 1 and trust.book_of(sde)["trusted"][keys[0]] is True
    assert any("tsde_trajectory_mlp_diag_logqp" in line for line in trust.describe(sde))
    monkeypatch.setattr(solvers, "VERIFY_EVERY", 1)      # every solve verifies again and returns the stepwise result
    again = run()
    assert torch.equal(again[0], untrusted[0]) and torch.equal(again[1], untrusted[1])


# ---- 3. chunking and re-running are invisible -----------------------------------------------------------------------------------
@pytest.mark.parametrize("index", (1, 8), ids=[CASES[i].id for i in (1, 8)])
def test_a_stash_budget_of_five_steps_changes_no_state_gradient(index, monkeypatch):
    from torchsde_amd import kernels
    case = CASES[index]
    whole = P.solve(case, DEV, expect_route=True)
    monkeypatch.setattr(kernels._MlpLogqpTrajectoryFn, "STASH_BYTES", 5 * case.B * (case.d + 2 * case.hidden) * 4)
    chunked = P.solve(case, DEV, expect_route=True)
    for label in whole:
        for name in ("ys", "log_ratio", "y0"):
            assert torch.equal(chunked[label][name], whole[label][name]), (label, name)
        for name, want in whole[label].items():
            _close(chunked[label][name], want, f"chunked {label} {name}", 1e-4)


@pytest.mark.parametrize("index", (1, 8), ids=[CASES[i].id for i in (1, 8)])
def test_a_small_state_budget_reruns_each_chunk_with_identical_results(index, monkeypatch):
    from torchsde_amd import kernels
    from torchsde_amd import mlp_adjoint
    case = CASES[index]
    whole = P.solve(case, DEV, expect_route=True)
    launches = []
    honest = mlp_adjoint.trajectory_mlp_diag_logqp
    monkeypatch.setattr(mlp_adjoint, "trajectory_mlp_diag_logqp", lambda *a, **k: (launches.append(1), honest(*a, **k))[1])
    monkeypatch.setattr(kernels._MlpLogqpTrajectoryFn, "STASH_BYTES", 5 * case.B * (case.d + 2 * case.hidden) * 4)
    monkeypatch.setattr(kernels._MlpLogqpTrajectoryFn, "STATE_BYTES", 1)
    rerun = P.solve(case, DEV, expect_route=True)
    # a forward launch per solve; 4 chunks of <= 5 steps run again in each backward pass: one of the verifying solve, then three
    assert len(launches) == 2 + 4 * (1 + 3), len(launches)
    for label in whole:
        for name in ("ys", "log_ratio", "y0"):
            assert torch.equal(rerun[label][name], whole[label][name]), (label, name)
        for name, want in whole[label].items():
            _close(rerun[label][name], want, f"re-run {label} {name}", 1e-4)


# ---- 4. sharding ----------------------------------------------------------------------------------------------------------------
def test_shards_equal_the_rows_of_the_whole():
    case = CASES[1]                                      # 37 x 20 x 36
    sde = case.module().to(DEV)
    y0_all = case.y0().to(DEV)
    _, wy, wl = case.cotangents()[0]

    def run(rows, offset):
        for _ in range(2):       # per batch size: the verifying solve, then the trusted one
            y0 = y0_all[offset:offset + rows].clone().requires_grad_(True)
            ys, log_ratio, _ = P.call(case, sde, DEV, y0=y0, rows=rows, row_offset=offset)
        assert L.graph_has(ys, FN)
        grad, = torch.autograd.grad([ys, log_ratio], [y0], grad_outputs=[wy[:, offset:offset + rows].to(DEV),
                                                                        wl[:, offset:offset + rows].to(DEV)])
        return ys.detach(), log_ratio.detach(), grad

    ys, log_ratio, grad = run(case.B, 0)
    for rows, offset in ((20, 0), (17, 20)):
        ys_part, lr_part, grad_part = run(rows, offset)
        assert torch.equal(ys_part, ys[:, offset:offset + rows]), offset
        assert torch.equal(lr_part, log_ratio[:, offset:offset + rows]), offset
        assert torch.equal(grad_part, grad[offset:offset + rows]), offset


# ---- 5. prior forms and names= --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior, theta_elements, names", (
    ("ou", None, None),
    ("mean_reverting", None, None),
    ("numbers", None, None),
    ("ou", 1, None),
    ("ou", None, {"prior_drift": "prior"}),
))
def test_prior_forms_take_the_route_and_their_parameters_get_the_stepwise_gradients(prior, theta_elements, names):
    case = L.Case(60, (37, 20, 36), P.SCHEMES[0], "softplus")
    kw = {} if theta_elements is None else {"theta_elements": theta_elements}
    module = case.module(prior=prior, named=names is not None, **kw)
    assert hasattr(module, "h") == (names is None)
    fast = P.solve(case, DEV, module=module, names=names, expect_route=True)
    stepwise = P.solve(case, DEV, module=module, names=names, fast=False, expect_route=False)
    expected = {"mean_reverting": {"theta", "mu"}, "numbers": set(), "ou": {"theta"}}[prior]
    assert expected <= set(fast["all"]) and not ({"theta", "mu"} - expected) & set(fast["all"])
    for name in expected:
        assert fast["log_ratio only"][name].abs().max().item() > 0.0, name
    _against_stepwise(fast, stepwise, what=f"{prior} ")


# ---- 6. what stays stepwise -----------------------------------------------------------------------------------------------------
def _stepwise_case(diffusion="sigmoid"):
    return L.Case(70, (16, 4, 16), ("euler", None, diffusion), "tanh")


STEPWISE = ("tanh prior", "prior with t", "stratonovich", "srk", "sigmoid with milstein", "adaptive", "extra",
            "extra_solver_state", "foreign brownian motion", "trajectory_kernel off", "hip_graph", "TSDE_RECOGNISE=0")


@pytest.mark.parametrize("what", STEPWISE)
def test_other_calls_stay_on_the_stepwise_route_with_unchanged_results(what, monkeypatch):
    import torchsde_amd
    from torchsde_amd import recognise
    case = _stepwise_case()
    prior = {"tanh prior": "tanh", "prior with t": "times_t"}.get(what, "ou")
    sde = case.module(prior=prior, sde_type="stratonovich" if what == "stratonovich" else "ito").to(DEV)
    method = {"stratonovich": "midpoint", "srk": "srk", "sigmoid with milstein": "milstein"}.get(what, "euler")
    ts = torch.tensor(case.ts(), device=DEV)
    if what == "TSDE_RECOGNISE=0":
        monkeypatch.setattr(recognise, "ENABLED", False)
    gen = torch.Generator().manual_seed(7)
    table = {(k * P.DT, (k + 1) * P.DT): ((P.DT ** 0.5) * torch.randn(case.B, case.d + 1, generator=gen).to(DEV), None, None)
             for k in range(P.STEPS)}

    def run(**options):
        out = None
        for _ in range(2):
            y0 = case.y0().to(DEV).requires_grad_(True)
            if what == "foreign brownian motion":
                bm = helpers.make_replay_bm(table, (case.B, case.d + 1), torch.float32, DEV, "none")
            else:
                bm = torchsde_amd.BrownianInterval(0.0, P.STEPS * P.DT, size=(case.B, case.d + 1), dtype=torch.float32,
                                                   device=DEV, entropy=case.entropy, dt=P.DT,
                                                   levy_area_approximation="space-time" if method == "srk" else "none")
            kw = {"adaptive": True} if what == "adaptive" else {}
            if what == "extra":
                kw["extra"] = True
            if what == "extra_solver_state":
                kw["extra_solver_state"] = ()
            if what == "hip_graph":
                options = dict(options, hip_graph=True)
            ys, log_ratio = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=P.DT, logqp=True,
                                                options=options or None, **kw)[:2]
            assert not L.graph_has(ys, FN), what
            grads = torch.autograd.grad(ys.sum() + log_ratio.sum(), [y0] + list(sde.parameters()), allow_unused=True)
            out = [ys.detach().clone(), log_ratio.detach().clone()] + [g.clone() for g in grads if g is not None]
        return out

    got = run(**({"trajectory_kernel": False} if what == "trajectory_kernel off" else {}))
    want = run(trajectory_kernel=False)                 # the parent's path for this call
    assert len(got) == len(want)
    for a, b in zip(got[:2], want[:2]):
        assert torch.equal(a, b), what
    for a, b in zip(got[2:], want[2:]):
        _close(a, b, what, 1e-5)


# ---- 7. the guard works ---------------------------------------------------------------------------------------------------------
def test_a_wrong_column_cotangent_is_refused_and_the_caller_gets_the_stepwise_result(monkeypatch):
    from torchsde_amd import kernels, trust
    case = L.Case(80, (37, 20, 36), P.SCHEMES[0], "softplus")
    sde = case.module().to(DEV)
    params = list(sde.parameters())
    _, wy, wl = case.cotangents()[0]
    honest = kernels._MlpLogqpTrajectoryFn.backward

    def wrong(ctx, gys):
        gys = gys.clone()
        gys[:, :, -1] *= 1.01
        return honest(ctx, gys)

    def call(**kw):
        ys, log_ratio, y0 = P.call(case, sde, DEV, **kw)
        grads = torch.autograd.grad([ys, log_ratio], [y0] + params, grad_outputs=[wy.to(DEV), wl.to(DEV)])
        return L.graph_has(ys, FN), [ys.detach(), log_ratio.detach()] + list(grads)

    monkeypatch.setattr(kernels._MlpLogqpTrajectoryFn, "backward", staticmethod(wrong))
    routed, got = call()                       # the verifying solve: both routes, the stepwise result returned
    assert not routed
    verdicts = [v for k, v in trust.book_of(sde)["trusted"].items() if "backprop" in k]
    assert len(verdicts) == 1 and verdicts[0] is not True and "gradient" in verdicts[0], verdicts
    assert not call()[0]                       # ... and the form stays stepwise from then on
    monkeypatch.undo()
    _, want = call(options={"trajectory_kernel": False})
    for a, b in zip(got[:2], want[:2]):
        assert torch.equal(a, b)
    for a, b in zip(got[2:], want[2:]):
        _close(a, b, "gradient of the verifying solve", 1e-5)


# ---- 8. one object, three routes, three keys ------------------------------------------------------------------------------------
def test_each_route_of_one_object_keeps_its_own_trust():
    import torchsde_amd
    from torchsde_amd import trust
    case = _stepwise_case()
    # (a prior without parameters of its own: `mlp_adjoint.route` takes a module whose parameters are the six tensors only)
    sde = case.module(prior="numbers").to(DEV)
    ts = torch.tensor(case.ts(), device=DEV)

    def bm(width):
        return torchsde_amd.BrownianInterval(0.0, P.STEPS * P.DT, size=(case.B, width), dtype=torch.float32, device=DEV,
                                             entropy=case.entropy, dt=P.DT)

    def adjoint():
        y0 = case.y0().to(DEV).requires_grad_(True)
        return torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm(case.d + 1), method="euler", adjoint_method="euler", dt=P.DT,
                                           logqp=True)[0]

    def backprop():
        return P.call(case, sde, DEV)[0]

    def plain():
        with torch.no_grad():
            return torchsde_amd.sdeint(sde, case.y0().to(DEV), ts, bm=bm(case.d), method="euler", dt=P.DT)

    for solve in (adjoint, backprop, plain, adjoint, backprop, plain):
        ys = solve()
    assert ys.grad_fn is None
    assert L.graph_has(adjoint(), "_MlpLogqpAdjointFn") and L.graph_has(backprop(), FN)
    verdicts = trust.book_of(sde)["trusted"]
    assert all(v is True for v in verdicts.values()), verdicts
    logqp_keys = [key for key in verdicts if "logqp" in key]
    assert len(logqp_keys) == 2 and sum("backprop" in key for key in logqp_keys) == 1
    assert sum("logqp" not in key for key in verdicts) >= 1
    assert any("tsde_trajectory_mlp_diag_logqp_backward" in line for line in trust.describe(sde))


# ---- 9. no double backward ------------------------------------------------------------------------------------------------------
def test_a_backward_pass_with_a_graph_raises():
    case = _stepwise_case()
    sde = case.module().to(DEV)
    for _ in range(2):
        ys, log_ratio, y0 = P.call(case, sde, DEV)
    assert L.graph_has(ys, FN)
    with pytest.raises(NotImplementedError, match="no differentiable backward pass was prepared"):
        torch.autograd.grad((ys[-1] ** 2).sum() + log_ratio.sum(), [y0], create_graph=True)
