"""Row-coupled systems TRAIN through `sdeint` in one launch (``-m gpu``): the generated tangent unit
(specialise.source_rows_sens, csrc/trajectory.hip trajectory_rows_sens_kernel) behind kernels._RowsTrajectoryFn. Its values
are the bits of the `no_grad` rows route, its gradients are held to the float64 oracle's rounding, the verifying solve catches
a wrong backward pass, and everything outside the route's conditions stays stepwise with unchanged results. Shapes: 257 rows
(a ragged second block) and one row; d = 2, 3 and 8 at the size rule's cap; 16 steps of 2^-8; outputs on step boundaries and
one inside a step; float32 and float64."""
import unittest.mock as mock

import pytest
import torch

from tests import helpers
from tests import helpers_rows_grad as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
FN = "_RowsTrajectoryFnBackward"


@pytest.fixture(autouse=True)
def _compile_in_the_calling_thread(monkeypatch, tmp_path_factory):
    from torchsde_amd import specialise
    monkeypatch.setattr(specialise, "MODE", "sync")
    monkeypatch.setenv("TSDE_SPECIALISE_CACHE", str(tmp_path_factory.getbasetemp() / "specialised"))
    yield


def _routed(ys):
    return type(ys.grad_fn).__name__ == FN


def _launches(fn):
    from torchsde_amd import kernels as K
    K.prof_begin(8, 64)
    out = fn()
    torch.cuda.synchronize()
    return out, K.prof_end()[1]


def _book(sde):
    from torchsde_amd import trust
    return trust.book_of(sde) or {"trusted": {}, "refused": {}}


def _case(name):
    return [c for c in H.CASES if c.name == name][0]


# ---- 1. route and bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("lorenz", torch.float32), ("lorenz", torch.float64), ("vanderpol", torch.float32),
                                        ("vanderpol", torch.float64), ("vanderpol_strat", torch.float32),
                                        ("ring8", torch.float32)])
def test_one_launch_with_the_bits_of_the_no_grad_rows_route(name, dtype):
    case = _case(name)
    sde = case.module().to(DEV).to(dtype)
    first, _ = H.solve(case, sde, DEV, dtype)                     # the verifying solve: both routes, the stepwise result
    assert not _routed(first) and first.grad_fn is not None
    verdicts = [v for k, v in _book(sde)["trusted"].items() if "autograd" in k]
    assert verdicts == [True], _book(sde)
    (ys, _), launches = _launches(lambda: H.solve(case, sde, DEV, dtype, entropy=case.entropy + 1))
    assert _routed(ys) and launches == 1
    H.solve(case, sde, DEV, dtype, grad=False)                    # (the forward route's own verifying solve)
    (plain, _), launches = _launches(lambda: H.solve(case, sde, DEV, dtype, grad=False, entropy=case.entropy + 1))
    assert launches == 1 and plain.grad_fn is None
    assert torch.equal(ys.detach(), plain)
    from torchsde_amd import recognise
    assert any("generated tangent unit: autograd" in line for line in recognise.describe(sde)), recognise.describe(sde)


# ---- 2. gradients against the float64 oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(H.CASES)), ids=[c.id for c in H.CASES])
def test_gradients_within_the_float64_oracles_rounding(index):
    for label, name, new32, ref32, ref64 in H.measured(index, DEV):
        assert tuple(new32.shape) == tuple(ref64.shape), (label, name)
        err_new, err_ref = (float((x.detach().double().cpu() - ref64).abs().max()) for x in (new32, ref32))
        print(f"{H.CASES[index].id} {label} {name}: |hip32 - ref64| = {err_new:.3e}, |ref32 - ref64| = {err_ref:.3e}")
        helpers.assert_within_reference_rounding(new32, ref32, ref64, what=f"{H.CASES[index].id} {label} {name}",
                                                 factor=H.ROWS_GRAD_FACTOR, floor=H.ROWS_GRAD_FLOOR)


def test_float64_gradients_are_the_oracles():
    """The float64 kernel against the float64 oracle: the same operations in another order at a few places (the tangents'
    sums), 16 steps -- 1e-11 of each quantity's scale is some 1e5 units in the last place, far above that rounding and far
    below any error of the method."""
    index = 0
    case = H.CASES[index]
    sde = case.module().to(DEV).double()
    H.solve(case, sde, DEV, torch.float64)
    ys, y0 = H.solve(case, sde, DEV, torch.float64)
    assert _routed(ys)
    ys64, grads64 = H.oracle(index)[torch.float64]
    for label, w in case.cotangents():
        got = H.quantities(case, ys.detach(), H.gradients(case, sde, ys, y0, w))
        for (name, a), (_, b) in zip(got, H.quantities(case, ys64, grads64[label])):
            assert float((a.cpu() - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), (label, name)


# ---- 3. training changes what the kernel sees -----------------------------------------------------------------------------------
def test_an_optimiser_step_reaches_the_next_launch():
    case = _case("vanderpol")
    sde = case.module().to(DEV)
    optimiser = torch.optim.SGD(sde.parameters(), lr=0.05)
    H.solve(case, sde, DEV)                                       # the verifying solve
    before, _ = H.solve(case, sde, DEV)
    assert _routed(before)
    optimiser.zero_grad()
    before.square().mean().backward()
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in sde.parameters())
    optimiser.step()
    (after, _), launches = _launches(lambda: H.solve(case, sde, DEV))
    assert launches == 1 and _routed(after) and not torch.equal(after.detach(), before.detach())
    slow, _ = H.solve(case, sde, DEV, options={"trajectory_kernel": False})
    torch.testing.assert_close(after.detach(), slow.detach(), rtol=2e-5, atol=2e-6)


# ---- 4. the guard works ---------------------------------------------------------------------------------------------------------
def test_exchanged_scalar_gradients_are_refused_and_the_caller_gets_the_stepwise_result(monkeypatch):
    from torchsde_amd import kernels
    case = _case("lorenz")
    sde = case.module().to(DEV)
    _, w = case.cotangents()[0]
    honest = kernels._RowsTrajectoryFn.backward

    def wrong(ctx, gys):
        grads = list(honest(ctx, gys))
        grads[-4], grads[-3] = grads[-3], grads[-4]               # the gradients of a1 and a2 (the sources are a1, a2, a3, b)
        return tuple(grads)

    def call(**kw):
        ys, y0 = H.solve(case, sde, DEV, **kw)
        return _routed(ys), [ys.detach()] + list(H.gradients(case, sde, ys, y0, w))

    monkeypatch.setattr(kernels._RowsTrajectoryFn, "backward", staticmethod(wrong))
    routed, got = call()                                          # the verifying solve: both routes, the stepwise result returned
    assert not routed
    verdicts = [v for k, v in _book(sde)["trusted"].items() if "autograd" in k]
    assert len(verdicts) == 1 and verdicts[0] is not True and "gradient" in verdicts[0], verdicts
    assert not call()[0]                                          # ... and the form stays stepwise from then on
    monkeypatch.undo()
    _, want = call(options={"trajectory_kernel": False})
    assert torch.equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


# ---- 5. what stays stepwise, with unchanged results -----------------------------------------------------------------------------
def _stays_stepwise(case, sde, **kw):
    for _ in range(2):
        (ys, y0), launches = _launches(lambda: H.solve(case, sde, DEV, **kw))
        assert launches == 0 and not _routed(ys) and ys.grad_fn is not None
    want, _ = H.solve(case, sde, DEV, options={"trajectory_kernel": False})
    assert torch.equal(ys.detach(), want.detach())


def test_what_stays_stepwise():
    import torchsde_amd
    from torchsde_amd import recognise, specialise
    ring = _case("ring8")
    over = H.Case("ring8_over", lambda: H.Ring(8, H.RING_RATES + 1), 8, 257, "euler", "none")
    sde = over.module().to(DEV)
    _stays_stepwise(over, sde)
    assert any("more than the 84" in line for line in recognise.describe(sde)), recognise.describe(sde)
    with mock.patch.object(specialise, "compiler", lambda: None):
        _stays_stepwise(ring, ring.module().to(DEV))
    lorenz = _case("lorenz")
    milstein = H.Case("lorenz", H.Lorenz, 3, 257, "milstein", "none")
    _stays_stepwise(milstein, milstein.module().to(DEV))
    # sdeint_adjoint: the reference's backward pass, not this route. (Its forward pass runs under no_grad and, as before, takes
    # the forward rows route once that is verified -- a launch of the plain unit; the tangent unit must not be asked for.)
    from torchsde_amd import kernels
    sde = lorenz.module().to(DEV)
    y0 = lorenz.y0().to(DEV).requires_grad_(True)
    ts = torch.tensor(H.TS, device=DEV)
    _, w = lorenz.cotangents()[0]

    def adjoint(**options):
        bm = torchsde_amd.BrownianInterval(0.0, H.STEPS * H.DT, size=(lorenz.B, 3), device=DEV, entropy=lorenz.entropy)
        ys = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method="euler", dt=H.DT, options={"hip_graph": False, **options})
        return ys, torch.autograd.grad((ys * w.to(DEV)).sum(), [y0] + list(sde.parameters()))
    with mock.patch.object(kernels, "trajectory_rows_differentiable", side_effect=AssertionError("the tangent unit")):
        for _ in range(2):
            (ys, grads), launches = _launches(adjoint)
            assert not _routed(ys)
    assert not any("autograd" in k for k in _book(sde)["trusted"])
    # the launches of the second call are those of a verified no_grad forward solve: the plain unit, once
    _, forward_only = _launches(lambda: H.solve(lorenz, sde, DEV, grad=False))
    assert launches == forward_only == 1
    want, want_grads = adjoint(trajectory_kernel=False)
    assert torch.equal(ys.detach(), want.detach())
    for a, b in zip(grads, want_grads):
        assert torch.equal(a, b)


def test_over_the_byte_budget_the_solve_stays_stepwise(monkeypatch):
    from torchsde_amd import kernels
    case = _case("lorenz")
    sde = case.module().to(DEV)
    H.solve(case, sde, DEV)                                       # the verifying solve
    assert _routed(H.solve(case, sde, DEV)[0])
    needed = (len(H.TS) - 1) * 9 * case.B * case.d * 4            # sens: (n_out, NT, rows, d) float32
    monkeypatch.setattr(kernels, "ROWS_SENS_BYTES", needed - 1)
    _stays_stepwise(case, sde)
    monkeypatch.setattr(kernels, "ROWS_SENS_BYTES", needed)
    assert _routed(H.solve(case, sde, DEV)[0])


def test_describe_names_why_a_module_trains_stepwise():
    from torchsde_amd import recognise

    class Detached(H.Lorenz):
        def f(self, t, y):
            return super().f(t, y.detach())

    class Hidden(H.Lorenz):
        def __init__(self):
            super().__init__()
            self.shift = torch.nn.Parameter(torch.tensor(0.5))

        def g(self, t, y):
            return y * self.b + float(self.shift.detach())
    for make, reason in ((Detached, "stop-gradient"), (Hidden, "not reached")):
        case = H.Case("lorenz", make, 3, 257, "euler", "none")
        sde = case.module().to(DEV)
        _stays_stepwise(case, sde)
        lines = recognise.describe(sde)
        assert any("with autograd recording stays stepwise" in line and reason in line for line in lines), lines
