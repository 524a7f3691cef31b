"""When a reversible-Heun solve takes the matrix-core kernels of neural_rheun.py.

An UNCHANGED user module whose drift and diffusion are perceptrons of (t, y) -- the reference's `Neural*` problems
(tests/problems.py:135-252) and the generator of examples/sde_gan.py:77-101 -- solved with ``method="reversible_heun"``:
``sdeint`` (with or without autograd recording) and ``sdeint_adjoint(..., adjoint_method="adjoint_reversible_heun")``, the
pair the reference recommends for training (DOCUMENTATION.md:97,118). The module is interpreted at every solve
(recognise.py, `deep_spec`), so the weights are this solve's live values and the kernels' gradients land on the user's own
tensors. Trust is earned as on the other recognised routes (solvers._integrate_recognised): the first solve of a (form, batch
size, route) on an SDE object runs BOTH ways and returns the stepwise result; values are compared elementwise and -- when a
gradient can flow -- the gradients with respect to y0 and every parameter for one random cotangent
(solvers._both_routes_agree). ``options={"trajectory_kernel": False}`` opts out; ``TSDE_VERIFY_EVERY`` re-verifies.
"""
import numpy as np
import torch

from . import kernels as K
from . import neural_rheun
from . import timegrid
from . import trust
from .brownian import BrownianInterval
from .settings import NOISE_TYPES


class Route:
    """One solve's plan on the kernels: `solve(y0)` launches it; `record(fast, stepwise, y0)` files the verdict of a verifying
    solve."""

    def __init__(self, solver, spec, schedule, times_host, ledger, key, trusted, reverify):
        self.solver, self.spec, self.schedule, self.times_host = solver, spec, schedule, times_host
        self.ledger, self.key, self.trusted, self.reverify = ledger, key, trusted, reverify

    def solve(self, y0, z_holder=None):
        _, drift, diffusion, noise, m = self.spec
        return neural_rheun.solve(y0, drift, diffusion, noise, m, self.schedule, self.times_host, self.solver._native_bm(),
                                  z_holder)

    def parameters(self):
        return self.spec[1].parameters() + self.spec[2].parameters()

    def record(self, fast, stepwise, y0, extra_inputs=()):
        verdict = self.solver._both_routes_agree(fast, stepwise, y0, "the reversible-Heun kernels", network=True,
                                                 extra_inputs=extra_inputs)
        self.ledger.file(self.key, verdict, self.reverify)
        return verdict


def plan(solver, y0, ts, differentiable, need_boundaries=False, tag=()):
    """The `Route` of this solve, or None when it stays stepwise. `differentiable`: a gradient will be asked of the result (the
    interpretation then watches for stop-gradients); `need_boundaries`: every output must sit on a step boundary (the backward
    sweep of `sdeint_adjoint` steps to each of them, adjoint.py:97-112, and the kernels' own sweep does not split an
    interpolated output's cotangent between the two states it mixes: every solve with a gradient asks for this). Checked
    before the ledger is consulted, so a solve that fails it files no verdict."""
    from . import recognise
    from .sde import ForwardSDE
    sde, bm = solver.sde, solver._native_bm()
    if (not recognise.ENABLED or not solver.options.get("trajectory_kernel", True) or solver.adaptive
            or type(sde) is not ForwardSDE or sde.user_product
            or sde.noise_type not in (NOISE_TYPES.diagonal, NOISE_TYPES.scalar, NOISE_TYPES.general)):
        return None
    if (not isinstance(bm, BrownianInterval) or y0.dim() != 2 or len(bm.shape) != 2 or bm.shape[0] != y0.shape[0]
            or not y0.is_cuda or y0.shape[0] < 1 or y0.dtype != torch.float32 or ts.dtype != y0.dtype or bm.dtype != y0.dtype
            or bm._rootW is not None or bm._rootH is not None or bm._snap or torch.cuda.is_current_stream_capturing()
            or y0.numel() >= 2 ** 30):
        return None
    ledger = trust.open_book(solver, who=type(solver).__name__ + (":kernels, with gradients" if differentiable else ":kernels"))
    if ledger is None or ledger.refused():
        return None
    try:
        found = recognise.recognise(sde, ts[0], y0, differentiable=differentiable)
        if not found.neural:
            raise recognise.NotElementwise("drift and diffusion are not both networks of (t, y)")
        spec = found.deep_spec(sde.noise_type)
    except recognise.NotElementwise as e:
        return ledger.refuse(str(e))
    if tuple(bm.shape) != (y0.shape[0], spec[4]):
        return None
    # the grid: steps on the generator's cells, outputs where the caller asked for them
    grid = timegrid.build(timegrid.ts_to_host(ts), solver.dt)
    steps = K.solve_steps(grid, bm)
    if steps is None or (need_boundaries and not steps.on_boundaries):
        return None
    schedule = steps.schedule(y0.device, y0.dtype)
    key = ledger.key(found, y0, "kernels", *tag, *(("autograd",) if differentiable else ()))
    verdict, reverify = ledger.verdict(key)
    if verdict is not None and verdict is not True:
        return None
    if verdict is None:
        # the verifying solve: a second interpretation on a probe of another height must find the same nets over the same
        # tensors, and the calls must leave the object's Python-side state and the random generators alone
        snapshot = ledger.snapshot(y0.device)
        if snapshot[0] is None:
            return None
        try:
            again = recognise.recognise(sde, ts[0], y0, differentiable=differentiable, rows=5).deep_spec(sde.noise_type)
        except recognise.NotElementwise as e:
            return ledger.refuse(str(e))
        same = again[3:] == spec[3:] and all(
            a.structure() == b.structure() and all(x is y for x, y in zip(a.parameters(), b.parameters()))
            for a, b in zip(again[1:3], spec[1:3]))
        if not same:
            ledger.file(key, "two interpretations of the same code (probes of 2 and 5 rows) found different networks",
                        reverify)
            return None
        side_effect = ledger.side_effect(snapshot, y0.device)
        if side_effect is not None:
            return ledger.refuse(side_effect)
    route = Route(solver, spec, schedule, np.ascontiguousarray(grid.t, dtype=np.float32), ledger, key, verdict is True,
                  reverify)
    route.cells, route.out_steps = steps.cells, steps.out_step
    return route


def plan_adjoint(solver, sde, y0, ts, bm, dt, adjoint_params):
    """The `Route` of ``sdeint_adjoint(method="reversible_heun", adjoint_method="adjoint_reversible_heun")`` on the kernels, or
    None: as `plan`, and the gradients asked for must be exactly those of the two nets' tensors (a narrower or wider
    `adjoint_params` is the stepwise adjoint's business), every output on a step boundary, the backward grids the forward
    cells walked backwards."""
    route = plan(solver, y0, ts, differentiable=True, need_boundaries=True, tag=("adjoint",))
    if route is None:
        return None
    wanted = {id(p) for p in adjoint_params}
    held = {id(p) for p in route.parameters() if p.requires_grad}
    if wanted != held:
        return None
    # (`bm` is the caller's object, kept for the call site: it may be a BrownianPath / BrownianTree around the interval that
    #  `plan` has just required `solver._native_bm()` to be, and only that interval has cells to walk)
    if K.backward_step_sizes(solver._native_bm(), timegrid.ts_to_host(ts), dt, route.cells, route.out_steps) is None:
        return None
    return route
