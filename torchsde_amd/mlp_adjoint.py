"""``sdeint_adjoint`` on the perceptron-drift module (closed_form.MLPDriftDiagonalSDE) through the matrix-core kernels.

What the reference computes for ``sdeint_adjoint(sde, y0, ts, method=..., adjoint_method="euler")`` on a diagonal-noise
SDE (torchsde/_core/adjoint.py:31-127 + adjoint_sde.py:177-230, 296-323 + methods/euler.py:29-37): a forward solve that
keeps only the states at the output times, and a backward Euler-Maruyama solve of the augmented state (y, a_y, a_theta)
on the same Brownian path, y reset to the stored state and the output's cotangent added to a_y at every output time
(adjoint.py:114-116). Here the forward solve is one launch of the sampling kernel (``tsde_trajectory_mlp_diag``) and
the backward solve is ``tsde_adjoint_mlp_diag`` -- y reconstructed and a_y advanced in registers, four matrix products
per step on the MFMA units -- per chunk of steps, each followed by the two tall-K weight-gradient products
(``tsde_gram_partials``) over that chunk's stash. Memory: the outputs plus O(chunk) stash, independent of the step
count. Same Brownian path and the same arithmetic structure as the stepwise adjoint (adjoint.py), which remains the
route for every other module, method and grid, and the parity reference for this one (tests/test_gpu_mlp_adjoint.py).

``logqp=True`` (the KL column of the latent-SDE training pattern, base_sde.py:240-306) takes the KL instantiations of the same
two kernels (``tsde_trajectory_mlp_diag_logqp``, ``tsde_adjoint_mlp_diag_logqp``) when the prior drift is per-channel affine
in y and does not read t: `plan_logqp`, `_MlpLogqpAdjointFn`. The row sum of the column is an f32 sum in the kernel's own
order, so this route agrees with the stepwise one to rounding, not bit for bit.

``sdeint(..., logqp=True)`` on the same module takes the same sampling kernel and, under autograd, the KL instantiation of
the reverse sweep (``tsde_trajectory_mlp_diag_logqp_backward``, `kernels._MlpLogqpTrajectoryFn`): `plan_logqp_sdeint`,
`LogqpSdeintRoute`. What the two planners share is `_logqp_frame`.
"""
import torch

from . import _native
from . import closed_form
from . import kernels as K
from . import timegrid
from .brownian import BrownianInterval
from .settings import METHOD_OPTIONS, METHODS, SDE_TYPES

# forward methods the sampling kernel has. (Backward: Euler-Maruyama is an Ito scheme -- the reference rejects it for a
# Stratonovich adjoint SDE, adjoint.py:83-93, and `_check_adjoint_method` has already done the same -- Milstein steps
# exist for both SDE types.)
_FORWARD_CODES = {
    (METHODS.euler, SDE_TYPES.ito): _native.TRAJ_EULER,
    (METHODS.milstein, SDE_TYPES.ito): _native.TRAJ_MILSTEIN_ITO,
    (METHODS.milstein, SDE_TYPES.stratonovich): _native.TRAJ_MILSTEIN_STRAT,
    (METHODS.midpoint, SDE_TYPES.stratonovich): _native.TRAJ_MIDPOINT,
    (METHODS.srk, SDE_TYPES.ito): _native.TRAJ_SRK,        # the reference's default for diagonal Ito noise
}
_BACKWARD_KINDS = {METHODS.euler: "euler", METHODS.milstein: "milstein"}


def adjoint_mlp_diag(y, a, stashes, row_rate, row_shift, w1, b1, w2, b2, rate, shift, diffusion, activation, ito,
                     schedule, k_lo, k_hi, bm, milstein=False):
    """One launch of ``tsde_adjoint_mlp_diag`` over steps k_hi-1 ... k_lo (y, a updated in place)."""
    stash_a, stash_hid, stash_delta, stash_y = stashes
    rows, d = y.shape
    lib, dt_code, stream = K._launch_env(y)
    code = lib.tsde_adjoint_mlp_diag(
        y.data_ptr(), a.data_ptr(), stash_a.data_ptr(), stash_hid.data_ptr(), stash_delta.data_ptr(), stash_y.data_ptr(),
        row_rate.data_ptr(), row_shift.data_ptr(), rows, d, b1.numel(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
        b2.data_ptr(), rate.data_ptr(), shift.data_ptr(), int(diffusion[0]), float(diffusion[1]), int(activation),
        (1 if ito else 0) | (2 if milstein else 0), *_native.sweep_tail(schedule, k_lo, k_hi, bm, dt_code, stream))
    _native.check(code, "tsde_adjoint_mlp_diag")


def trajectory_mlp_diag_logqp(ys, logqp, y0, w1, b1, w2, b2, rate, shift, prior_rate, prior_shift, activation, diffusion,
                              method, schedule, bm):
    """One launch of ``tsde_trajectory_mlp_diag_logqp``: ys (n_out, rows, d) and the KL column logqp (n_out, rows), the
    increments from the (rows, d + 1) field of `bm`."""
    tensors = (ys, logqp, y0, w1, b1, w2, b2, rate, shift, prior_rate, prior_shift)
    _native.require_device(*tensors)
    rows, d = y0.shape
    hidden = b1.numel()
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        raise ValueError("the perceptron-drift kernel takes contiguous float32 tensors")
    if (w1.shape != (d, hidden) or w2.shape != (hidden, d) or b2.numel() != d or ys.shape != (schedule.n_out, rows, d)
            or logqp.shape != (schedule.n_out, rows) or any(t.numel() != d for t in (rate, shift, prior_rate, prior_shift))):
        raise ValueError("shape mismatch: w1 (d, hidden), w2 (hidden, d), ys (n_out, rows, d), logqp (n_out, rows)")
    lib, dt_code, stream = K._launch_env(y0)
    code = lib.tsde_trajectory_mlp_diag_logqp(
        ys.data_ptr(), logqp.data_ptr(), y0.data_ptr(), rows, d, hidden, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
        b2.data_ptr(), rate.data_ptr(), shift.data_ptr(), prior_rate.data_ptr(), prior_shift.data_ptr(), int(diffusion[0]),
        float(diffusion[1]), int(activation), int(method), *_native.trajectory_tail(schedule, bm, dt_code, stream))
    _native.check(code, "tsde_trajectory_mlp_diag_logqp")


def adjoint_mlp_diag_logqp(y, a, a_l, stashes, row_sums, w1, b1, w2, b2, rate, shift, prior_rate, prior_shift, diffusion,
                           activation, schedule, k_lo, k_hi, bm, milstein=False):
    """One launch of ``tsde_adjoint_mlp_diag_logqp`` over steps k_hi-1 ... k_lo (y, a updated in place; a_l, the cotangent of
    the KL column, read). `row_sums`: (row_rate, row_shift, row_prior_rate, row_prior_shift)."""
    stash_a, stash_hid, stash_delta, stash_y = stashes
    rows, d = y.shape
    lib, dt_code, stream = K._launch_env(y)
    code = lib.tsde_adjoint_mlp_diag_logqp(
        y.data_ptr(), a.data_ptr(), a_l.data_ptr(), stash_a.data_ptr(), stash_hid.data_ptr(), stash_delta.data_ptr(),
        stash_y.data_ptr(), *(t.data_ptr() for t in row_sums), rows, d, b1.numel(), w1.data_ptr(), b1.data_ptr(),
        w2.data_ptr(), b2.data_ptr(), rate.data_ptr(), shift.data_ptr(), prior_rate.data_ptr(), prior_shift.data_ptr(),
        int(diffusion[0]), float(diffusion[1]), int(activation), 1 | (2 if milstein else 0),
        *_native.sweep_tail(schedule, k_lo, k_hi, bm, dt_code, stream))
    _native.check(code, "tsde_adjoint_mlp_diag_logqp")


class _MlpAdjointFn(torch.autograd.Function):
    """Forward: the sampling kernel, outputs only. Backward: the stochastic adjoint (Euler or Milstein steps) on the
    matrix cores."""

    STASH_BYTES = 3 << 30      # per-chunk stash of the backward sweep (four (steps, rows, width) float32 arrays)

    @staticmethod
    def _chunk(n_steps, rows, d, hidden):
        return K.PerceptronGradients.chunk_length(n_steps, rows, 2 * d + 2 * hidden, _MlpAdjointFn.STASH_BYTES)

    @staticmethod
    def forward(ctx, activation, diffusion, method_code, ito, backward_kind, schedule, backward_schedule, out_steps, bm,
                y0, w1, b1, w2, b2, rate, shift):
        rows, d = y0.shape
        y0c = _native.contiguous(y0.detach())
        net = K.PerceptronGradients.prepare(d, w1, b1, w2, b2, rate, shift)
        ys = torch.empty((len(out_steps) + 1, rows, d), dtype=y0.dtype, device=y0.device)
        ys[0].copy_(y0c)
        K.trajectory_mlp_diag(ys[1:], y0c, *net, activation, diffusion, method_code, schedule, bm)
        ctx.save_for_backward(ys, *net)
        ctx.activation, ctx.diffusion, ctx.ito = int(activation), (int(diffusion[0]), float(diffusion[1])), bool(ito)
        ctx.backward_kind = backward_kind
        ctx.schedule, ctx.bm, ctx.out_steps = backward_schedule, bm, tuple(out_steps)
        ctx.param_shapes = (tuple(rate.shape), tuple(shift.shape))
        ctx.generic = None
        return ys

    @staticmethod
    def backward(ctx, gys):
        if torch.is_grad_enabled():    # create_graph=True: the kernels below leave no graph; see adjoint_double.py
            return _MlpAdjointFn._backward_with_graph(ctx, gys)
        ys, w1_in, b1c, w2_in, b2c, rate, shift = ctx.saved_tensors
        rows, d = ys.shape[1], ys.shape[2]
        hidden = b1c.numel()
        dev = ys.device
        gys = _native.contiguous(gys)
        chunk = _MlpAdjointFn._chunk(ctx.schedule.n_steps, rows, d, hidden)
        sums = K.PerceptronGradients(rows, d, hidden, dev)
        stashes = sums.stashes(chunk, (d, hidden, hidden, d))
        row_rate = torch.zeros((rows, d), dtype=torch.float32, device=dev)
        row_shift = torch.zeros_like(row_rate)
        boundaries = (0,) + ctx.out_steps                   # step boundary of output i
        y = ys[-1].clone()
        a = gys[-1].clone()
        for i in range(len(boundaries) - 1, 0, -1):
            for k_hi in range(boundaries[i], boundaries[i - 1], -chunk):
                k_lo = max(boundaries[i - 1], k_hi - chunk)
                adjoint_mlp_diag(y, a, stashes, row_rate, row_shift, w1_in, b1c, w2_in, b2c, rate, shift, ctx.diffusion,
                                 ctx.activation, ctx.ito, ctx.schedule, k_lo, k_hi, ctx.bm,
                                 milstein=ctx.backward_kind == "milstein")
                sums.accumulate(k_hi - k_lo, *stashes)
            # adjoint.py:114-116: the forward state is known again at an output time; its cotangent joins a_y
            y.copy_(ys[i - 1])
            a += gys[i - 1]
        diffusion = K.PerceptronGradients.diffusion_gradients((row_rate, row_shift), ctx.param_shapes)
        grad_y0 = a if ctx.needs_input_grad[9] else None
        return (None,) * 9 + (grad_y0, sums.g_w1, sums.g_b1, sums.g_w2, sums.g_b2, *diffusion)

    @staticmethod
    def _backward_with_graph(ctx, gys):
        from . import adjoint, adjoint_double
        if ctx.generic is None:
            raise NotImplementedError("torchsde_amd: no differentiable backward pass was prepared for this call.")
        sde, ts_host, dt, own = ctx.generic
        ys = ctx.saved_tensors[0]
        params = [p for p in own if p.requires_grad]
        with _native.on_device_of(ys):
            plan = adjoint._plan_backward(ts_host, dt, ctx.bm, ys.device)
            a_y, a_theta = adjoint_double.run(adjoint.AdjointSDE(sde, params), ctx.backward_kind, ctx.bm, plan, ys, gys)
        a_theta = iter(a_theta)
        grads = [next(a_theta) if p.requires_grad else None for p in own]
        return (None,) * 9 + (a_y if ctx.needs_input_grad[9] else None, *grads)


class _MlpLogqpAdjointFn(torch.autograd.Function):
    """`_MlpAdjointFn` for ``logqp=True``: the state has the KL column l as its last column (contract.check_contract), the
    prior drift is h = hr * y + hs. Forward: the KL instantiation of the sampling kernel. Backward: that of the adjoint
    kernel, with a_l -- the cotangent of the column, constant between outputs -- carried through the output loop.

    Inputs after `y0`: the module's six perceptron / diffusion tensors; `hr_t`, `hs_t`, which carry the user's graph from the
    prior's own parameters (recognise.prior_coefficient_graph) and receive dL/dhr, dL/dhs; the coefficient VALUES the kernels
    take (detached); then the prior's parameters themselves, which receive a gradient only from a backward pass that builds
    a graph (``create_graph=True``: adjoint_double differentiates the user's code directly, and hr_t, hs_t get none)."""

    N_PLAIN = 8                # arguments before y0

    @staticmethod
    def forward(ctx, activation, diffusion, method_code, backward_kind, schedule, backward_schedule, out_steps, bm, y0, w1,
                b1, w2, b2, rate, shift, hr_t, hs_t, hr, hs, *prior_params):
        rows, d = y0.shape[0], y0.shape[1] - 1
        y0d = y0.detach()
        net = K.PerceptronGradients.prepare(d, w1, b1, w2, b2, rate, shift)
        states = torch.empty((len(out_steps) + 1, rows, d), dtype=y0.dtype, device=y0.device)
        states[0].copy_(y0d[:, :d])
        column = torch.empty((len(out_steps), rows), dtype=y0.dtype, device=y0.device)
        trajectory_mlp_diag_logqp(states[1:], column, states[0], *net, hr, hs, activation, diffusion, method_code, schedule,
                                  bm)
        ys = torch.empty((len(out_steps) + 1, rows, d + 1), dtype=y0.dtype, device=y0.device)
        ys[:, :, :d].copy_(states)
        ys[0, :, d].copy_(y0d[:, d])
        torch.add(column, y0d[:, d], out=ys[1:, :, d])
        ctx.save_for_backward(states, *net, hr, hs, ys)
        ctx.activation, ctx.diffusion = int(activation), (int(diffusion[0]), float(diffusion[1]))
        ctx.backward_kind = backward_kind
        ctx.schedule, ctx.bm, ctx.out_steps = backward_schedule, bm, tuple(out_steps)
        ctx.param_shapes = (tuple(rate.shape), tuple(shift.shape))
        ctx.n_prior = len(prior_params)
        ctx.generic = None
        return ys

    @staticmethod
    def backward(ctx, gys):
        if torch.is_grad_enabled():
            return _MlpLogqpAdjointFn._backward_with_graph(ctx, gys)
        states, w1_in, b1c, w2_in, b2c, rate, shift, hr, hs, _ = ctx.saved_tensors
        rows, d = states.shape[1], states.shape[2]
        hidden = b1c.numel()
        dev = states.device
        g_state = gys[:, :, :d].contiguous()
        g_column = gys[:, :, d].contiguous()
        chunk = _MlpAdjointFn._chunk(ctx.schedule.n_steps, rows, d, hidden)
        sums = K.PerceptronGradients(rows, d, hidden, dev)
        stashes = sums.stashes(chunk, (d, hidden, hidden, d))
        row_sums = tuple(torch.zeros((rows, d), dtype=torch.float32, device=dev) for _ in range(4))
        boundaries = (0,) + ctx.out_steps
        y = states[-1].clone()
        a = g_state[-1].clone()
        a_l = g_column[-1].clone()
        for i in range(len(boundaries) - 1, 0, -1):
            for k_hi in range(boundaries[i], boundaries[i - 1], -chunk):
                k_lo = max(boundaries[i - 1], k_hi - chunk)
                adjoint_mlp_diag_logqp(y, a, a_l, stashes, row_sums, w1_in, b1c, w2_in, b2c, rate, shift, hr, hs,
                                       ctx.diffusion, ctx.activation, ctx.schedule, k_lo, k_hi, ctx.bm,
                                       milstein=ctx.backward_kind == "milstein")
                sums.accumulate(k_hi - k_lo, *stashes)
            # adjoint.py:114-116, for the state and for the column alike
            y.copy_(states[i - 1])
            a += g_state[i - 1]
            a_l += g_column[i - 1]
        diffusion = K.PerceptronGradients.diffusion_gradients(row_sums[:2], ctx.param_shapes)
        grad_y0 = torch.cat((a, a_l.unsqueeze(1)), dim=1) if ctx.needs_input_grad[_MlpLogqpAdjointFn.N_PLAIN] else None
        return ((None,) * _MlpLogqpAdjointFn.N_PLAIN
                + (grad_y0, sums.g_w1, sums.g_b1, sums.g_w2, sums.g_b2, *diffusion, row_sums[2].sum(dim=0),
                   row_sums[3].sum(dim=0), None, None) + (None,) * ctx.n_prior)

    @staticmethod
    def _backward_with_graph(ctx, gys):
        from . import adjoint, adjoint_double
        if ctx.generic is None:
            raise NotImplementedError("torchsde_amd: no differentiable backward pass was prepared for this call.")
        sde, ts_host, dt, own = ctx.generic          # own: the six tensors, then the prior's parameters
        ys = ctx.saved_tensors[-1]
        params = [p for p in own if p.requires_grad]
        with _native.on_device_of(ys):
            plan = adjoint._plan_backward(ts_host, dt, ctx.bm, ys.device)
            a_y, a_theta = adjoint_double.run(adjoint.AdjointSDE(sde, params), ctx.backward_kind, ctx.bm, plan, ys, gys)
        a_theta = iter(a_theta)
        grads = [next(a_theta) if p.requires_grad else None for p in own]
        return ((None,) * _MlpLogqpAdjointFn.N_PLAIN
                + (a_y if ctx.needs_input_grad[_MlpLogqpAdjointFn.N_PLAIN] else None, *grads[:6], None, None, None, None,
                   *grads[6:]))


class LogqpRoute:
    """One ``sdeint_adjoint(..., logqp=True)`` call's plan on the KL kernels (`plan_logqp`): `solve(y0)` launches it,
    `record(fast, stepwise, y0)` files the verdict of a verifying solve (the interface of neural_rheun_route.Route)."""

    def __init__(self, solver, args, own, prior_params, generic, ledger, key, trusted, reverify):
        self.solver, self.args, self.own, self.prior_params, self.generic = solver, args, own, prior_params, generic
        self.ledger, self.key, self.trusted, self.reverify = ledger, key, trusted, reverify

    def solve(self, y0, z_holder=None):
        from . import recognise
        inner, t0, d, hr, hs = self.prior
        hr_t, hs_t = recognise.prior_coefficient_graph(inner.h, t0, d, y0.dtype, y0.device)
        ys = _MlpLogqpAdjointFn.apply(*self.args, y0, *self.own, hr_t, hs_t, hr, hs, *self.prior_params)
        if ys.grad_fn is not None:
            ys.grad_fn.generic = self.generic
        return ys

    def record(self, fast, stepwise, y0, extra_inputs=()):
        verdict = self.solver._both_routes_agree(fast, stepwise, y0, "the KL perceptron kernels", network=True,
                                                 extra_inputs=extra_inputs)
        self.ledger.file(self.key, verdict, self.reverify)
        if verdict is True:
            self.ledger.name_kernel(self.key, "tsde_trajectory_mlp_diag_logqp + tsde_adjoint_mlp_diag_logqp")
        return verdict


class _LogqpFrame:
    """What `plan_logqp` (``sdeint_adjoint``) and `plan_logqp_sdeint` (``sdeint``) both need of a ``logqp=True`` call on the
    perceptron-drift module: the unwrapped module, its interpretation (`found`, `spec`, `own`: the six tensors), the prior's
    coefficients (`hr`, `hs`), the module's other trainable parameters (`prior_params`), the ledger, and grid and steps."""

    def shape_of(self, c):
        return "number" if isinstance(c, (bool, int, float)) else tuple(c.shape)

    def prior_vectors(self, y0):
        from . import recognise
        return (recognise.prior_vector(self.hr, self.d, y0.dtype, y0.device),
                recognise.prior_vector(self.hs, self.d, y0.dtype, y0.device))

    def verdict(self, key, y0):
        """(verdict, reverify) of this solve of `key`, or None where the route declines: a form that was refused, or -- ahead
        of a verifying solve -- a stream capture, a second interpretation on a probe of another height that finds other forms
        or other tensors, calls that touch the object's Python-side state or a random generator."""
        from . import recognise
        ledger, d = self.ledger, self.d
        verdict, reverify = ledger.verdict(key)
        if verdict is not None and verdict is not True:
            return None
        if verdict is None:
            if torch.cuda.is_current_stream_capturing():
                return None
            snapshot = ledger.snapshot(y0.device)
            if snapshot[0] is None:
                return None
            try:
                again, again_spec, (hr5, hs5) = self.interpret(rows=5)
            except recognise.NotElementwise as e:
                return ledger.refuse(str(e))
            own5 = again.perceptron_parameters()
            same = (again.structure() == self.found.structure() and again_spec[-2:] == self.spec[-2:] and own5 is not None
                    and all(x is y or (not x.requires_grad and torch.equal(x, y)) for x, y in zip(own5, self.own))
                    and all(self.shape_of(x) == self.shape_of(y)
                            and bool((recognise.prior_vector(x, d, y0.dtype, y0.device)
                                      == recognise.prior_vector(y, d, y0.dtype, y0.device)).all())
                            for x, y in ((self.hr, hr5), (self.hs, hs5))))
            if not same:
                ledger.file(key, "two interpretations of the same code (probes of 2 and 5 rows) found different forms", reverify)
                return None
            side_effect = ledger.side_effect(snapshot, y0.device)
            if side_effect is not None:
                return ledger.refuse(side_effect)
        return verdict, reverify


def _logqp_frame(sde, y0, ts, bm, dt, solver):
    """The `_LogqpFrame` of a ``logqp=True`` call, or None where no KL kernel can take it. `sde` is
    ``ForwardSDE(SDELogqp([RenameMethodsSDE(] module [)]))`` and `y0` carries the extra column (contract.check_contract).
    Conditions: an Ito SDE with diagonal noise, drift ``lin2(act(lin1(y)))``, affine or sigmoid elementwise diffusion, the shape
    limits, this package's BrownianInterval in float32 with d + 1 columns, a fixed-step grid on its cells, a prior drift that
    is per-channel affine in y and does not read t (recognise.recognise_prior)."""
    from . import recognise, trust
    from .sde import ForwardSDE, RenameMethodsSDE, SDELogqp
    from .settings import NOISE_TYPES
    wrapped = getattr(sde, "_base_sde", None)
    if (type(sde) is not ForwardSDE or type(wrapped) is not SDELogqp or sde.sde_type != SDE_TYPES.ito
            or sde.noise_type != NOISE_TYPES.diagonal or sde.user_product):
        return None
    inner = wrapped._base_sde
    module = inner._base_sde if type(inner) is RenameMethodsSDE else inner
    if not isinstance(module, torch.nn.Module) or hasattr(module, "_base_sde") or not hasattr(inner, "h"):
        return None
    if (not isinstance(bm, BrownianInterval) or bm._rootW is not None or bm._rootH is not None or bm._snap or y0.dim() != 2
            or not y0.is_cuda or y0.shape[1] < 2 or tuple(bm.shape) != tuple(y0.shape) or y0.dtype != torch.float32
            or bm.dtype != torch.float32 or ts.dtype != y0.dtype or y0.numel() == 0):
        return None
    d = y0.shape[1] - 1
    ledger = trust.open_book(solver, who=type(solver).__name__ + ":KL perceptron kernels")
    if ledger is None or ledger.refused():
        return None
    state = y0.detach()[:, :d]
    inner_forward = ForwardSDE(inner)
    if inner_forward.user_product:
        return None

    def interpret(rows=None):
        found = recognise.recognise(inner_forward, ts[0], state, differentiable=True, rows=rows)
        if not found.perceptron:
            raise recognise.NotElementwise("the drift is not a two-layer perceptron of y beside an elementwise diffusion")
        return found, found.perceptron_spec(), recognise.recognise_prior(inner.h, ts[0], state, differentiable=True, rows=rows)

    try:
        found, spec, (hr, hs) = interpret()
    except recognise.NotElementwise as e:
        return ledger.refuse(str(e))
    own = found.perceptron_parameters()
    if own is None:
        return None
    hidden = own[1].numel()
    # gradients go to exactly the module's trainable parameters: the six tensors of drift and diffusion, and whatever else
    # the module holds -- which can only reach the solve through the prior (f and g are the recognised forms over `own`)
    module_params = list(module.parameters())
    module_ids = {id(p) for p in module_params}
    own_ids = {id(p) for p in own}
    if (any(p.requires_grad and id(p) not in module_ids for p in own)
            or hidden % 4 != 0 or y0.shape[0] * (max(d, hidden) + 1) >= 2 ** 30):
        return None
    ts_host = timegrid.ts_to_host(ts)
    grid = timegrid.build(ts_host, dt)
    if grid.n_steps == 0:
        return None
    steps = K.solve_steps(grid, bm)
    if steps is None:
        return None
    frame = _LogqpFrame()
    frame.inner, frame.module, frame.d, frame.hidden, frame.ledger, frame.interpret = inner, module, d, hidden, ledger, interpret
    frame.found, frame.spec, frame.own, frame.hr, frame.hs = found, spec, own, hr, hs
    frame.module_params = module_params
    frame.prior_params = [p for p in module_params if id(p) not in own_ids and p.requires_grad]
    frame.ts_host, frame.grid, frame.steps, frame.t0 = ts_host, grid, steps, ts[0]
    return frame


def plan_logqp(sde, y0, ts, bm, method, adjoint_method, dt, adaptive, adjoint_adaptive, options, adjoint_options,
               adjoint_params, extra_solver_state, solver):
    """The `LogqpRoute` of ``sdeint_adjoint(sde, y0, ts, logqp=True)`` if the call can take the KL kernels, else None (it stays
    on the stepwise stochastic adjoint). Conditions: everything `_logqp_frame` asks, Euler or Milstein both ways, outputs on
    step boundaries, `adjoint_params` exactly the module's trainable parameters. `solver.recognised_perceptron`
    cannot verify this call (its forward solve has a (B, d) state against a (B, d + 1) Brownian motion), so trust is earned
    here as on the reversible-Heun route: the first solve of a (form, batch size, "logqp") on an SDE object runs BOTH routes,
    returns the stepwise result and files the verdict of `solvers._both_routes_agree` -- values of ys and of the column,
    gradients for y0 and every parameter. TSDE_VERIFY_EVERY applies; no verifying solve runs under stream capture."""
    from . import recognise
    if (adaptive or adjoint_adaptive or extra_solver_state is not None or adjoint_method not in _BACKWARD_KINDS
            or method not in (METHODS.euler, METHODS.milstein)
            or adjoint_options.get(METHOD_OPTIONS.grad_free, False) or options.get(METHOD_OPTIONS.grad_free, False)
            or not options.get("trajectory_kernel", True) or not adjoint_options.get("trajectory_kernel", True)
            or not recognise.ENABLED or solver is None):
        return None
    frame = _logqp_frame(sde, y0, ts, bm, dt, solver)
    if frame is None:
        return None
    code = _FORWARD_CODES[(method, SDE_TYPES.ito)]
    if {id(p) for p in adjoint_params} != {id(p) for p in frame.module_params if p.requires_grad}:
        return None
    # ---- grids: every output on a forward step boundary, every backward step exactly one forward cell ------------------
    steps = frame.steps
    if any(not (w0 == 0.0 and w1 == 1.0) for (_, _, w0, w1) in frame.grid.outputs):
        return None
    backward_dt = K.backward_step_sizes(bm, frame.ts_host, dt, steps.cells, steps.out_step)
    if backward_dt is None:
        return None
    ledger, spec, own = frame.ledger, frame.spec, frame.own
    key = ledger.key(frame.found, y0, "logqp", method, adjoint_method, frame.shape_of(frame.hr), frame.shape_of(frame.hs))
    decided = frame.verdict(key, y0)
    if decided is None:
        return None
    verdict, reverify = decided
    schedule = steps.schedule(y0.device, y0.dtype)
    backward_schedule = steps.schedule(y0.device, y0.dtype, dt=backward_dt)
    args = (spec[-2], tuple(spec[-1]), code, _BACKWARD_KINDS[adjoint_method], schedule, backward_schedule,
            tuple(int(k) for k in steps.out_step), bm)
    plan = LogqpRoute(solver, args, own, frame.prior_params, (sde, frame.ts_host, dt, list(own) + frame.prior_params), ledger,
                      key, verdict is True, reverify)
    plan.prior = (frame.inner, frame.t0, frame.d) + frame.prior_vectors(y0)
    return plan


class LogqpSdeintRoute:
    """One ``sdeint(..., logqp=True)`` call's plan on the KL kernels (`plan_logqp_sdeint`), the interface of `LogqpRoute`.
    With autograd recording: `kernels._MlpLogqpTrajectoryFn` (the KL sampling kernel at every step and at the outputs inside
    steps, then the KL reverse sweep); without: one launch of the KL sampling kernel."""

    def __init__(self, solver, frame, args, recording, ledger, key, trusted, reverify):
        self.solver, self.frame, self.args, self.recording = solver, frame, args, recording
        self.ledger, self.key, self.trusted, self.reverify = ledger, key, trusted, reverify

    def solve(self, y0, z_holder=None):
        from . import recognise
        frame = self.frame
        hr, hs = frame.prior_vectors(y0)
        if self.recording:
            hr_t, hs_t = recognise.prior_coefficient_graph(frame.inner.h, frame.t0, frame.d, y0.dtype, y0.device)
            return K._MlpLogqpTrajectoryFn.apply(*self.args, y0, *frame.own, hr_t, hs_t, hr, hs)
        activation, diffusion, code, schedule, bm = self.args
        rows, d = y0.shape[0], frame.d
        y0d = y0.detach()
        net = K.PerceptronGradients.prepare(d, *frame.own)
        states = torch.empty((schedule.n_out + 1, rows, d), dtype=y0.dtype, device=y0.device)
        states[0].copy_(y0d[:, :d])
        column = torch.empty((schedule.n_out, rows), dtype=y0.dtype, device=y0.device)
        trajectory_mlp_diag_logqp(states[1:], column, states[0], *net, hr, hs, activation, diffusion, code, schedule, bm)
        return K.assemble_logqp_output(states, column, y0d[:, d])

    def record(self, fast, stepwise, y0, extra_inputs=()):
        what = "the KL perceptron kernels" + (" (back-propagation)" if self.recording else " (sampling)")
        verdict = self.solver._both_routes_agree(fast, stepwise, y0, what, network=True, extra_inputs=extra_inputs)
        self.ledger.file(self.key, verdict, self.reverify)
        if verdict is True:
            weighted = "_weighted (outputs inside steps)" if "interpolated outputs" in self.key else ""
            self.ledger.name_kernel(self.key, "tsde_trajectory_mlp_diag_logqp + tsde_trajectory_mlp_diag_logqp_backward" + weighted
                                    if self.recording else "tsde_trajectory_mlp_diag_logqp")
        return verdict


def _leaves_reached(tensors):
    """ids of the leaf tensors the autograd graphs of `tensors` reach."""
    reached, seen = set(), set()
    stack = [t.grad_fn for t in tensors]
    reached.update(id(t) for t in tensors if t.is_leaf)
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)                                     # (the node itself: the id of a collected wrapper is used again)
        if hasattr(fn, "variable"):
            reached.add(id(fn.variable))
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return reached


def plan_logqp_sdeint(sde, y0, ts, bm, method, dt, adaptive, options, extra, extra_solver_state, solver):
    """The `LogqpSdeintRoute` of ``sdeint(sde, y0, ts, logqp=True)`` if the call can take the KL kernels, else None (it stays
    on the stepwise solver). Conditions: everything `_logqp_frame` asks; Euler, or Milstein with the affine diffusion when
    autograd records (the reverse sweep has no sigmoid Milstein terms); no `adaptive`, `extra`, given `extra_solver_state`,
    ``options={"hip_graph": True}`` or ``options={"trajectory_kernel": False}``. With autograd recording (`y0` or a parameter
    of the module requires a gradient) every trainable parameter of the module must be one of the six tensors or reached by
    the prior's coefficients: `kernels._MlpLogqpTrajectoryFn`. Outputs inside steps are interpolated by the sampling kernel
    either way; under autograd the reverse sweep splits their cotangents by the interpolation weights. Trust as in
    `plan_logqp`, on keys of its own (..., "logqp", "backprop" | "sampling", ["interpolated outputs",] ...): the first solve of
    a key runs both routes and returns the stepwise result -- a grid that interpolates an output under autograd has a key of
    its own, so trust earned on an aligned grid does not cover it; TSDE_VERIFY_EVERY applies; no verifying solve runs under
    stream capture."""
    from . import graph, recognise
    if (adaptive or extra or extra_solver_state is not None or method not in (METHODS.euler, METHODS.milstein)
            or options.get(METHOD_OPTIONS.grad_free, False) or not options.get("trajectory_kernel", True)
            or graph.mode_of(options) is True or not recognise.ENABLED or solver is None):
        return None
    frame = _logqp_frame(sde, y0, ts, bm, dt, solver)
    if frame is None:
        return None
    code = _FORWARD_CODES[(method, SDE_TYPES.ito)]
    spec, steps, ledger = frame.spec, frame.steps, frame.ledger
    recording = torch.is_grad_enabled() and (y0.requires_grad or any(p.requires_grad for p in frame.module_params))
    if recording:
        if spec[-1][0] == _native.DIFF_SIGMOID and code != _native.TRAJ_EULER:
            return None
        hr_t, hs_t = recognise.prior_coefficient_graph(frame.inner.h, frame.t0, frame.d, y0.dtype, y0.device)
        reached = _leaves_reached((hr_t, hs_t)) | {id(p) for p in frame.own}
        if any(p.requires_grad and id(p) not in reached for p in frame.module_params):
            return None
    # (a grid that interpolates an output under autograd runs the weighted reverse sweep and the merged forward launch: code
    #  that trust earned on an aligned grid has not seen, so it earns its own)
    interpolates = ("interpolated outputs",) if recording and not steps.on_boundaries else ()
    key = ledger.key(frame.found, y0, "logqp", "backprop" if recording else "sampling", *interpolates, method,
                     frame.shape_of(frame.hr), frame.shape_of(frame.hs))
    decided = frame.verdict(key, y0)
    if decided is None:
        return None
    verdict, reverify = decided
    if recording:
        args = (spec[-2], tuple(spec[-1]), code, steps.schedule(y0.device, y0.dtype, every_step=True),
                K.OutputMap.cached(steps.out_step, steps.out_w), bm)
    else:
        args = (spec[-2], tuple(spec[-1]), code, steps.schedule(y0.device, y0.dtype), bm)
    return LogqpSdeintRoute(solver, frame, args, recording, ledger, key, verdict is True, reverify)


def route(sde, y0, ts, bm, method, adjoint_method, dt, adaptive, adjoint_adaptive, options, adjoint_options,
          adjoint_params, extra_solver_state, solver=None, logqp=False):
    """`ys` with a grad_fn towards y0 and the module's six parameters if this call can take the kernels above, else
    None (the caller then runs the stepwise stochastic adjoint). ``logqp=True`` is `plan_logqp`'s business."""
    from .sde import ForwardSDE
    if logqp:
        return None
    if (adaptive or adjoint_adaptive or extra_solver_state is not None or adjoint_method not in _BACKWARD_KINDS
            or adjoint_options.get(METHOD_OPTIONS.grad_free, False) or options.get(METHOD_OPTIONS.grad_free, False)
            or not options.get("trajectory_kernel", True) or not adjoint_options.get("trajectory_kernel", True)):
        return None
    base = getattr(sde, "_base_sde", None)
    if type(sde) is not ForwardSDE:
        return None
    published = hasattr(base, "closed_form") and closed_form.publishes_its_own_dynamics(base)
    code = _FORWARD_CODES.get((method, sde.sde_type))
    if (code is None or not isinstance(bm, BrownianInterval) or bm._rootW is not None or bm._rootH is not None
            or bm._snap or y0.dim() != 2 or tuple(bm.shape) != tuple(y0.shape) or y0.dtype != torch.float32
            or bm.dtype != torch.float32 or bm._elem0 % 4 != 0 or y0.numel() == 0
            or (code == _native.TRAJ_SRK and not bm._have_H)):
        return None
    if published:
        spec = base.closed_form(y0.shape[1], y0.dtype, y0.device)
        if spec is None or spec[0] != "mlp_diagonal":
            return None
        own = list(base.closed_form_parameters())
    else:
        # an UNCHANGED user module whose drift turns out to be lin2(act(lin1(y))) with an affine / sigmoid diagonal
        # diffusion (recognise.py), its forward solve through the sampling kernel verified against the stepwise one
        if solver is None or not isinstance(base, torch.nn.Module):
            return None
        found = solver.recognised_perceptron(y0, ts)
        if found is None:
            return None
        own = found.perceptron_parameters()
        if own is None:
            return None
        spec = found.perceptron_spec()
    hidden = own[1].numel()
    # gradients go to exactly the module's own trainable parameters: a narrower or wider `adjoint_params` is the
    # stepwise adjoint's business
    module_params = {id(p) for p in base.parameters()}
    if ({id(p) for p in adjoint_params} != {id(p) for p in own if p.requires_grad}
            or module_params != {id(p) for p in own if id(p) in module_params or published}
            or hidden % 4 != 0 or y0.shape[0] * max(y0.shape[1], hidden) >= 2 ** 30):
        return None

    # ---- grids: every output on a forward step boundary, every backward step exactly one forward cell ------------------
    ts_host = timegrid.ts_to_host(ts)
    grid = timegrid.build(ts_host, dt)
    if grid.n_steps == 0 or any(not (w0 == 0.0 and w1 == 1.0) for (_, _, w0, w1) in grid.outputs):
        return None
    steps = K.solve_steps(grid, bm)
    if steps is None:
        return None
    # (it is the backward solver's step sizes the backward kernel is given)
    backward_dt = K.backward_step_sizes(bm, ts_host, dt, steps.cells, steps.out_step)
    if backward_dt is None:
        return None
    schedule = steps.schedule(y0.device, y0.dtype)
    backward_schedule = steps.schedule(y0.device, y0.dtype, dt=backward_dt)
    ys = _MlpAdjointFn.apply(spec[-2], tuple(spec[-1]), code, sde.sde_type == SDE_TYPES.ito,
                             _BACKWARD_KINDS[adjoint_method], schedule, backward_schedule,
                             tuple(int(k) for k in steps.out_step), bm, y0, *own)
    if ys.grad_fn is not None:           # what a second-order backward pass needs (`ys.grad_fn` is the Function's ctx)
        ys.grad_fn.generic = (sde, ts_host, dt, own)
    return ys
