"""Cases, reference and solves of ``sdeint(..., logqp=True)`` on the KL perceptron kernels (tests/test_gpu_mlp_logqp_backprop.py,
tools/mlp_logqp_backprop_rounding_ratios.py; the route is torchsde_amd/mlp_adjoint.plan_logqp_sdeint, the autograd function
torchsde_amd/kernels._MlpLogqpTrajectoryFn).

Modules, `Case`, cotangents and the comparison are those of tests/helpers_logqp.py. The reference is autograd THROUGH the oracle's
stepwise solver over `LogqpRef` (oracle/solvers_ref.py) -- back-propagation through the solver, what ``loss.backward()`` gives on
the reference -- on the same counter path (a Brownian motion of d + 1 columns), in float32 and float64."""
import copy

import numpy as np
import torch

from tests import helpers
from tests import helpers_logqp as L

F32, F64 = L.F32, L.F64
DT, STEPS, OUTPUTS = L.DT, L.STEPS, L.OUTPUTS
SHAPES = L.SHAPES
# method, (unused: the adjoint method of helpers_logqp.Case), diffusion: the reverse sweep has no sigmoid Milstein terms
SCHEMES = (("euler", None, "sigmoid"), ("euler", None, "affine"), ("milstein", None, "affine"))
FIRST_INDEX = 40
# The kernels' result may differ from the float64 oracle by BACKPROP_FACTOR times the float32 oracle's own difference from it,
# plus BACKPROP_FLOOR of the quantity's scale: twice the worst ratio measured on an MI355X over every case, cotangent and
# quantity (profiles/mlp_logqp_backprop_rounding_ratios.txt, written by tools/mlp_logqp_backprop_rounding_ratios.py), rounded
# up, and at least 4 -- the rule of helpers.MLP_GRAD_FACTOR. Measured: worst ratio 0.103 over 648 comparisons, so 4.
BACKPROP_FACTOR = 4.0
BACKPROP_FLOOR = 1e-6
FN = "_MlpLogqpTrajectoryFn"


def cases():
    out = []
    for scheme in SCHEMES:
        for shape in SHAPES:
            out.append(L.Case(FIRST_INDEX + len(out), shape, scheme, ("tanh", "softplus")[len(out) % 2]))
    return out


def oracle(case, module=None, names=None, ts=None, gradients=True):
    """``{dtype: {label: {quantity: tensor}}}`` from autograd through the oracle's stepwise solver in float32 and float64,
    plus ``min_g``: the smallest |g| the float64 run meets at its output states. `ts`: other output times than the case's
    (`gradients=False`: values only, under the one label "values")."""
    from oracle import solvers_ref
    module = case.module() if module is None else module
    pnames = [name for name, _ in module.named_parameters()]
    times = case.ts() if ts is None else list(ts)
    edges = helpers.rheun_grid(times, DT).t_f64()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {}
    try:
        for dtype in (F32, F64):
            ref = copy.deepcopy(module).cpu().to(dtype)
            params = list(ref.parameters())
            bm = helpers.counter_rows_bm(np.arange(case.B), case.d + 1, case.entropy, edges, dtype)
            ts_t = torch.tensor(times, dtype=dtype)
            y0 = case.y0().to(dtype).requires_grad_(gradients)
            y0_aug = torch.cat((y0, y0.new_zeros(case.B, 1)), dim=1)
            with torch.set_grad_enabled(gradients):
                ys_aug = solvers_ref.integrate(solvers_ref.LogqpRef(ref, names), bm, y0_aug, ts_t, DT, case.method)
            col = ys_aug[:, :, -1]
            values = {"ys": ys_aug[:, :, :-1].detach(), "log_ratio": (col[1:] - col[:-1]).detach()}
            out[dtype] = {}
            if not gradients:
                out[dtype]["values"] = values
            else:
                for label, wy, wl in case.cotangents():
                    loss = (ys_aug * L.column_cotangent(wy, wl).to(dtype)).sum()
                    grads = torch.autograd.grad(loss, [y0] + params, retain_graph=True, allow_unused=True)
                    grads = [torch.zeros_like(x) if g is None else g.detach() for g, x in zip(grads, [y0] + params)]
                    found = dict(values)
                    found.update(zip(["y0"] + pnames, grads))
                    out[dtype][label] = found
            if dtype == F64:
                with torch.no_grad():
                    g = getattr(ref, (names or {}).get("diffusion", "g"))(ts_t[0], values["ys"].reshape(-1, case.d))
                out["min_g"] = g.abs().min().item()
    finally:
        torch.set_num_threads(threads)
    return out


def call(case, sde, device, y0=None, ts=None, names=None, rows=None, row_offset=0, **kw):
    """One ``sdeint(..., logqp=True)`` of `sde`: (ys, log_ratio, y0)."""
    import torchsde_amd
    if y0 is None:
        y0 = case.y0().to(device).requires_grad_(True)
    ts = torch.tensor(case.ts() if ts is None else list(ts), device=device)
    ys, log_ratio = torchsde_amd.sdeint(sde, y0, ts, bm=L.brownian(case, device, rows=rows, row_offset=row_offset),
                                        method=case.method, dt=DT, logqp=True, names=names, **kw)
    return ys, log_ratio, y0


def solve(case, device, module=None, fast=True, names=None, expect_route=None, solves=2, **kw):
    """`solves` calls of ``sdeint(..., logqp=True)`` under autograd on a copy of the case's module (the first of a form
    verifies and returns the stepwise result) and one backward pass per cotangent through the last:
    ``{label: {quantity: tensor}}``. `fast=False`: the stepwise route (``trajectory_kernel: False``). `expect_route`: assert
    that the FIRST solve did not and the last did (not) go through `_MlpLogqpTrajectoryFn`."""
    sde = (case.module() if module is None else copy.deepcopy(module)).to(device)
    if not fast:
        kw = dict(kw, options={"trajectory_kernel": False})
    for i in range(solves if fast else 1):
        ys, log_ratio, y0 = call(case, sde, device, names=names, **kw)
        if expect_route is not None and i == 0:
            assert not L.graph_has(ys, FN), "the first solve of a form returns the stepwise result"
    if expect_route is not None:
        assert L.graph_has(ys, FN) == expect_route, ("route", expect_route)
        assert L.graph_has(log_ratio, FN) == expect_route
    pnames, params = zip(*sde.named_parameters())
    out = {}
    for label, wy, wl in case.cotangents():
        grads = torch.autograd.grad([ys, log_ratio], [y0] + list(params), grad_outputs=[wy.to(device), wl.to(device)],
                                    retain_graph=True, allow_unused=True)
        grads = [torch.zeros_like(x) if g is None else g.detach().clone() for g, x in zip(grads, [y0] + list(params))]
        out[label] = dict(zip(["y0"] + list(pnames), grads))
        out[label]["ys"], out[label]["log_ratio"] = ys.detach(), log_ratio.detach()
    return out


def compare(got, ref, factor=BACKPROP_FACTOR, floor=BACKPROP_FLOOR):
    return L.compare(got, ref, factor=factor, floor=floor)


# ---- the step equations of csrc/mlp_backward.hip's KL instantiation, stated on the CPU (tests/test_mlp_logqp_backprop_host.py) --
def reverse_sweep(module, y0, dW, dt, cot_y, cot_l, drop_w=False):
    """dL/dy0 and the parameter gradients of L = <ys, cot_y> + <l, cot_l> over an every-step Euler solve of `module`
    (float64 tensors; a LatentLogqp with the "ou" prior: h = -theta y) with increments dW (K, B, d), by the reverse step of
    include/torchsde_amd.h (tsde_trajectory_mlp_diag_logqp_backward) written out with torch ops: `cot_y` (K + 1, B, d),
    `cot_l` (K + 1, B). `drop_w`: the MUTANT that feeds dt * lam instead of dt * (lam + w) to the W2 product."""
    W1, b1, W2, b2 = module.lin1.weight, module.lin1.bias, module.lin2.weight, module.lin2.bias
    c, e, hr, hs = module.rate, module.shift, -module.theta, torch.zeros_like(module.theta)
    sigmoid = module.diffusion == "sigmoid"
    act = torch.tanh if isinstance(module.act, torch.nn.Tanh) else torch.nn.functional.softplus
    steps = dW.shape[0]
    with torch.no_grad():
        ys = [y0]
        for k in range(steps):
            y = ys[-1]
            f = act(y @ W1.t() + b1) @ W2.t() + b2
            z = c * y + e
            g = 0.4 * torch.sigmoid(z) if sigmoid else z
            ys.append(y + f * dt + g * dW[k])
        lam = torch.zeros_like(y0)
        a_l = torch.zeros(y0.shape[0], dtype=y0.dtype)
        grads = {name: torch.zeros_like(p) for name, p in module.named_parameters()}
        for k in range(steps - 1, -1, -1):
            lam = lam + cot_y[k + 1]
            a_l = a_l + cot_l[k + 1]
            y = ys[k]
            zh = y @ W1.t() + b1
            hid = act(zh)
            slope = 1 - hid ** 2 if act is torch.tanh else torch.sigmoid(zh)
            f = hid @ W2.t() + b2
            z = c * y + e
            s = torch.sigmoid(z)
            g, q = (0.4 * s, 0.4 * s * (1 - s)) if sigmoid else (z, torch.ones_like(z))
            safe = g                                    # (|g| > 1e-7 on these cases: asserted by the caller)
            u = (f - (hr * y + hs)) / safe
            w = a_l[:, None] * u / safe
            fed = dt * (lam if drop_w else lam + w)
            delta = (fed @ W2) * slope
            kq = dt * a_l[:, None] * u ** 2 / safe
            lw = lam * dW[k] * q
            grads["lin2.weight"] += fed.t() @ hid
            grads["lin2.bias"] += fed.sum(0)
            grads["lin1.weight"] += delta.t() @ y
            grads["lin1.bias"] += delta.sum(0)
            grads["rate"] += ((lw - kq * q) * y).sum(0)
            grads["shift"] += (lw - kq * q).sum(0)
            grads["theta"] += (dt * w * y).sum(0)       # dL/dhr = sum -dt w y, hr = -theta
            lam = lam + delta @ W1 + lw * c - dt * hr * w - kq * q * c
        return lam + cot_y[0], grads
