"""Training through ``sdeint`` on the perceptron kernels on ANY output grid: outputs inside steps, several in one step, one
inside the first step, a ragged last step (tests/test_interp_backprop_host.py, tests/test_gpu_interp_backprop.py,
tools/interp_backprop_rounding_ratios.py; the routes are `kernels._MlpTrajectoryFn` behind ``sdeint`` on `MLPDriftDiagonalSDE`
and `kernels._MlpLogqpTrajectoryFn` behind ``sdeint(..., logqp=True)`` on an unchanged user module, the kernels
tsde_trajectory_mlp_diag_backward_weighted and tsde_trajectory_mlp_diag_logqp_backward_weighted).

Grids are in units of DT = 2^-5 over 16 steps, every time a multiple of DT / 4 (the rule of tests/helpers.py: float32 and float64
then hold the same grid). The reference is autograd THROUGH the oracle's stepwise solver (oracle/solvers_ref.integrate, which
interpolates as interp.py:15-18 does) on the same counter path, in float32 and float64."""
import copy

import numpy as np
import torch

from tests import helpers
from tests import helpers_logqp as L
from tests import helpers_logqp_backprop as KL

F32, F64 = torch.float32, torch.float64
DT, STEPS = helpers.RHEUN_DT, 16
assert DT == L.DT and STEPS == L.STEPS
GRIDS = dict(helpers.RHEUN_GRIDS)
# With a five-step stash budget the chunk tops are 16, 11, 6 and 1: an output in the step above an edge (10.5) and one in the
# step below it (11.5), one on the edge (11), two in one step (6.25, 6.75: the step above edge 6), one inside step 1 (0.5).
GRIDS["chunk_edges"] = (0, 0.5, 6.25, 6.75, 10.5, 11, 11.5, 16)
INSIDE_GRIDS = ("inside", "crowded", "first_step", "chunk_edges")       # those with an output inside a step
GPU_GRIDS = INSIDE_GRIDS + ("ragged", "every_step")
SHAPES = (helpers.MLP_GRAD_SHAPES[0], helpers.MLP_GRAD_SHAPES[1], helpers.MLP_GRAD_SHAPES[2])
assert SHAPES == ((16, 128, 128), (37, 20, 36), (129, 4, 16))
# method, sde type, diffusion of the plain route; the KL route takes helpers_logqp_backprop.SCHEMES
PLAIN_SCHEMES = (("euler", "ito", "affine"), ("euler", "ito", "sigmoid"), ("milstein", "ito", "affine"),
                 ("milstein", "stratonovich", "affine"))
# The kernels' result may differ from the float64 oracle by INTERP_FACTOR times the float32 oracle's own difference from it, plus
# INTERP_FLOOR of the quantity's scale: twice the worst ratio measured on an MI355X over every grid, shape, scheme, cotangent and
# quantity of both routes (profiles/interp_backprop_rounding_ratios.txt, written by tools/interp_backprop_rounding_ratios.py),
# rounded up, and at least 4 -- the rule of helpers.MLP_GRAD_FACTOR. Measured: worst ratio 5.516 over 3016 comparisons
# (dL/dshift of the affine KL diffusion at 129 x 4 x 16 on `every_step`, a boundary-only solve: 2.3e-6 of a gradient of size 130
# that sums 1032 terms of u^2 / g, against a float32 oracle run that happens to be right to 2.3e-7 there; five ratios above 1,
# all of them that sum at that shape), so 12.
INTERP_FACTOR = 12.0
INTERP_FLOOR = 1e-6
PLAIN_FN, KL_FN = "_MlpTrajectoryFn", KL.FN


def grid_ts(grid):
    return [u * DT for u in GRIDS[grid]]


def output_map(ts_list):
    """[(k_curr, w0, w1)] of the outputs after the first, from the solver's own grid."""
    return [(int(kc), float(w0), float(w1)) for (_, kc, w0, w1) in helpers.rheun_grid(ts_list, DT).outputs]


# ---- cases -------------------------------------------------------------------------------------------------------------------
class PlainCase:
    """`MLPDriftDiagonalSDE` under ``sdeint`` with autograd recording, on one grid."""
    route = "plain"

    def __init__(self, index, shape, scheme, activation, grid):
        self.B, self.d, self.hidden = shape
        self.method, self.sde_type, self.diffusion = scheme
        self.activation, self.grid = activation, grid
        self.seed, self.entropy = 500 + index, 11000 + index
        self.id = "-".join(["plain", self.method, self.sde_type, self.diffusion, activation, "x".join(str(v) for v in shape), grid])

    def module(self):
        return helpers.mlp_grad_module(self.d, self.hidden, self.activation, seed=self.seed, sde_type=self.sde_type,
                                       diffusion=self.diffusion)

    def y0(self):
        return 0.5 * torch.randn(self.B, self.d, generator=torch.Generator().manual_seed(self.seed))

    def ts(self):
        return grid_ts(self.grid)

    def cotangents(self):
        """helpers.rheun_cotangents: random on every output, and the same masked to the outputs inside steps."""
        return helpers.rheun_cotangents(self.ts(), self.B, self.d, self.seed + 1, DT)


class KlCase(L.Case):
    """helpers_logqp.Case (a `LatentLogqp` user module under ``sdeint(..., logqp=True)``) on one grid."""
    route = "logqp"

    def __init__(self, index, shape, scheme, activation, grid):
        super().__init__(index, shape, scheme, activation)
        self.grid = grid
        self.id = "-".join(["logqp", self.method, self.diffusion, activation, "x".join(str(v) for v in shape), grid])

    def ts(self):
        return grid_ts(self.grid)

    def cotangents(self):
        """[(label, cotangent of ys, cotangent of log_ratio)]: both on every output; both masked to the outputs inside steps
        (log_ratio[i] = l[i + 1] - l[i] counts as inside when either end is); the column's alone (helpers_logqp.Case)."""
        ts = self.ts()
        (_, wy), *masked = helpers.rheun_cotangents(ts, self.B, self.d, self.seed + 1, DT)
        wl = torch.randn(len(ts) - 1, self.B, generator=torch.Generator().manual_seed(self.seed + 2))
        out = [("all", wy, wl)]
        if masked:
            inside = helpers.rheun_inside(ts, DT)
            either = torch.tensor([float(a or b) for a, b in zip(inside[:-1], inside[1:])]).reshape(-1, 1)
            out.append(("inside", masked[0][1], wl * either))
        out.append(("log_ratio only", torch.zeros_like(wy), wl))
        return out


def plain_cases(grids=GPU_GRIDS, shapes=SHAPES, schemes=PLAIN_SCHEMES):
    out = []
    for scheme in schemes:
        for shape in shapes:
            for grid in grids:
                out.append(PlainCase(len(out), shape, scheme, ("tanh", "softplus")[len(out) % 2], grid))
    return out


def kl_cases(grids=GPU_GRIDS, shapes=SHAPES, schemes=KL.SCHEMES):
    out = []
    for scheme in schemes:
        for shape in shapes:
            for grid in grids:
                out.append(KlCase(60 + len(out), shape, scheme, ("tanh", "softplus")[len(out) % 2], grid))
    return out


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def plain_oracle(case, ts=None, module=None):
    """``{dtype: {label: {quantity: tensor}}}``: autograd through oracle/solvers_ref.integrate in float32 and float64."""
    sde = case.module() if module is None else module
    names = [name for name, _ in sde.named_parameters()]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        refs = helpers.grid_oracle(sde, case.d, case.ts() if ts is None else ts, range(case.B), case.entropy, case.y0(),
                                   case.cotangents(), dt=DT, method=case.method)
    finally:
        torch.set_num_threads(threads)
    return {dtype: {label: dict([("ys", ys), ("y0", g[0])] + list(zip(names, g[1:]))) for label, g in grads.items()}
            for dtype, (ys, grads) in refs.items()}


def oracle(case, ts=None):
    return plain_oracle(case, ts) if case.route == "plain" else KL.oracle(case, ts=ts)


# ---- GPU solves ------------------------------------------------------------------------------------------------------------------
def brownian(case, device, ts_list, rows=None, row_offset=0):
    """This package's BrownianInterval of `case` over [0, STEPS * DT] in cells of DT -- or, where the grid ends inside a cell
    (`ragged`), over [0, ts[-1]]: a step is then exactly one cell, the short last one included."""
    import torchsde_amd
    whole = abs(ts_list[-1] / DT - round(ts_list[-1] / DT)) == 0.0
    columns = case.d + (1 if case.route == "logqp" else 0)
    return torchsde_amd.BrownianInterval(0.0, STEPS * DT if whole else ts_list[-1], size=(case.B if rows is None else rows, columns),
                                         dtype=F32, device=device, entropy=case.entropy, dt=DT, row_offset=row_offset)


def plain_call(case, sde, device, ts=None, y0=None, rows=None, row_offset=0, **kw):
    import torchsde_amd
    if y0 is None:
        y0 = case.y0().to(device).requires_grad_(True)
    ts_list = case.ts() if ts is None else list(ts)
    bm = brownian(case, device, ts_list, rows=rows, row_offset=row_offset)
    return torchsde_amd.sdeint(sde, y0, torch.tensor(ts_list, device=device), bm=bm, method=case.method, dt=DT, **kw), y0


def kl_call(case, sde, device, ts=None, y0=None, rows=None, row_offset=0, **kw):
    """One ``sdeint(..., logqp=True)`` of `sde`: (ys, log_ratio, y0)."""
    import torchsde_amd
    if y0 is None:
        y0 = case.y0().to(device).requires_grad_(True)
    ts_list = case.ts() if ts is None else list(ts)
    bm = brownian(case, device, ts_list, rows=rows, row_offset=row_offset)
    ys, log_ratio = torchsde_amd.sdeint(sde, y0, torch.tensor(ts_list, device=device), bm=bm, method=case.method, dt=DT,
                                        logqp=True, **kw)
    return ys, log_ratio, y0


def plain_solve(case, device, **kw):
    """One ``sdeint`` under autograd on `_MlpTrajectoryFn` (this route verifies nothing: `MLPDriftDiagonalSDE` publishes its own
    dynamics) and one backward pass per cotangent: ``{label: {quantity: tensor}}``."""
    sde = case.module().to(device)
    ys, y0 = plain_call(case, sde, device, **kw)
    assert type(ys.grad_fn).__name__.startswith(PLAIN_FN), type(ys.grad_fn).__name__
    names, params = zip(*sde.named_parameters())
    out = {}
    for label, w in case.cotangents():
        grads = torch.autograd.grad(ys, [y0] + list(params), grad_outputs=w.to(device), retain_graph=True)
        out[label] = dict(zip(["y0"] + list(names), (g.detach().clone() for g in grads)))
        out[label]["ys"] = ys.detach()
    return out


def kl_solve(case, device, **kw):
    """Two ``sdeint(..., logqp=True)`` under autograd on a fresh copy of the case's module -- the first solve of the grid's key
    verifies and returns the stepwise result, the second goes through `_MlpLogqpTrajectoryFn` -- and one backward pass per
    cotangent through the second: ``{label: {quantity: tensor}}``."""
    sde = case.module().to(device)
    for i in range(2):
        ys, log_ratio, y0 = kl_call(case, sde, device, **kw)
        assert L.graph_has(ys, KL_FN) == (i == 1) and L.graph_has(log_ratio, KL_FN) == (i == 1), ("solve", i)
    pnames, params = zip(*sde.named_parameters())
    out = {}
    for label, wy, wl in case.cotangents():
        grads = torch.autograd.grad([ys, log_ratio], [y0] + list(params), grad_outputs=[wy.to(device), wl.to(device)],
                                    retain_graph=True, allow_unused=True)
        grads = [torch.zeros_like(x) if g is None else g.detach().clone() for g, x in zip(grads, [y0] + list(params))]
        out[label] = dict(zip(["y0"] + list(pnames), grads))
        out[label]["ys"], out[label]["log_ratio"] = ys.detach(), log_ratio.detach()
    return out


def solve(case, device, **kw):
    """Gradients of `case` on the kernels, the route asserted."""
    return plain_solve(case, device, **kw) if case.route == "plain" else kl_solve(case, device, **kw)


def compare(got, ref, factor=INTERP_FACTOR, floor=INTERP_FLOOR):
    return L.compare(got, ref, factor=factor, floor=floor)


# ---- the reverse step with interpolation weights, stated on the CPU in float64 (tests/test_interp_backprop_host.py) ------------
def increments(case, ts_list, dtype=F64, columns=None):
    """dW (K, B, columns) of the steps of `ts_list` on the case's counter path, and the step sizes (K)."""
    grid = helpers.rheun_grid(ts_list, DT)
    edges = grid.t_f64()
    m = case.d if columns is None else columns
    bm = helpers.counter_rows_bm(np.arange(case.B), m, case.entropy, edges, dtype)
    dW = torch.stack([bm(edges[k], edges[k + 1]) for k in range(len(edges) - 1)], dim=0)
    return dW, torch.tensor(np.diff(edges), dtype=dtype)


def reverse_sweep(net, y0, dW, dts, outputs, cot_y, cot_l=None, method="euler", ito=True, mutant=None):
    """dL/dy0 and the gradients of L = <ys, cot_y> [+ <l, cot_l>] for outputs anywhere in a step, by the reverse step of
    include/torchsde_amd.h (tsde_trajectory_mlp_diag_backward_weighted, tsde_trajectory_mlp_diag_logqp_backward_weighted) written
    out with float64 torch ops. `net`: W1 (hidden, d), b1, W2 (d, hidden), b2, c, e, act ("tanh" | "softplus"), amp (None: affine
    diffusion; else amp * sigmoid), and for the KL column hr, hs (else absent). `outputs`: [(k_curr, w0, w1)] after y0; `cot_y`
    (T, B, d), `cot_l` (T, B): cotangent of the column l itself. Returns (dL/dy0, dL/dl0 or None, {name: gradient}).
    `mutant`: "drop_w0" (the w0 share never added) or "exchange" (w0 and w1 exchanged)."""
    W1, b1, W2, b2, c, e = net["W1"], net["b1"], net["W2"], net["b2"], net["c"], net["e"]
    kl = "hr" in net
    act = torch.tanh if net["act"] == "tanh" else torch.nn.functional.softplus
    amp = net["amp"]
    steps = dW.shape[0]
    ys = [y0]
    for k in range(steps):
        y, dt, w = ys[-1], dts[k], dW[k]
        f = act(y @ W1.t() + b1) @ W2.t() + b2
        z = c * y + e
        g = z if amp is None else amp * torch.sigmoid(z)
        y1 = y + f * dt + g * w
        if method == "milstein":
            y1 = y1 + g * c * (0.5 * (w ** 2 - dt) if ito else 0.5 * w ** 2)
        ys.append(y1)
    lam = torch.zeros_like(y0)
    a_l = torch.zeros(y0.shape[0], dtype=y0.dtype)
    names = ["W1", "b1", "W2", "b2", "c", "e"] + (["hr", "hs"] if kl else [])
    grads = {name: torch.zeros_like(net[name]) for name in names}
    by_step = {}
    for j, (kc, w0, w1) in enumerate(outputs):
        if mutant == "exchange" and (w0, w1) != (0.0, 1.0):
            w0, w1 = w1, w0
        by_step.setdefault(kc, []).append((j + 1, w0, w1))
    for k in range(steps - 1, -1, -1):
        here = by_step.get(k + 1, ())
        for j, w0, w1 in here:                                     # before the products: lam is dL/dy_{k+1}
            lam = lam + w1 * cot_y[j]
            if kl:
                a_l = a_l + w1 * cot_l[j]
        y, dt, w = ys[k], dts[k], dW[k]
        zh = y @ W1.t() + b1
        hid = act(zh)
        slope = 1 - hid ** 2 if net["act"] == "tanh" else torch.sigmoid(zh)
        z = c * y + e
        s = torch.sigmoid(z)
        g, q = (z, torch.ones_like(z)) if amp is None else (amp * s, amp * s * (1 - s))
        fed, extra_y, kq = dt * lam, 0.0, 0.0
        if kl:
            f = hid @ W2.t() + b2
            u = (f - (net["hr"] * y + net["hs"])) / g                # (|g| > 1e-7 on these cases: asserted by the caller)
            wkl = a_l[:, None] * u / g
            kq = dt * a_l[:, None] * u ** 2 / g * q
            fed = dt * (lam + wkl)
            extra_y = -dt * net["hr"] * wkl - kq * c
            grads["hr"] += (-dt * wkl * y).sum(0)
            grads["hs"] += (-dt * wkl).sum(0)
        delta = (fed @ W2) * slope
        grads["W2"] += fed.t() @ hid
        grads["b2"] += fed.sum(0)
        grads["W1"] += delta.t() @ y
        grads["b1"] += delta.sum(0)
        if method == "milstein":
            v = 0.5 * (w ** 2 - dt) if ito else 0.5 * w ** 2
            grads["c"] += (lam * (y * w + v * (g + c * y)) - kq * y).sum(0)
            grads["e"] += (lam * (w + c * v) - kq).sum(0)
            step = lam * (c * w + c ** 2 * v)
        else:
            lw = lam * w * q
            grads["c"] += ((lw - kq) * y).sum(0)
            grads["e"] += (lw - kq).sum(0)
            step = lw * c
        lam = lam + delta @ W1 + step + extra_y
        if mutant != "drop_w0":
            for j, w0, w1 in here:                                 # after them: lam is dL/dy_k
                lam = lam + w0 * cot_y[j]
                if kl:
                    a_l = a_l + w0 * cot_l[j]
    return lam + cot_y[0], (a_l + cot_l[0]) if kl else None, grads


def plain_net(sde, dtype=F64):
    """`net` of `reverse_sweep` and the parameter name of each entry, from an `MLPDriftDiagonalSDE`."""
    m = copy.deepcopy(sde).cpu().to(dtype)
    d = m.lin1.in_features
    net = {"W1": m.lin1.weight.detach(), "b1": m.lin1.bias.detach(), "W2": m.lin2.weight.detach(), "b2": m.lin2.bias.detach(),
           "c": m.diff_rate.detach().expand(d), "e": m.diff_shift.detach().expand(d), "act": m.activation,
           "amp": m.diff_scale if m.diffusion == "sigmoid" else None}
    return net, {"lin1.weight": "W1", "lin1.bias": "b1", "lin2.weight": "W2", "lin2.bias": "b2", "diff_rate": "c",
                 "diff_shift": "e"}


def kl_net(module, dtype=F64):
    """... from a `LatentLogqp` with the "ou" prior: h = -theta y, so dL/dtheta = -dL/dhr."""
    m = copy.deepcopy(module).cpu().to(dtype)
    net = {"W1": m.lin1.weight.detach(), "b1": m.lin1.bias.detach(), "W2": m.lin2.weight.detach(), "b2": m.lin2.bias.detach(),
           "c": m.rate.detach(), "e": m.shift.detach(), "act": "tanh" if isinstance(m.act, torch.nn.Tanh) else "softplus",
           "amp": 0.4 if m.diffusion == "sigmoid" else None, "hr": -m.theta.detach(), "hs": torch.zeros_like(m.theta.detach())}
    return net, {"lin1.weight": "W1", "lin1.bias": "b1", "lin2.weight": "W2", "lin2.bias": "b2", "rate": "c", "shift": "e",
                 "theta": "hr"}


def stated_gradients(case, label, mutant=None, ts=None):
    """{quantity: tensor} of `reverse_sweep` for cotangent `label` of `case` in float64: "y0" and every parameter."""
    ts_list = case.ts() if ts is None else ts
    y0 = case.y0().to(F64)
    if case.route == "plain":
        sde = case.module()
        net, names = plain_net(sde)
        dW, dts = increments(case, ts_list)
        cot = dict(case.cotangents())[label].to(F64)
        gy, _, grads = reverse_sweep(net, y0, dW, dts, output_map(ts_list), cot, method=case.method,
                                     ito=case.sde_type == "ito", mutant=mutant)
        shapes = {name: p.shape for name, p in sde.named_parameters()}
        out = {"y0": gy}
        out.update((name, grads[key].reshape(shapes[name])) for name, key in names.items())
        return out
    net, names = kl_net(case.module())
    dW, dts = increments(case, ts_list, columns=case.d + 1)
    wy, wl = next((a, b) for (lab, a, b) in case.cotangents() if lab == label)
    cot = L.column_cotangent(wy, wl).to(F64)
    gy, _, grads = reverse_sweep(net, y0, dW[:, :, :case.d], dts, output_map(ts_list), cot[:, :, :case.d], cot[:, :, case.d],
                                 method=case.method, mutant=mutant)
    out = {"y0": gy}
    out.update((name, -grads[key] if name == "theta" else grads[key]) for name, key in names.items())
    return out
