"""Cases, modules, reference and comparison of ``sdeint_adjoint(..., logqp=True)`` on the KL perceptron kernels
(tests/test_gpu_mlp_logqp_adjoint.py, tools/mlp_logqp_rounding_ratios.py; the route is torchsde_amd/mlp_adjoint.plan_logqp).

A user-style module -- drift ``lin2(act(lin1(y)))``, affine or sigmoid diagonal diffusion, a per-channel affine prior drift --
solved on the grid of `helpers.MLP_GRAD_OUTPUTS`; the reference is the oracle's restatement of the reference's `SDELogqp` under
its stochastic adjoint (oracle/solvers_ref.LogqpRef + oracle/adjoint_ref.adjoint_gradients) on the same counter path, whose
Brownian motion has d + 1 columns, in float32 and float64."""
import copy

import numpy as np
import torch
from torch import nn

from tests import helpers

F32, F64 = torch.float32, torch.float64
DT, STEPS, OUTPUTS = helpers.MLP_GRAD_DT, helpers.MLP_GRAD_STEPS, helpers.MLP_GRAD_OUTPUTS
# (B, d, hidden): the exact-tile, 8-wave shape; ragged batch and padded channels; one row past a block with d + 1 = 5, so that
# every residue of the row's first element modulo the RNG quad occurs within eight rows
SHAPES = ((16, 128, 128), (37, 20, 36), (129, 4, 16))
# forward method, adjoint method (None: the default, Milstein), diffusion
SCHEMES = (("euler", "euler", "sigmoid"), ("euler", None, "affine"), ("milstein", None, "sigmoid"))
# Smallest |g| the float64 reference run may meet: u = (f - h) / g and its derivatives are then conditioned well enough for the
# float32 reference's own error to be a meaningful yardstick.
MIN_DIFFUSION = 0.05
# The kernels' result may differ from the float64 oracle by LOGQP_FACTOR times the float32 oracle's own difference from it, plus
# LOGQP_FLOOR of the quantity's scale: twice the worst ratio measured on an MI355X over every case, cotangent and quantity
# (profiles/mlp_logqp_adjoint_rounding_ratios.txt, written by tools/mlp_logqp_rounding_ratios.py), rounded up, and at least 4 --
# the rule of helpers.MLP_GRAD_FACTOR.
LOGQP_FACTOR = 4.0
LOGQP_FLOOR = 1e-6


class LatentNamed(nn.Module):
    """Written as a user would: nothing of this package in it. The prior drift is the method `prior`: for
    ``names={"prior_drift": "prior"}``."""
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, d, hidden, activation="softplus", diffusion="sigmoid", prior="ou", seed=0, theta_elements=None,
                 sde_type="ito"):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.sde_type = sde_type
        self.lin1, self.lin2 = nn.Linear(d, hidden), nn.Linear(hidden, d)
        self.act = nn.Tanh() if activation == "tanh" else nn.Softplus()
        self.diffusion, self.prior_kind = diffusion, prior
        with torch.no_grad():
            self.lin1.weight.copy_(torch.randn(hidden, d, generator=gen) / d ** 0.5)
            self.lin2.weight.copy_(torch.randn(d, hidden, generator=gen) / hidden ** 0.5)
            self.lin1.bias.copy_(0.3 * torch.randn(hidden, generator=gen))
            self.lin2.bias.copy_(0.3 * torch.randn(d, generator=gen))
        if diffusion == "sigmoid":     # 0.4 sigmoid(z), z >= -0.5 |y| + 0.1: above 0.07 for |y| <= 3
            self.rate = nn.Parameter(torch.rand(d, generator=gen) - 0.5)
            self.shift = nn.Parameter(0.1 + 0.2 * torch.rand(d, generator=gen))
        else:                          # c y + e with c in [-0.05, 0.05], e in [0.2, 0.3]
            self.rate = nn.Parameter(0.1 * torch.rand(d, generator=gen) - 0.05)
            self.shift = nn.Parameter(0.2 + 0.1 * torch.rand(d, generator=gen))
        if prior in ("ou", "mean_reverting", "tanh", "times_t"):
            self.theta = nn.Parameter(0.5 + torch.rand(d if theta_elements is None else theta_elements, generator=gen))
        if prior == "mean_reverting":
            self.mu = nn.Parameter(0.3 * torch.randn(d, generator=gen))

    def f(self, t, y):
        return self.lin2(self.act(self.lin1(y)))

    def g(self, t, y):
        z = self.rate * y + self.shift
        return 0.4 * torch.sigmoid(z) if self.diffusion == "sigmoid" else z

    def prior(self, t, y):
        if self.prior_kind == "ou":
            return -self.theta * y
        if self.prior_kind == "mean_reverting":
            return self.theta * (self.mu - y)
        if self.prior_kind == "numbers":
            return -0.5 * y + 0.05
        if self.prior_kind == "tanh":
            return -self.theta * torch.tanh(y)
        if self.prior_kind == "times_t":
            return -self.theta * y * t
        raise AssertionError(self.prior_kind)


class LatentLogqp(LatentNamed):
    """... with the prior drift under its canonical name."""

    def h(self, t, y):
        return self.prior(t, y)


class Case:
    def __init__(self, index, shape, scheme, activation):
        self.B, self.d, self.hidden = shape
        self.method, self.adjoint_method, self.diffusion = scheme
        self.activation = activation
        self.seed, self.entropy = 300 + index, 9000 + index
        self.id = "-".join([self.method, self.adjoint_method or "default", self.diffusion, activation,
                            "x".join(str(v) for v in shape)])

    def module(self, prior="ou", named=False, **kw):
        return (LatentNamed if named else LatentLogqp)(self.d, self.hidden, self.activation, self.diffusion, prior=prior, seed=self.seed, **kw)

    def y0(self):
        return 0.5 * torch.randn(self.B, self.d, generator=torch.Generator().manual_seed(self.seed))

    def ts(self):
        return [k * DT for k in OUTPUTS]

    def cotangents(self):
        """[(label, cotangent of ys (T, B, d), cotangent of log_ratio (T - 1, B))]: both, the KL terms alone, the state's
        alone. The log-ratio's is scaled to the state's size of gradient (the column is a sum over d channels of u^2 / 2)."""
        gen = torch.Generator().manual_seed(self.seed + 1)
        wy = torch.randn(len(OUTPUTS), self.B, self.d, generator=gen)
        wl = torch.randn(len(OUTPUTS) - 1, self.B, generator=gen)
        return [("all", wy, wl), ("log_ratio only", torch.zeros_like(wy), wl), ("ys only", wy, torch.zeros_like(wl))]


def cases():
    out = []
    for scheme in SCHEMES:
        for shape in SHAPES:
            out.append(Case(len(out), shape, scheme, ("tanh", "softplus")[len(out) % 2]))
    return out


def column_cotangent(wy, wl):
    """The cotangent of the augmented output (T, B, d + 1) that <ys, wy> + <log_ratio, wl> is, log_ratio[k] = l[k + 1] - l[k]
    (sdeint.py:284-295)."""
    col = torch.zeros(wy.shape[0], wy.shape[1], dtype=wy.dtype)
    col[1:] += wl
    col[:-1] -= wl
    return torch.cat((wy, col.unsqueeze(-1)), dim=2)


def quantities(module):
    return ["ys", "log_ratio", "y0"] + [name for name, _ in module.named_parameters()]


def oracle(case, module=None, names=None):
    """``{dtype: {label: {quantity: tensor}}}`` from the oracle in float32 and float64, plus ``min_g``: the smallest |g| the
    float64 run meets at its output states."""
    from oracle import adjoint_ref, solvers_ref
    module = case.module() if module is None else module
    pnames = [name for name, _ in module.named_parameters()]
    edges = helpers.rheun_grid(case.ts(), DT).t_f64()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {}
    try:
        for dtype in (F32, F64):
            ref = copy.deepcopy(module).cpu().to(dtype)
            aug = solvers_ref.LogqpRef(ref, names)
            bm = helpers.counter_rows_bm(np.arange(case.B), case.d + 1, case.entropy, edges, dtype)
            ts = torch.tensor(case.ts(), dtype=dtype)
            y0 = case.y0().to(dtype)
            y0_aug = torch.cat((y0, y0.new_zeros(case.B, 1)), dim=1)
            out[dtype] = {}
            for label, wy, wl in case.cotangents():
                ys_aug, gy, gp = adjoint_ref.adjoint_gradients(aug, y0_aug, ts, bm, DT, case.method, case.adjoint_method,
                                                               column_cotangent(wy, wl).to(dtype))
                col = ys_aug[:, :, -1]
                found = {"ys": ys_aug[:, :, :-1].detach(), "log_ratio": (col[1:] - col[:-1]).detach(),
                         "y0": gy[:, :-1].detach()}
                found.update(zip(pnames, (g.detach() for g in gp)))
                out[dtype][label] = found
            if dtype == F64:
                with torch.no_grad():
                    ys = out[dtype]["all"]["ys"]
                    g = getattr(ref, (names or {}).get("diffusion", "g"))(ts[0], ys.reshape(-1, case.d))
                out["min_g"] = g.abs().min().item()
    finally:
        torch.set_num_threads(threads)
    return out


def brownian(case, device, rows=None, row_offset=0):
    import torchsde_amd
    return torchsde_amd.BrownianInterval(0.0, STEPS * DT, size=(case.B if rows is None else rows, case.d + 1), dtype=F32,
                                         device=device, entropy=case.entropy, dt=DT, row_offset=row_offset)


def graph_has(tensor, name):
    """Whether a node whose class name starts with `name` is within a few edges of `tensor` in the autograd graph
    (contract.parse_return splits the Function's output)."""
    seen, frontier = set(), [tensor.grad_fn]
    for _ in range(6):
        nxt = []
        for fn in frontier:
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            if type(fn).__name__.startswith(name):
                return True
            nxt.extend(f for f, _ in fn.next_functions)
        frontier = nxt
    return False


def solve(case, device, module=None, fast=True, names=None, expect_route=None, solves=2, **kw):
    """`solves` calls of ``sdeint_adjoint(..., logqp=True)`` on a copy of the case's module (the first of a form verifies and
    returns the stepwise result) and one backward pass per cotangent through the last: ``{label: {quantity: tensor}}``.
    `fast=False`: the stepwise route. `expect_route`: assert that the last solve did (not) go through the KL Function."""
    import torchsde_amd
    sde = (case.module() if module is None else copy.deepcopy(module)).to(device)
    y0 = case.y0().to(device).requires_grad_(True)
    ts = torch.tensor(case.ts(), device=device)
    options = {} if fast else {"adjoint_options": {"trajectory_kernel": False}}
    options.update(kw)
    for _ in range(solves if fast else 1):
        ys, log_ratio = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=brownian(case, device), method=case.method,
                                                    adjoint_method=case.adjoint_method, dt=DT, logqp=True, names=names,
                                                    **options)
    if expect_route is not None:
        assert graph_has(ys, "_MlpLogqpAdjointFn") == expect_route, ("route", expect_route)
        assert graph_has(log_ratio, "_MlpLogqpAdjointFn") == expect_route
    pnames, params = zip(*sde.named_parameters())
    out = {}
    for label, wy, wl in case.cotangents():
        grads = torch.autograd.grad([ys, log_ratio], [y0] + list(params), grad_outputs=[wy.to(device), wl.to(device)],
                                    retain_graph=True, allow_unused=True)
        grads = [torch.zeros_like(x) if g is None else g.detach().clone() for g, x in zip(grads, [y0] + list(params))]
        out[label] = dict(zip(["y0"] + list(pnames), grads))
        out[label]["ys"], out[label]["log_ratio"] = ys.detach(), log_ratio.detach()
    return out


def compare(got, ref, factor=LOGQP_FACTOR, floor=LOGQP_FLOOR):
    """Every quantity of `got` against the oracle: [(what, err_new, err_ref, ratio)] with ratio = (err_new - floor * scale) /
    err_ref -- the factor that quantity needs -- and the messages of those `helpers.assert_within_reference_rounding` refuses."""
    records, failures = [], []
    for label, found in got.items():
        for name, value in found.items():
            new = value.double().cpu()
            r32, r64 = ref[F32][label][name].double(), ref[F64][label][name]
            assert new.shape == r64.shape and new.numel() > 0, (name, new.shape, r64.shape)
            scale = max(1.0, r64.abs().max().item())
            err_new, err_ref = (new - r64).abs().max().item(), (r32 - r64).abs().max().item()
            excess = err_new - floor * scale
            ratio = 0.0 if excess <= 0.0 else (excess / err_ref if err_ref > 0.0 else float("inf"))
            what = f"{label} {name}"
            records.append((what, err_new, err_ref, ratio))
            try:
                helpers.assert_within_reference_rounding(new, r32, r64, what, factor=factor, floor=floor)
            except AssertionError as e:
                failures.append(str(e))
    return records, failures
