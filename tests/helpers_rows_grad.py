"""Row-coupled systems trained through `sdeint` (kernels._RowsTrajectoryFn): the modules, the cases and the float64 oracle that
test_rows_grad_host.py, test_gpu_rows_grad.py and tools/rows_grad_rounding_ratios.py share."""
import functools

import numpy as np
import torch
from torch import nn

from tests import helpers

DT = 2.0 ** -8
STEPS = 16
TS = (0.0, 5.5 * DT, STEPS * DT)          # a boundary output, one inside the sixth step (weights 1/2, 1/2), the last boundary
# The float32 kernel may differ from the float64 oracle by ROWS_GRAD_FACTOR times what the oracle's own float32 run differs from
# it, plus ROWS_GRAD_FLOOR of the quantity's scale (helpers.assert_within_reference_rounding). The factor is twice the worst
# ratio measured on an MI355X over every case, cotangent and quantity below (tools/rows_grad_rounding_ratios.py,
# profiles/rows_grad_rounding_ratios.txt), rounded up, and at least 4.
ROWS_GRAD_FACTOR = 4.0
ROWS_GRAD_FLOOR = 1e-6


class Lorenz(nn.Module):
    """The stochastic Lorenz system of the reference's examples/latent_sde_lorenz.py:56-86 with its six constants as
    parameters."""
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, a=(10.0, 28.0, 8.0 / 3.0), b=(0.1, 0.28, 0.3)):
        super().__init__()
        self.a = nn.Parameter(torch.tensor(a))
        self.b = nn.Parameter(torch.tensor(b))

    def f(self, t, y):
        x1, x2, x3 = torch.split(y, (1, 1, 1), dim=1)
        a1, a2, a3 = self.a
        return torch.cat([a1 * (x2 - x1), a2 * x1 - x2 - x1 * x3, x1 * x2 - a3 * x3], dim=1)

    def g(self, t, y):
        return y * self.b


class ForcedVanDerPol(nn.Module):
    """tests/test_gpu_rows.py's module: a 0-d `mu`, a one-element `amp`, a two-element `sigma`."""
    noise_type = "diagonal"

    def __init__(self, sde_type="ito"):
        super().__init__()
        self.sde_type = sde_type
        self.mu = nn.Parameter(torch.tensor(1.5))
        self.amp = nn.Parameter(torch.tensor([0.4]))
        self.sigma = nn.Parameter(torch.tensor([0.2, 0.3]))

    def f(self, t, y):
        x, v = y[:, 0], y[:, 1]
        return torch.stack([v, self.mu * (1 - x ** 2) * v - x + self.amp * torch.sin(t)], dim=1)

    def g(self, t, y):
        x, v = y.unbind(dim=1)
        return torch.stack([torch.tanh(v), torch.sigmoid(x)], dim=1) * self.sigma


class Ring(nn.Module):
    """d channels, each reading every channel (through the row's sum) and its neighbour; `n` trainable rates in turn."""
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, d, n):
        super().__init__()
        self.d = d
        self.rate = nn.ParameterList([nn.Parameter(v) for v in torch.linspace(0.6, 1.4, n)])      # n 0-d parameters

    def f(self, t, y):
        cols, rate = y.unbind(dim=1), list(self.rate)
        total = cols[0]
        for c in cols[1:]:
            total = total + c
        return torch.stack([rate[c % len(rate)] * (total * 0.25 - cols[c]) - cols[c] * cols[(c + 1) % self.d]
                            for c in range(self.d)], dim=1)

    def g(self, t, y):
        cols, rate = y.unbind(dim=1), list(self.rate)
        return torch.stack([0.3 * torch.tanh(cols[(c + 2) % self.d] * rate[(c + 1) % len(rate)]) for c in range(self.d)], dim=1)


class Case:
    def __init__(self, name, make, d, B, method, levy, y0_grad=True, direct=False):
        self.name, self.make, self.d, self.B, self.method, self.levy = name, make, d, B, method, levy
        self.y0_grad, self.direct = y0_grad, direct
        self.seed = 40 + sum(name.encode()) % 50
        self.entropy = 9100 + sum(name.encode()) % 97
        self.id = f"{name}-{method}-B{B}"

    def module(self):
        """On the CPU, float32."""
        torch.manual_seed(self.seed)
        return self.make()

    def y0(self, dtype=torch.float32):
        gen = torch.Generator().manual_seed(self.seed)
        return (0.5 + 0.5 * torch.randn(self.B, self.d, generator=gen)).to(dtype)

    def cotangents(self):
        """A random cotangent on all outputs, and the same one masked to the interpolated output."""
        gen = torch.Generator().manual_seed(self.seed + 1)
        w = torch.randn(len(TS), self.B, self.d, generator=gen)
        mask = torch.tensor([0.0, 1.0, 0.0]).reshape(-1, 1, 1)
        return [("all", w), ("inside", w * mask)]

    def names(self):
        return ["ys"] + (["y0"] if self.y0_grad else []) + [n for n, _ in self.module().named_parameters()]


# d = 8 at the Euler cap of float32 (specialise.ROWS_SENS_CAP, 84): y0's eight tangents and one rate, 8 * (9 + 1) = 80; one
# more rate (88) is over the size rule
RING_RATES = 1
CASES = (
    Case("lorenz", Lorenz, 3, 257, "euler", "none"),
    Case("vanderpol", ForcedVanDerPol, 2, 257, "srk", "space-time"),
    Case("vanderpol_strat", lambda: ForcedVanDerPol("stratonovich"), 2, 257, "midpoint", "none"),
    Case("ring8", lambda: Ring(8, RING_RATES), 8, 257, "euler", "none"),
    Case("lorenz_one_row", Lorenz, 3, 1, "euler", "none", direct=True),
)


@functools.lru_cache(maxsize=None)
def oracle(index):
    """{dtype: (ys, {label: [ys-sized gradients...]})} of case `index` from autograd through oracle/solvers_ref.integrate on the
    counter path, in float32 and in float64; computed once."""
    case = CASES[index]
    out = helpers.grid_oracle(case.module(), case.d, list(TS), np.arange(case.B), case.entropy, case.y0(), case.cotangents(),
                              dt=DT, method=case.method, levy=case.levy != "none")
    if not case.y0_grad:
        out = {dtype: (ys, {label: g[1:] for label, g in grads.items()}) for dtype, (ys, grads) in out.items()}
    return out


def quantities(case, ys, grads):
    """[(name, tensor)] of a result in the order of `case.names()`."""
    return list(zip(case.names(), [ys] + list(grads)))


def solve(case, sde, device, dtype=torch.float32, options=None, grad=True, entropy=None):
    """(ys, y0) of `sdeint` on the case's path."""
    import torchsde_amd
    y0 = case.y0(dtype).to(device)
    if grad and case.y0_grad:
        y0.requires_grad_(True)
    bm = torchsde_amd.BrownianInterval(0.0, STEPS * DT, size=(case.B, case.d), device=device, dtype=dtype,
                                       entropy=case.entropy if entropy is None else entropy, levy_area_approximation=case.levy)
    ts = torch.tensor(TS, device=device, dtype=dtype)
    opts = {"hip_graph": False}
    opts.update(options or {})
    with (torch.enable_grad() if grad else torch.no_grad()):
        ys = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=case.method, dt=DT, options=opts)
    return ys, y0


def solve_direct(case, sde, device, dtype=torch.float32):
    """(ys, y0) of the tangent unit launched without `sdeint` (whose recognised routes take batches of eight rows and more)."""
    import torchsde_amd
    from torchsde_amd import kernels as K, recognise_rows, timegrid
    from torchsde_amd.sde import ForwardSDE
    y0 = case.y0(dtype).to(device).requires_grad_(case.y0_grad)
    bm = torchsde_amd.BrownianInterval(0.0, STEPS * DT, size=(case.B, case.d), device=device, dtype=dtype, entropy=case.entropy,
                                       levy_area_approximation=case.levy)
    ts = torch.tensor(TS, device=device, dtype=dtype)
    found = recognise_rows.recognise_rows(ForwardSDE(sde), ts[0], y0, differentiable=True)
    steps = K.solve_steps(timegrid.build(timegrid.ts_to_host(ts), DT), bm)
    schedule = steps.schedule(device, dtype)
    from torchsde_amd import _native
    code = {"euler": _native.TRAJ_EULER, "midpoint": _native.TRAJ_MIDPOINT, "srk": _native.TRAJ_SRK}[case.method]
    return K.trajectory_rows_differentiable(y0, found, code, schedule, bm), y0


def gradients(case, sde, ys, y0, w):
    inputs = ([y0] if case.y0_grad else []) + list(sde.parameters())
    return torch.autograd.grad((ys * w.to(ys)).sum(), inputs, retain_graph=True)


def measured(index, device):
    """[(label, name, kernel float32, oracle float32, oracle float64)] of case `index`, every quantity and cotangent."""
    case = CASES[index]
    sde = case.module().to(device)
    if case.direct:
        ys, y0 = solve_direct(case, sde, device)
    else:
        solve(case, sde, device)                                # the verifying solve
        ys, y0 = solve(case, sde, device)
    assert ys is not None and type(ys.grad_fn).__name__ == "_RowsTrajectoryFnBackward"
    ref = oracle(index)
    rows = []
    for label, w in case.cotangents():
        got = quantities(case, ys.detach(), gradients(case, sde, ys, y0, w))
        want32 = quantities(case, ref[torch.float32][0], ref[torch.float32][1][label])
        want64 = quantities(case, ref[torch.float64][0], ref[torch.float64][1][label])
        rows += [(label, name, a, b[1], c[1]) for (name, a), b, c in zip(got, want32, want64)]
    return rows


def dense_system(d, nt):
    """(structure, n_const, slots, y0_grad) of the dense system with d channels and nt tangents: with s = x_0 + ... + x_{d-1},
    f_c = k * (x_c * s) and g_c = k' * tanh(s - x_c), the constants taken in turn from the trainable ones. y0 carries tangents
    once nt >= d; the rest are trainable scalars (nt < d: trainable scalars only)."""
    y0_grad = nt >= d
    n_train = nt - (d if y0_grad else 0)
    n_const = max(n_train, 1)
    slots = tuple(range(n_train)) if n_train else (-1,)
    statements, outputs = [], []

    def emit(op, *operands):
        statements.append((op, tuple(operands)))
        return f"n{len(statements) - 1}"
    s = "x.v[0]"
    for c in range(1, d):
        s = emit("add", s, f"x.v[{c}]")
    turn = 0
    for c in range(d):
        outputs.append(emit("mul", f"c[{turn % n_const}]", emit("mul", f"x.v[{c}]", s)))
        turn += 1
    for c in range(d):
        outputs.append(emit("mul", f"c[{turn % n_const}]", emit("tanh", emit("sub", s, f"x.v[{c}]"))))
        turn += 1
    structure = (("rows", d, tuple(statements), tuple(outputs)), ("consts", n_const))
    return structure, n_const, slots, y0_grad
