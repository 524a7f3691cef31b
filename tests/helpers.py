"""Shared test helpers: golden fixture loading and replay Brownian motions."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def solver_cases():
    return sorted(f[len("solver_"):-4] for f in os.listdir(GOLDEN) if f.startswith("solver_") and f.endswith(".npz"))


def adjoint_cases():
    return sorted(f[len("adjoint_"):-4] for f in os.listdir(GOLDEN)
                  if f.startswith("adjoint_") and f.endswith(".npz") and not f.startswith("adjoint_adaptive_"))


class Case:
    """One golden solver case in one precision."""

    def __init__(self, name, tag, prefix="solver_"):
        z = load(f"{prefix}{name}.npz")
        self.z = z
        self.name, self.tag, self.dtype = name, tag, TORCH_DT[tag]
        self.problem, self.method, self.levy = str(z["problem"]), str(z["method"]), str(z["levy"])
        self.dt = float(z["dt"])
        self.options = {"grad_free": True} if bool(z["grad_free"]) else None
        self.B, self.d, self.m = (int(v) for v in z["shape"])
        self.ts = torch.tensor(z[f"{tag}__ts"], dtype=self.dtype)
        self.queries = z[f"{tag}__queries"]
        self.W = z[f"{tag}__W"]
        self.U = z[f"{tag}__U"]
        self.A = z[f"{tag}__A"] if f"{tag}__A" in z.files else None
        self.ys = torch.tensor(z[f"{tag}__ys"], dtype=self.dtype)
        self.param_checksum = float(z[f"{tag}__param_checksum"])

    def sde(self, device="cpu"):
        from workloads import problems
        sde = problems.make(self.problem, dtype=self.dtype, d=self.d, m=self.m)
        got = float(sum(p.detach().double().abs().sum() for p in sde.parameters()))
        assert abs(got - self.param_checksum) <= 1e-9 * max(1.0, abs(got)), "test problem parameters drifted"
        return sde.to(device)

    def y0(self, device="cpu"):
        return torch.full((self.B, self.d), 0.1, dtype=self.dtype, device=device)

    def table(self, device="cpu"):
        return {(float(a), float(b)): (torch.tensor(self.W[i], dtype=self.dtype, device=device),
                                       torch.tensor(self.U[i], dtype=self.dtype, device=device),
                                       None if self.A is None else torch.tensor(self.A[i], dtype=self.dtype,
                                                                                device=device))
                for i, (a, b) in enumerate(self.queries)}


def make_replay_bm(table, shape, dtype, device, levy):
    """A foreign BaseBrownian (seam S3) that replays stored increments. Intervals are matched to 1e-10: an adaptive
    solve proposes its step sizes from an error norm whose last bits depend on the reduction order, so its query
    times agree with the recorded ones to rounding, not bit for bit."""
    from torchsde_amd import BaseBrownian
    _dtype, _device, _shape, _levy = dtype, device, shape, levy
    nearby = {}
    for (a, b), v in table.items():
        nearby.setdefault((round(a, 10), round(b, 10)), v)

    class Replay(BaseBrownian):
        def __call__(self, ta, tb=None, return_U=False, return_A=False):
            key = (float(ta), float(tb))
            W, U, A = table[key] if key in table else nearby[(round(key[0], 10), round(key[1], 10))]
            if return_U:
                return (W, U, A) if return_A else (W, U)
            return (W, A) if return_A else W

        def __repr__(self):
            return "Replay"

        @property
        def dtype(self):
            return _dtype

        @property
        def device(self):
            return torch.device(_device)

        @property
        def shape(self):
            return tuple(_shape)

        @property
        def levy_area_approximation(self):
            return _levy

    return Replay()


def has_gpu():
    return torch.cuda.is_available()


def mlp_module_from(z, dtype, device):
    """The perceptron-drift module of a closed_form_mlp_*.npz fixture, with the fixture's parameter values."""
    import torchsde_amd
    B, d, hidden, steps = (int(v) for v in z["shape"])
    sde = torchsde_amd.MLPDriftDiagonalSDE(d, hidden, activation=str(z["activation"]), sde_type=str(z["sde_type"]),
                                           diffusion=str(z["diffusion"]), diff_scale=float(z["diff_scale"]),
                                           diff_rate=torch.tensor(z["param__diff_rate"]),
                                           diff_shift=torch.tensor(z["param__diff_shift"]), dtype=dtype)
    with torch.no_grad():
        for name, p in sde.named_parameters():
            p.copy_(torch.tensor(z["param__" + name]).to(dtype))
    return sde.to(device)


def sampled_rows(B, n=64, seed=0, seams=()):
    """~n global rows of a B-row batch: the first and last rows, both sides of every kernel / shard seam handed in
    (`seams`), both sides of the 256-row tile boundaries next to them, and random rows in between."""
    rows = {0, 1, B - 2, B - 1}
    for s in tuple(seams) + (B // 2, 256, 512, B - 256):
        rows.update(r for r in (s - 1, s, s + 1) if 0 <= r < B)
    gen = np.random.default_rng(seed)
    while len(rows) < n:
        rows.add(int(gen.integers(0, B)))
    return np.array(sorted(rows), dtype=np.int64)


def counter_rows_bm(rows, m, entropy, edges, dtype, levy=False):
    """The counter-RNG Brownian path of GLOBAL batch rows `rows` (m channels each) from the oracle's C twin of the
    generator, as the callable the oracle's solvers take: ``bm(ta, tb, return_U=False) -> (len(rows), m)`` tensors.
    Row r of an unsharded (B, m) BrownianInterval is elements r*m .. r*m + m - 1 of the counter field."""
    from oracle import counter
    npdt = np.float32 if dtype == torch.float32 else np.float64
    edges = np.ascontiguousarray(edges, dtype=np.float64)

    rows = np.asarray(rows, dtype=np.int64)
    # runs of consecutive rows are consecutive elements of the field: one query each
    starts = [0] + [k for k in range(1, len(rows)) if rows[k] != rows[k - 1] + 1] + [len(rows)]

    def bm(ta, tb, return_U=False, return_A=False):
        W = np.empty((len(rows), m), dtype=npdt)
        U = np.empty((len(rows), m), dtype=npdt) if levy else None
        for k0, k1 in zip(starts[:-1], starts[1:]):
            w, u, _ = counter.query((k1 - k0) * m, entropy, edges, float(ta), float(tb), dtype=npdt,
                                    elem0=int(rows[k0]) * m, have_h=levy)
            W[k0:k1] = w.reshape(k1 - k0, m)
            if levy:
                U[k0:k1] = u.reshape(k1 - k0, m)
        W = torch.from_numpy(W)
        return (W, torch.from_numpy(U)) if return_U else W

    return bm


# ---- the reversible-Heun pair over output-time grids (test_rheun_grids.py, test_gpu_neural_rheun*.py) -------------------------
RHEUN_DT = 2.0 ** -5
# Output times in units of RHEUN_DT. Every one is a multiple of DT / 4, so float32 and float64 hold the same grid (a time that
# float32 rounds, 3.4 DT say, gives the two oracle runs different steps and their difference stops measuring rounding).
RHEUN_GRIDS = {
    "aligned": (0, 5, 16),                            # the grid that earns trust
    "inside": (0, 3.5, 16),                           # one interpolated output
    "crowded": (0, 3.25, 3.5, 3.75, 4, 16),           # three outputs inside one step and one on its right boundary
    "first_step": (0, 0.5, 16),                       # interpolation against y0 (out_step = 1)
    "ragged": (0, 5, 15.25),                          # a short last step
    "one_short_step": (0, 0.75),                      # K = 1
    "every_step": tuple(range(9)),                    # consecutive out_step
}


def rheun_modules():
    """name -> (factory of the module on the CPU, d, m): the sde_gan generator at depth 2 and the reference's Neural* problems."""
    from workloads import problems
    return {"sde_gan_2": (lambda: problems.SdeGanGenerator(3, 16, 16, 2, seed=2), 16, 3),
            "neural_diagonal": (lambda: problems.make("netdiag_strat", d=12, hidden=16), 12, 12),
            "neural_scalar": (lambda: problems.make("netscalar_strat", d=6, hidden=8), 6, 1)}


def rheun_ts(name):
    return [u * RHEUN_DT for u in RHEUN_GRIDS[name]]


def rheun_grid(ts_list, dt=RHEUN_DT):
    """The solver's own grid of `ts_list` (timegrid.TimeGrid): step boundaries, and per output (k_prev, k_curr, w0, w1)."""
    from torchsde_amd import timegrid
    return timegrid.build(np.asarray(ts_list, dtype=np.float64), dt)


def rheun_inside(ts_list, dt=RHEUN_DT):
    """Per entry of `ts_list`: is that output interpolated inside a step (ys[0] never is)?"""
    return [False] + [not (w0 == 0.0 and w1 == 1.0) for (_, _, w0, w1) in rheun_grid(ts_list, dt).outputs]


def rheun_snapped(ts_list, dt=RHEUN_DT):
    """`ts_list` with every interpolated output moved to its step's right boundary: what a gradient that ignores the
    interpolation weights differentiates. Same steps, same Brownian cells."""
    grid = rheun_grid(ts_list, dt)
    return [ts_list[0]] + [float(grid.t[k_curr]) for (_, k_curr, _, _) in grid.outputs]


def rheun_cotangents(ts_list, B, d, seed, dt=RHEUN_DT):
    """[(label, (len(ts), B, d) float32 CPU tensor)]: a random cotangent on all outputs and, where the grid has an output
    inside a step, the same one masked to those outputs. The second is what makes a misplaced cotangent visible: among
    sixteen steps' worth of gradient from the boundary outputs it moves dL/dy0 by a few parts in a thousand only."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(len(ts_list), B, d, generator=gen)
    inside = rheun_inside(ts_list, dt)
    out = [("all", w)]
    if any(inside):
        out.append(("inside", w * torch.tensor(inside, dtype=w.dtype).reshape(-1, 1, 1)))
    return out


def grid_oracle(sde, m, ts_list, rows, entropy, y0, cotangents, dt=RHEUN_DT, adjoint=False, method="reversible_heun",
                adjoint_method=None, levy=False):
    """The oracle's reversible-Heun solve of a copy of `sde` on the counter path of global batch rows `rows`, in float32
    and in float64: ``{dtype: (ys, {label: [dL/dy0, dL/dtheta...]})}`` for L = sum(ys * cotangent), by back-propagation
    through oracle/solvers_ref.integrate_reversible_heun -- or, `adjoint`, by the reference's own backward pass
    (oracle/adjoint_ref.reversible_heun_adjoint_gradients, which steps to every output time). `y0`: (len(rows), d).
    Another `method`: oracle/solvers_ref.integrate, and adjoint_ref.adjoint_gradients with `adjoint_method`. `levy`: the path
    also serves the space-time Levy area (SRK)."""
    import copy
    from oracle import adjoint_ref, solvers_ref
    edges = rheun_grid(ts_list, dt).t_f64()
    out = {}
    for dtype in (torch.float32, torch.float64):
        ref_sde = copy.deepcopy(sde).cpu().to(dtype)
        params = [p for p in ref_sde.parameters() if p.requires_grad]
        bm = counter_rows_bm(np.asarray(rows), m, entropy, edges, dtype, levy=levy)
        ts = torch.tensor(ts_list, dtype=dtype)
        grads = {}
        if adjoint:
            for label, w in cotangents:
                if method == "reversible_heun":
                    ys, gy, gp = adjoint_ref.reversible_heun_adjoint_gradients(ref_sde, y0.detach().cpu().to(dtype), ts, bm,
                                                                               dt, w.to(dtype))
                else:
                    ys, gy, gp = adjoint_ref.adjoint_gradients(ref_sde, y0.detach().cpu().to(dtype), ts, bm, dt, method,
                                                               adjoint_method, w.to(dtype))
                grads[label] = [gy] + list(gp)
        else:
            y0_ref = y0.detach().cpu().to(dtype).requires_grad_(True)
            if method == "reversible_heun":
                ys, _ = solvers_ref.integrate_reversible_heun(ref_sde, bm, y0_ref, ts, dt)
            else:
                ys = solvers_ref.integrate(ref_sde, bm, y0_ref, ts, dt, method)
            for label, w in cotangents:
                got = torch.autograd.grad((ys * w.to(dtype)).sum(), [y0_ref] + params, retain_graph=True, allow_unused=True)
                grads[label] = [torch.zeros_like(x) if g is None else g for g, x in zip(got, [y0_ref] + params)]
        out[dtype] = (ys.detach(), grads)
    return out


def assert_within_reference_rounding(new32, ref32, ref64, what="", factor=4.0, floor=1e-6):
    """the float32 HIP result may differ from the float64 oracle by at most `factor` times what
    the oracle's own float32 run differs from it, plus `floor` (scaled by the magnitude of the compared quantity)."""
    new32, ref32, ref64 = (torch.as_tensor(x).detach().double().cpu() for x in (new32, ref32, ref64))
    scale = max(1.0, ref64.abs().max().item())
    err_new = (new32 - ref64).abs().max().item()
    err_ref = (ref32 - ref64).abs().max().item()
    assert err_new <= factor * err_ref + floor * scale, \
        f"{what}: |hip32 - ref64| = {err_new:.3e} > {factor} * |ref32 - ref64| ({err_ref:.3e}) + {floor * scale:.1e}"
    return err_new, err_ref


# ---- the perceptron training kernels held to float32 rounding (test_mlp_gradient_criterion.py, --------------------------------
# ---- test_gpu_mlp_gradient_rounding.py): autograd through `sdeint` (_MlpTrajectoryFn) and `sdeint_adjoint` (_MlpAdjointFn) ----
MLP_GRAD_DT = 2.0 ** -5
MLP_GRAD_STEPS = 16
# Output times in steps: the first step, two consecutive boundaries, an interior one and the last. Both routes take outputs
# on step boundaries only.
MLP_GRAD_OUTPUTS = (0, 1, 2, 9, 16)
# (B, d, hidden): each the smallest that reaches one edge of the kernels.
MLP_GRAD_SHAPES = (
    (16, 128, 128),      # one exact tile
    (37, 20, 36),        # ragged batch, padded channels
    (129, 4, 16),        # one row past a 128-row block
    (33, 64, 256),       # wide hidden layer
    (48, 124, 120),      # both widths just under a tile multiple
)
# route, forward method, adjoint method, sde type, diffusion. method None: every default (SRK forward with the space-time
# Levy area; Milstein backward for diagonal Ito noise).
MLP_GRAD_SCHEMES = (
    ("backprop", "euler", None, "ito", "affine"),
    ("backprop", "euler", None, "ito", "sigmoid"),
    ("backprop", "milstein", None, "ito", "affine"),
    ("backprop", "milstein", None, "stratonovich", "affine"),
    ("adjoint", "euler", "euler", "ito", "sigmoid"),
    ("adjoint", "euler", "milstein", "ito", "affine"),
    ("adjoint", "milstein", None, "ito", "sigmoid"),
    ("adjoint", "midpoint", "milstein", "stratonovich", "affine"),
    ("adjoint", None, None, "ito", "sigmoid"),
)
# The kernels' result may differ from the float64 oracle by MLP_GRAD_FACTOR times the float32 oracle's own difference from it,
# plus MLP_GRAD_FLOOR of the quantity's scale. The factor is twice the worst ratio measured on an MI355X over every case,
# cotangent and quantity below (profiles/mlp_gradient_rounding_ratios.txt), rounded up, and at least 4.
MLP_GRAD_FACTOR = 4.0
MLP_GRAD_FLOOR = 1e-6
MLP_GRAD_QUANTITIES = ("ys", "y0", "lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "diff_rate", "diff_shift")


class MlpGradCase:
    def __init__(self, index, shape, scheme, activation, scalar=False):
        self.B, self.d, self.hidden = shape
        self.route, self.method, self.adjoint_method, self.sde_type, self.diffusion = scheme
        self.activation, self.scalar = activation, scalar
        self.seed = 100 + index
        self.entropy = 7000 + index
        self.levy = self.method is None
        self.id = "-".join([self.route, self.method or "default", *([self.adjoint_method or "default"] * (self.route == "adjoint")),
                            self.sde_type, self.diffusion, activation, "x".join(str(v) for v in shape)]
                           + ["scalar"] * scalar)

    def module(self):
        """On the CPU, float32."""
        return mlp_grad_module(self.d, self.hidden, self.activation, seed=self.seed, scalar_diffusion=self.scalar,
                               sde_type=self.sde_type, diffusion=self.diffusion)

    def y0(self):
        gen = torch.Generator().manual_seed(self.seed)
        return 0.5 * torch.randn(self.B, self.d, generator=gen)

    def ts(self, outputs=MLP_GRAD_OUTPUTS):
        return [k * MLP_GRAD_DT for k in outputs]

    def cotangents(self):
        """[(label, (outputs, B, d) float32 CPU tensor)]: random on every output (ys[0] included), and the same one masked to
        the first, a middle and the last output in turn."""
        gen = torch.Generator().manual_seed(self.seed + 1)
        w = torch.randn(len(MLP_GRAD_OUTPUTS), self.B, self.d, generator=gen)
        out = [("all", w)]
        for label, j in (("first", 0), ("middle", len(MLP_GRAD_OUTPUTS) // 2), ("last", len(MLP_GRAD_OUTPUTS) - 1)):
            mask = torch.zeros(len(MLP_GRAD_OUTPUTS), 1, 1)
            mask[j] = 1.0
            out.append((label, w * mask))
        return out


def mlp_grad_module(d, hidden, activation, seed=0, scalar_diffusion=False, sde_type="ito", diffusion="affine"):
    """The recipe of tests/test_gpu_mlp_backward.py::_sde on the CPU: asymmetric, well-scaled weights (a transposed operand
    cannot pass) and per-channel diffusion parameters -- or, `scalar_diffusion`, 0-d ones."""
    import torchsde_amd
    gen = torch.Generator().manual_seed(seed)
    sigmoid = diffusion == "sigmoid"
    rate = torch.tensor(0.05) if scalar_diffusion else (2.0 if sigmoid else 0.2) * torch.rand(d, generator=gen) - 0.1
    shift = torch.tensor(0.2) if scalar_diffusion else 0.1 + 0.2 * torch.rand(d, generator=gen)
    sde = torchsde_amd.MLPDriftDiagonalSDE(d, hidden, activation=activation, diff_rate=rate, diff_shift=shift,
                                           sde_type=sde_type, diffusion=diffusion, diff_scale=0.4 if sigmoid else 1.0)
    with torch.no_grad():
        sde.lin1.weight.copy_(torch.randn(hidden, d, generator=gen) / d ** 0.5)
        sde.lin2.weight.copy_(torch.randn(d, hidden, generator=gen) / hidden ** 0.5)
        sde.lin1.bias.copy_(0.3 * torch.randn(hidden, generator=gen))
        sde.lin2.bias.copy_(0.3 * torch.randn(d, generator=gen))
    return sde


def mlp_grad_cases():
    """Every shape under every scheme; the activation alternates along the table so that each shape and each scheme meets
    both (five shapes and nine schemes: an odd stride)."""
    cases = []
    for scheme in MLP_GRAD_SCHEMES:
        for shape in MLP_GRAD_SHAPES:
            cases.append(MlpGradCase(len(cases), shape, scheme, ("tanh", "softplus")[len(cases) % 2]))
    return cases


def mlp_grad_scalar_cases():
    """0-d diffusion parameters, on each route (affine and sigmoid), at the ragged shape."""
    return [MlpGradCase(900 + i, MLP_GRAD_SHAPES[1], MLP_GRAD_SCHEMES[k], act, scalar=True)
            for i, (k, act) in enumerate(((0, "softplus"), (2, "tanh"), (4, "tanh"), (5, "softplus")))]


def mlp_grad_oracle(case, sde=None, outputs=MLP_GRAD_OUTPUTS, cotangents=None):
    """``{dtype: {label: {quantity: tensor}}}`` over MLP_GRAD_QUANTITIES from `grid_oracle` for `case`: autograd through
    oracle/solvers_ref.integrate, or oracle/adjoint_ref.adjoint_gradients, in float32 and float64, on the counter path of
    rows 0 .. B-1. `sde`: another module than the case's own (a mutant); `outputs`: another grid, in steps."""
    sde = case.module() if sde is None else sde
    cotangents = case.cotangents() if cotangents is None else cotangents
    names = [name for name, _ in sde.named_parameters()]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)       # tensors this small only wait for a thread pool; and one summation order on every machine
    try:
        refs = grid_oracle(sde, case.d, case.ts(outputs), range(case.B), case.entropy, case.y0(), cotangents,
                           dt=MLP_GRAD_DT, adjoint=case.route == "adjoint", method=case.method or "srk",
                           adjoint_method=case.adjoint_method, levy=case.levy)
    finally:
        torch.set_num_threads(threads)
    out = {}
    for dtype, (ys, grads) in refs.items():
        out[dtype] = {label: dict([("ys", ys), ("y0", g[0])] + list(zip(names, g[1:]))) for label, g in grads.items()}
    return out


def mlp_grad_ragged_slices(case, quantity):
    """The sub-blocks of `quantity` to compare on their own (a max-norm over the whole tensor can hide an error confined to
    one): the rows of the ragged last 16-row tile of dL/dy0, the last partial 16-wide tile of rows and of columns of each
    weight gradient. {label: index tuple}."""
    def last_tile(n):
        return slice(16 * ((n - 1) // 16), n)
    if quantity == "y0":
        return {"last row tile": (last_tile(case.B),)}
    if quantity in ("lin1.weight", "lin2.weight"):
        rows, cols = (case.hidden, case.d) if quantity == "lin1.weight" else (case.d, case.hidden)
        return {"last tile of rows": (last_tile(rows),), "last tile of columns": (slice(None), last_tile(cols))}
    return {}
