"""The reversible Heun pair on the matrix cores (csrc/tsde_neural_rheun.h, torchsde_amd/neural_rheun.py; ``-m gpu``).

Kernel level, through the C ABI: `tsde_rheun_mlp_forward` / `_backward` against a float64 torch statement of
methods/reversible_heun.py:48-73 on the SAME increments (the Brownian motion's own, queried interval by interval), values and --
by autograd through that statement -- the gradients with respect to y0 and every weight: what `sdeint_adjoint(method=
"reversible_heun", adjoint_method="adjoint_reversible_heun")` returns in the reference up to rounding (the pair's backward pass is
exact, reversible_heun.py:76-144)."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = 2.0 ** -6


def _linears(gen, sizes, bias=True):
    out = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        w = (torch.randn(b, a, generator=gen) / a ** 0.5).to(DEV).requires_grad_(True)
        out.append((w, (0.1 * torch.randn(b, generator=gen)).to(DEV).requires_grad_(True) if bias else None))
    return out


def _nets(d, m, hidden, depth, act, final_f, final_g, noise, seed, time_input=True):
    from torchsde_amd import _native
    from torchsde_amd.neural_rheun import DeepNet
    gen = torch.Generator().manual_seed(seed)
    out = d * m if noise == "general" else d
    inp = d + (1 if time_input else 0)
    act_code = {"tanh": _native.ACT_TANH, "softplus": _native.ACT_SOFTPLUS, "lipswish": _native.ACT_SILU}[act]
    finals = {None: _native.FINAL_NONE, "sigmoid": _native.FINAL_SIGMOID, "tanh": _native.FINAL_TANH}
    scale = 0.909 if act == "lipswish" else 1.0
    f = DeepNet(_linears(gen, [inp] + [hidden] * (depth - 1) + [d]), act_code, scale, finals[final_f], 1.0, time_input)
    g = DeepNet(_linears(gen, [inp] + [hidden] * (depth - 1) + [out]), act_code, scale, finals[final_g], 0.3, time_input)
    return f, g


def _pairs(outputs):
    """[(out_step, (w0, w1))]: a bare step number is an output on that step's right boundary."""
    return [(int(o), (0.0, 1.0)) if np.isscalar(o) else (int(o[0]), (float(o[1][0]), float(o[1][1]))) for o in outputs]


def _schedule(bm, steps, outputs, B):
    """`steps`: a number of steps of DT, or the per-step sizes; `outputs`: step numbers or (out_step, (w0, w1)) pairs, several of
    which may share a step (ys[j + 1] = w0 * y[out_step - 1] + w1 * y[out_step])."""
    from torchsde_amd import kernels as K
    sizes = np.full(steps, DT) if np.isscalar(steps) else np.asarray(steps, dtype=np.float64)
    grid = np.concatenate([[0.0], np.cumsum(sizes)])
    bm.adopt_grid(grid)
    cells = np.asarray(bm.match_grid(grid), dtype=np.int64)
    rows = np.zeros((len(sizes), 8))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = sizes, sizes / 2, 1 / sizes, np.sqrt(sizes)
    rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7] = np.sqrt(sizes), np.sqrt(sizes / 12), sizes, grid[:-1]
    pairs = _pairs(outputs)
    return K.TrajectorySchedule(rows, cells, [k for k, _ in pairs], [w for _, w in pairs], torch.device(DEV), torch.float32), grid


def _named(name):
    """Per-step sizes and (out_step, (w0, w1)) pairs of `helpers.RHEUN_GRIDS[name]` at this file's DT, from the solver's own grid
    builder."""
    grid = helpers.rheun_grid([u * DT for u in helpers.RHEUN_GRIDS[name]], DT)
    return np.asarray(grid.dt, dtype=np.float64), [(kc, (w0, w1)) for (_, kc, w0, w1) in grid.outputs]


def _reference(f, g, y0, bm, grid, outputs, noise, d, m):
    """methods/reversible_heun.py:48-73 in float64 on the generator's increments, recorded by autograd; an output inside a step
    mixes the states on either side of it (base_solver.py:147, interp.py:15-18)."""
    f64 = lambda net: net.rebuilt([t.double() for t in net.parameters()])                 # noqa: E731
    fd, gd = f64(f), f64(g)
    pairs = _pairs(outputs)

    def fg(t, z):
        tt = torch.tensor(t, dtype=torch.float64, device=DEV)
        gv = gd(tt, z)
        return fd(tt, z), (gv.reshape(z.shape[0], d, m) if noise == "general" else gv)

    def prod(gv, w):
        return torch.bmm(gv, w.unsqueeze(-1)).squeeze(-1) if noise == "general" else gv * w
    y = y0.double()
    z = y
    f0, g0 = fg(grid[0], z)
    ys = [y]
    for k in range(len(grid) - 1):
        dt = float(grid[k + 1]) - float(grid[k])
        dW = bm(float(grid[k]), float(grid[k + 1])).double()
        if noise == "scalar":
            dW = dW.expand(-1, d)
        z1 = 2 * y - z + f0 * dt + prod(g0, dW)
        f1, g1 = fg(grid[k + 1], z1)
        y_prev, y = y, y + (f0 + f1) * (0.5 * dt) + prod(g0 + g1, 0.5 * dW)
        z, f0, g0 = z1, f1, g1
        for step, (w0, w1) in pairs:
            if step == k + 1:
                ys.append(y if (w0, w1) == (0.0, 1.0) else w0 * y_prev + w1 * y)
    return torch.stack(ys), z


CASES = [
    # d, m, hidden, depth, act, final_f, final_g, noise, B
    (8, 3, 8, 2, "lipswish", "tanh", "tanh", "general", 40),          # examples/sde_gan.py:50-66,93-94 (num_layers = 1)
    (16, 3, 16, 3, "lipswish", "tanh", "tanh", "general", 33),         # ... num_layers = 2, the example's sizes
    (8, 16, 8, 2, "tanh", None, "sigmoid", "general", 24),             # tests/problems.py:226-252 (NeuralGeneral)
    (20, 7, 24, 4, "softplus", None, None, "general", 17),             # four Linear layers, channel counts between the tiles
    (32, 16, 64, 2, "softplus", None, "sigmoid", "general", 48),       # the BASELINE configs[2] shape
    (8, 8, 8, 2, "tanh", None, "sigmoid", "diagonal", 40),             # NeuralDiagonal
    (12, 12, 20, 3, "softplus", "tanh", None, "diagonal", 19),
    (6, 1, 8, 2, "tanh", None, "sigmoid", "scalar", 21),               # NeuralScalar
    (3, 2, 8, 2, "tanh", None, None, "general", 9),                    # rows that are not 16-byte groups
    # more than 32 state channels: the 64-channel instantiations (run-time row stride of the diffusion's last layer)
    (40, 4, 16, 2, "tanh", None, "sigmoid", "general", 20),
    (36, 12, 16, 3, "softplus", None, "tanh", "general", 18),
    (48, 48, 32, 2, "softplus", None, None, "diagonal", 18),
]


@pytest.mark.parametrize("d,m,hidden,depth,act,final_f,final_g,noise,B", CASES)
def test_forward_and_backward_against_a_float64_statement_of_the_reference(d, m, hidden, depth, act, final_f, final_g, noise, B):
    import torchsde_amd
    from torchsde_amd import _native, neural_rheun
    steps, outputs = 12, [5, 12]
    f, g = _nets(d, m, hidden, depth, act, final_f, final_g, noise, seed=d + m)
    code = {"general": _native.NOISE_GENERAL, "diagonal": _native.NOISE_DIAGONAL, "scalar": _native.NOISE_SCALAR}[noise]
    assert neural_rheun.lds_bytes(d, m, f, g, code) > 0
    bm = torchsde_amd.BrownianInterval(0.0, steps * DT, size=(B, m), dtype=torch.float32, device=DEV, entropy=5, dt=DT)
    schedule, grid = _schedule(bm, steps, outputs, B)
    gen = torch.Generator(device=DEV).manual_seed(1)
    y0 = (0.3 * torch.randn(B, d, device=DEV, generator=gen)).requires_grad_(True)
    weights = torch.randn(3, B, d, device=DEV, generator=gen)
    ys = neural_rheun.solve(y0, f, g, code, m, schedule, grid.astype(np.float32), bm)
    want, _ = _reference(f, g, y0, bm, grid, outputs, noise, d, m)
    scale = want.detach().abs().max().item()
    assert (ys.detach().double() - want.detach()).abs().max().item() <= 2e-5 * scale + 1e-6
    params = [y0] + f.parameters() + g.parameters()
    got = torch.autograd.grad((ys * weights).sum(), params)
    ref = torch.autograd.grad((want * weights.double()).sum(), params)
    for i, (a, b) in enumerate(zip(got, ref)):
        s = b.abs().max().item() + 1e-12
        err = (a.double() - b).abs().max().item()
        assert err <= 2e-4 * s + 1e-7, (i, tuple(a.shape), err, s)


def test_chunked_backward_sweep_equals_the_single_launch(monkeypatch):
    """The stash budget cuts the sweep into launches of a few evaluations each: same gradients, bit for bit in the state."""
    import torchsde_amd
    from torchsde_amd import _native, neural_rheun
    d, m, B, steps = 8, 3, 40, 16
    f, g = _nets(d, m, 8, 3, "lipswish", "tanh", "tanh", "general", seed=3)
    bm = torchsde_amd.BrownianInterval(0.0, steps * DT, size=(B, m), dtype=torch.float32, device=DEV, entropy=9, dt=DT)
    schedule, grid = _schedule(bm, steps, [4, 9, 16], B)
    y0 = torch.full((B, d), 0.2, device=DEV, requires_grad=True)
    params = [y0] + f.parameters() + g.parameters()
    results = []
    for budget in (neural_rheun.STASH_BYTES, 3 * B * neural_rheun._Stash.floats_per_row(d, m, f, g, True) * 4):
        monkeypatch.setattr(neural_rheun, "STASH_BYTES", budget)
        ys = neural_rheun.solve(y0, f, g, _native.NOISE_GENERAL, m, schedule, grid.astype(np.float32), bm)
        results.append(torch.autograd.grad((ys ** 2).sum(), params))
    assert torch.equal(results[0][0], results[1][0])
    for a, b in zip(results[0][1:], results[1][1:]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


# ---- the output map and the per-step sizes: what a kernel does with `out_step`, `out_w`, a short last step ---------------------
GRID_CASES = [CASES[0], CASES[6], CASES[7]]          # one general (8, 3), one diagonal (12, 12), the scalar one
NOISE = {"general": "NOISE_GENERAL", "diagonal": "NOISE_DIAGONAL", "scalar": "NOISE_SCALAR"}


def _solve_on(case, sizes, outputs, seed, grad=True):
    """(ys, the float64 statement's ys, the inputs a gradient is taken for, schedule pieces) of one case on one schedule."""
    import torchsde_amd
    from torchsde_amd import _native, neural_rheun
    d, m, hidden, depth, act, final_f, final_g, noise, B = case
    f, g = _nets(d, m, hidden, depth, act, final_f, final_g, noise, seed=d + m)
    code = getattr(_native, NOISE[noise])
    sizes = np.asarray(sizes, dtype=np.float64)
    bm = torchsde_amd.BrownianInterval(0.0, float(sizes.sum()), size=(B, m), dtype=torch.float32, device=DEV, entropy=seed)
    schedule, grid = _schedule(bm, sizes, outputs, B)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    y0 = (0.3 * torch.randn(B, d, device=DEV, generator=gen)).requires_grad_(grad)
    weights = torch.randn(len(outputs) + 1, B, d, device=DEV, generator=gen)

    def solve():
        return neural_rheun.solve(y0, f, g, code, m, schedule, grid.astype(np.float32), bm)
    want, _ = _reference(f, g, y0, bm, grid, outputs, noise, d, m)
    return solve, want, [y0] + f.parameters() + g.parameters(), weights


@pytest.mark.parametrize("name", ["inside", "crowded", "first_step", "ragged", "one_short_step"])
@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: f"{c[7]}-{c[0]}x{c[1]}")
def test_forward_values_over_output_maps(case, name):
    """Interpolated outputs (one, several in one step, against y0), a short last step, a single short step: values against the
    float64 statement, at the tolerance of the uniform schedule above."""
    sizes, outputs = _named(name)
    solve, want, _, _ = _solve_on(case, sizes, outputs, seed=21)
    with torch.no_grad():
        ys = solve()
    assert ys.shape == want.shape
    scale = want.detach().abs().max().item()
    err = (ys.double() - want.detach()).abs().max(dim=2)[0].max(dim=1)[0]
    print(name, case[7], "per-output error / scale:", " ".join(f"{e / scale:.2e}" for e in err.tolist()))
    assert err.max().item() <= 2e-5 * scale + 1e-6, (err.tolist(), scale)


BOUNDARY_SCHEDULES = {
    "ragged": lambda: _named("ragged"),
    "one_short_step": lambda: _named("one_short_step"),
    "every_step": lambda: _named("every_step"),
    "output_at_step_1": lambda: (np.full(16, DT), [1, 16]),
}


@pytest.mark.parametrize("name", sorted(BOUNDARY_SCHEDULES))
@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: f"{c[7]}-{c[0]}x{c[1]}")
def test_gradients_over_boundary_only_schedules(case, name):
    """The backward sweep with per-step sizes (a short last step, one short step), consecutive outputs, an output after the
    first step, and -- in every case -- a cotangent on ys[0]: gradients with respect to y0 and every weight against autograd
    through the float64 statement, at the tolerance of the uniform schedule above."""
    sizes, outputs = BOUNDARY_SCHEDULES[name]()
    solve, want, params, weights = _solve_on(case, sizes, outputs, seed=23)
    assert float(weights[0].abs().min()) > 0.0
    ys = solve()
    assert type(ys.grad_fn).__name__ == "ReversibleHeunFnBackward"
    scale = want.detach().abs().max().item()
    assert (ys.detach().double() - want.detach()).abs().max().item() <= 2e-5 * scale + 1e-6
    got = torch.autograd.grad((ys * weights).sum(), params)
    ref = torch.autograd.grad((want * weights.double()).sum(), params)
    for i, (a, b) in enumerate(zip(got, ref)):
        s = b.abs().max().item() + 1e-12
        err = (a.double() - b).abs().max().item()
        print(name, case[7], f"input {i}: error / scale {err / s:.2e}")
        assert err <= 2e-4 * s + 1e-7, (i, tuple(a.shape), err, s)


@pytest.mark.parametrize("evaluations", [1, 2, 3])
def test_chunked_backward_sweep_with_close_outputs_and_a_short_last_step(monkeypatch, evaluations):
    """Stash budgets of one, two and three evaluations per launch (a batch near the route's 2^30-element limit reaches one in
    production), outputs after steps 1, 2, 3 and the last, whose step is a quarter of the others: every launch finds its own
    outputs and step sizes. Same comparison as the test above."""
    import torchsde_amd
    from torchsde_amd import _native, neural_rheun
    d, m, B = 8, 3, 40
    sizes = np.concatenate([np.full(15, DT), [DT / 4]])
    f, g = _nets(d, m, 8, 3, "lipswish", "tanh", "tanh", "general", seed=3)
    bm = torchsde_amd.BrownianInterval(0.0, float(sizes.sum()), size=(B, m), dtype=torch.float32, device=DEV, entropy=9)
    schedule, grid = _schedule(bm, sizes, [1, 2, 3, 16], B)
    y0 = torch.full((B, d), 0.2, device=DEV, requires_grad=True)
    params = [y0] + f.parameters() + g.parameters()
    gen = torch.Generator(device=DEV).manual_seed(5)
    weights = torch.randn(5, B, d, device=DEV, generator=gen)
    results = []
    for budget in (neural_rheun.STASH_BYTES, evaluations * B * neural_rheun._Stash.floats_per_row(d, m, f, g, True) * 4):
        monkeypatch.setattr(neural_rheun, "STASH_BYTES", budget)
        ys = neural_rheun.solve(y0, f, g, _native.NOISE_GENERAL, m, schedule, grid.astype(np.float32), bm)
        results.append(torch.autograd.grad((ys * weights).sum(), params))
    assert torch.equal(results[0][0], results[1][0])
    for a, b in zip(results[0][1:], results[1][1:]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    # (and the single launch is right: against the float64 statement)
    want, _ = _reference(f, g, y0, bm, grid, [1, 2, 3, 16], "general", d, m)
    ref = torch.autograd.grad((want * weights.double()).sum(), params)
    for i, (a, b) in enumerate(zip(results[0], ref)):
        s = b.abs().max().item() + 1e-12
        assert (a.double() - b).abs().max().item() <= 2e-4 * s + 1e-7, (i, tuple(a.shape), s)


@pytest.mark.parametrize("name", ["inside", "crowded", "first_step"])
def test_an_interpolated_output_with_a_gradient_is_refused(name):
    """The backward sweep places an output's whole cotangent on its step (it never reads `out_w`): a schedule that interpolates
    is solved without a gradient only, and says so otherwise."""
    sizes, outputs = _named(name)
    for wants in ("y0", "weights", "both"):
        solve, want, params, _ = _solve_on(GRID_CASES[0], sizes, outputs, seed=29, grad=wants != "weights")
        for p in params[1:]:
            p.requires_grad_(wants != "y0")
        with pytest.raises(ValueError, match="step boundar"):
            solve()
        with torch.no_grad():
            ys = solve()
        assert ys.grad_fn is None and torch.isfinite(ys).all()
    for p in params:
        p.requires_grad_(False)
    ys = solve()                                                     # nothing requires a gradient: solved, grad mode or not
    want = want.detach()
    scale = want.abs().max().item()
    assert ys.grad_fn is None and (ys.double() - want).abs().max().item() <= 2e-5 * scale + 1e-6


@pytest.mark.parametrize("d,m,hidden,final,N", [(16, 3, 16, "tanh", 1000), (32, 16, 64, "sigmoid", 4099), (8, 5, 24, None, 77),
                                                 (3, 2, 8, "tanh", 16), (64, 16, 40, "sigmoid", 300)])
def test_last_layer_gradient_kernel_against_a_torch_statement(d, m, hidden, final, N):
    """``tsde_rheun_last_layer_grad``: dL/dW2, dL/db2 of a general diffusion net's last layer from stash rows (hid, p, q, wa, wb),
    against the (N, d m) cotangent formed in torch -- every tile path (outputs not a multiple of 16 or of the 256-output slice,
    rows not a multiple of 16, hidden between the tile widths, strides wider than the widths)."""
    from torchsde_amd import _native, neural_rheun
    f, g = _nets(d, m, hidden, 2, "tanh", None, final, "general", seed=N)
    gen = torch.Generator(device=DEV).manual_seed(N)
    pad = lambda n: (n + 3) // 4 * 4                                                      # noqa: E731
    mk = lambda w: torch.randn(N, pad(w), device=DEV, generator=gen)                      # noqa: E731
    hid, p, q, wa, wb = mk(hidden), mk(d), mk(d), mk(m), mk(m)
    acc_w = torch.zeros(d * m, hidden, device=DEV)
    acc_b = torch.zeros(d * m, device=DEV)
    neural_rheun._general_last_layer(g, acc_w, acc_b, hid, p, q, wa, wb, d, m)
    want_w, want_b = neural_rheun.general_last_layer_reference(
        g.rebuilt([t.double() for t in g.parameters()]), hid.double(), p.double(), q.double(), wa.double(), wb.double(), d, m)
    for got, want in ((acc_w, want_w), (acc_b, want_b)):
        scale = want.abs().max().item()
        assert (got.double() - want).abs().max().item() <= 2e-5 * scale + 1e-6, (got.shape, scale)
