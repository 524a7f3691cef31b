"""The activations and slopes the matrix-core kernels form, read back from ONE step against float64 (``-m gpu``).

The kernels evaluate tanh, softplus, LipSwish and the closing sigmoid / tanh with hand-written formulas on the raw hardware
transcendentals, at eleven places (tests/neural_activation_forms.py lists them). Here each place is driven through read-out networks
in which a sample x passes exactly one activation and reaches the output without another rounding: one step of dt = 1 from
t = 0, 0/1 weight matrices (every sum has one nonzero term, and 0 + v * 1 = v), zero diffusion where the drift is read.

  per row      state channels are inputs (they carry x) or outputs (they start at 0); W1 sends input i to hidden unit pi(i) --
               the padded last tile included --, W2 sends it on to output channel d - 1 - i:  y1[out] = act(x)
  per channel  closing functions and the perceptron's sigmoid diffusion: zero weights, the bias / shift carries x, one point
               per channel and launch; a diffusion is read as y1 = g(x) * dW against reference * dW on the same increments
  slopes       gradients through the same networks: L = sum of the output channels, dL/dy0[input] = act'(x); for a closing
               function and for q of `diffusion_value` the gradient with respect to the bias / shift, on ONE row (the kernels sum
               those over the batch)

Asserted: (a) every value and slope within `forms.bound(site, quantity)` = 2 E_form + 2^-24 in the measure |got - ref| /
max(1, |ref|); (b) nothing is NaN or infinite anywhere on the grid; (c) tanh and softplus values are bit-equal across every user of
`activate` / `activate_with_slope`; (d) with dyadic x every output holds the value of its OWN input.

Two sample points cannot travel through a STATE: reversible Heun forms 2 y - z, which overflows at |x| = 3e38 whatever the
activation does; the deep-network values at those two points are read through the same kernel's Euler scheme, their slopes not at
all. Two quantities are formed by a kernel and isolated by no read-out: in the adjoint's own sigmoid diffusion (mlp_adjoint.hip)
q' = q (1 - 2 s) and the g it subtracts when it reconstructs the state -- both reach the outputs only in products with the rate c,
and with c = 0 (which makes the argument exactly x) they drop out; its q is read. A Milstein slope can be recovered only where
g (x) is not zero in float32: at the other points (tanh below 2^-25, softplus and sigmoid below -104) the step is asserted to
be exactly zero instead."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import neural_activation_forms as forms

pytestmark = pytest.mark.gpu
DEV = "cuda"
X = forms.sample_grid()
REF = forms.reference(X)
for _v in REF.values():
    _v.setflags(write=False)
ACTS = {"tanh": 0, "softplus": 1, "lipswish": 2}
MEASURED = {}                              # (site, quantity) -> [(what, x, error per point)]: tools/neural_activation_accuracy.py


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)             # (a copy: the grid is read-only)


def _bm(rows, m, entropy=11):
    import torchsde_amd
    return torchsde_amd.BrownianInterval(0.0, 1.0, size=(rows, m), dtype=torch.float32, device=DEV, entropy=entropy)


def _one_step(bm):
    from torchsde_amd import kernels as K
    grid = np.array([0.0, 1.0])
    bm.adopt_grid(grid)
    cells = np.asarray(bm.match_grid(grid), dtype=np.int64)
    rows = np.array([[1.0, 0.5, 1.0, 1.0, 1.0, math.sqrt(1.0 / 12.0), 1.0, 0.0]])
    return K.TrajectorySchedule(rows, cells, [1], [(0.0, 1.0)], torch.device(DEV), torch.float32)


class ReadOut:
    """The per-row read-out network of a (d, hidden) shape."""

    def __init__(self, d, hidden):
        self.d, self.hidden, self.n = d, hidden, d // 2
        step = max(1, hidden // self.n)
        self.ins = list(range(self.n))
        self.pi = [hidden - 1 - i * step for i in self.ins]           # (from the last unit down: the padded tile is used)
        self.outs = [d - 1 - i for i in self.ins]                     # (reversed: a neighbour's value would show)
        assert len(set(self.pi)) == self.n and min(self.pi) >= 0 and min(self.outs) >= self.n
        self.w1 = np.zeros((d, hidden), dtype=np.float32)             # input-major, as the kernels read it
        self.w2 = np.zeros((hidden, d), dtype=np.float32)
        for i in self.ins:
            self.w1[i, self.pi[i]] = 1.0
            self.w2[self.pi[i], self.outs[i]] = 1.0

    def pack(self, x):
        rows = -(-len(x) // self.n)
        y0 = np.zeros((rows, self.d), dtype=np.float32)
        y0[:, :self.n] = np.resize(x, rows * self.n).reshape(rows, self.n)
        return y0

    def unpack(self, y, count, channels=None):
        return np.ascontiguousarray(y[:, self.outs if channels is None else channels]).reshape(-1)[:count]


def _dyadic(count):
    """`count` distinct dyadic points within +-4: multiples of 1/32, or of the power of two that fits them in."""
    denominator = max(32, 1 << int(math.ceil(math.log2(count / 8.0))))
    return ((np.arange(count) - count // 2) / float(denominator)).astype(np.float32)


# ---- the five per-row routes: each returns {"value": (N,), "slope": (N,) or None, "y1": the whole final state} ---------------------
def _perceptron_module(ro, act):
    import torchsde_amd
    sde = torchsde_amd.MLPDriftDiagonalSDE(ro.d, ro.hidden, activation=act, diff_rate=0.0, diff_shift=0.0).to(DEV)
    with torch.no_grad():
        sde.lin1.weight.copy_(_dev(ro.w1.T))
        sde.lin2.weight.copy_(_dev(ro.w2.T))
        sde.lin1.bias.zero_()
        sde.lin2.bias.zero_()
    return sde


def _run_perceptron_sampling(ro, act, x):
    from torchsde_amd import kernels as K
    y0 = _dev(ro.pack(x))
    bm = _bm(y0.shape[0], ro.d)
    zeros = torch.zeros(ro.d, device=DEV)
    ys = torch.empty(1, *y0.shape, device=DEV)
    K.trajectory_mlp_diag(ys, y0, _dev(ro.w1), torch.zeros(ro.hidden, device=DEV), _dev(ro.w2), zeros, zeros, zeros.clone(),
                          ACTS[act], (0, 1.0), 0, _one_step(bm), bm)
    return ys[0].cpu().numpy(), None


def _run_perceptron_gradient(ro, act, x, adjoint):
    import torchsde_amd
    sde = _perceptron_module(ro, act)
    y0 = _dev(ro.pack(x)).requires_grad_(True)
    bm = _bm(y0.shape[0], ro.d)
    ts = torch.tensor([0.0, 1.0], device=DEV)
    if adjoint:
        ys = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method="euler", adjoint_method="euler", dt=1.0)
        assert type(ys.grad_fn).__name__.startswith("_MlpAdjointFn"), "the matrix-core adjoint was not taken"
    else:
        ys = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method="euler", dt=1.0, options={"trajectory_kernel": True})
        assert "MlpTrajectoryFn" in type(ys.grad_fn).__name__, "the training kernel was not taken"
    ys[-1][:, ro.outs].sum().backward()
    return ys[-1].detach().cpu().numpy(), y0.grad.cpu().numpy()


def _run_general(ro, act, x):
    from torchsde_amd import _native, kernels as K
    y0 = _dev(ro.pack(x))
    bm = _bm(y0.shape[0], ro.d)
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    fnet = K.NeuralNet(_dev(ro.w1), None, z(ro.hidden), _dev(ro.w2), z(ro.d), ACTS[act])
    gnet = K.NeuralNet(z(ro.d, ro.hidden), None, z(ro.hidden), z(ro.hidden, ro.d), z(ro.d), ACTS[act])
    ys = torch.empty(1, *y0.shape, device=DEV)
    K.trajectory_mlp_general(ys, y0, fnet, gnet, _native.NOISE_DIAGONAL, ro.d, _native.TRAJ_EULER, _one_step(bm), bm)
    return ys[0].cpu().numpy(), None


def _deep_nets(d, hidden, act, w1, w2, b2=None, final=0):
    """(drift, diffusion) of the deep-network kernels, depth 2; the diffusion is identically zero."""
    from torchsde_amd.neural_rheun import DeepNet
    c = float(forms.LIPSWISH_C) if act == "lipswish" else 1.0
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    b2 = z(d) if b2 is None else b2
    f = DeepNet([(_dev(w1.T), z(hidden)), (_dev(w2.T), b2)], ACTS[act], c, final, 1.0, False)
    g = DeepNet([(z(hidden, d), z(hidden)), (z(d, hidden), z(d))], ACTS[act], c, 0, 1.0, False)
    return f, g


def _run_deep(ro, act, x, euler):
    from torchsde_amd import _native, neural_rheun
    y0 = _dev(ro.pack(x))
    bm = _bm(y0.shape[0], ro.d)
    f, g = _deep_nets(ro.d, ro.hidden, act, ro.w1, ro.w2)
    schedule = _one_step(bm)
    times = np.array([0.0, 1.0], dtype=np.float32)
    if euler:
        ys, z_out = torch.empty(1, *y0.shape, device=DEV), torch.empty_like(y0)
        neural_rheun.forward(ys, z_out, y0, f, g, _native.NOISE_DIAGONAL, ro.d, schedule, torch.from_numpy(times).to(DEV), bm,
                             method=_native.TRAJ_EULER)
        return ys[0].cpu().numpy(), None
    y0.requires_grad_(True)
    ys = neural_rheun.solve(y0, f, g, _native.NOISE_DIAGONAL, ro.d, schedule, times, bm)
    (grad,) = torch.autograd.grad(ys[-1][:, ro.outs].sum(), y0)
    return ys[-1].detach().cpu().numpy(), grad.cpu().numpy()


ROUTES = {
    # route: (runner, site of its values, site of its slopes, activations)
    "perceptron_sampling": (_run_perceptron_sampling, "activate", None, ("tanh", "softplus")),
    "perceptron_training": (functools.partial(_run_perceptron_gradient, adjoint=False), "activate", "activate_with_slope",
                            ("tanh", "softplus")),
    "perceptron_adjoint": (functools.partial(_run_perceptron_gradient, adjoint=True), "activate", "activate_with_slope",
                           ("tanh", "softplus")),
    "mlp_general": (_run_general, "activate", None, ("tanh", "softplus")),
    "deep_euler": (functools.partial(_run_deep, euler=True), "hidden_act", None, ("tanh", "softplus", "lipswish")),
    "deep_rheun": (functools.partial(_run_deep, euler=False), "hidden_act", "hidden_act", ("tanh", "softplus", "lipswish")),
}
PERCEPTRON_SHAPES, GENERAL_SHAPES, DEEP_SHAPES = [(16, 16), (20, 36)], [(16, 16), (12, 24), (63, 32)], [(16, 16), (20, 24)]
SHAPES = {"perceptron_sampling": PERCEPTRON_SHAPES, "perceptron_training": PERCEPTRON_SHAPES,
          "perceptron_adjoint": PERCEPTRON_SHAPES, "mlp_general": GENERAL_SHAPES, "deep_euler": DEEP_SHAPES,
          "deep_rheun": DEEP_SHAPES}
CASES = [(route, d, h, act) for route in ROUTES for d, h in SHAPES[route] for act in ROUTES[route][3]]
STATE_SAFE = np.abs(X) < 1e38              # (2 y - z of reversible Heun overflows beyond: see the head of this file)


def _points(route):
    return X[STATE_SAFE] if route == "deep_rheun" else X


def _reference(route, quantity):
    return REF[quantity][STATE_SAFE] if route == "deep_rheun" else REF[quantity]


@functools.lru_cache(maxsize=None)
def _per_row(route, d, hidden, act, dyadic=False):
    ro = ReadOut(d, hidden)
    x = _dyadic(20 * ro.n) if dyadic else _points(route)
    y1, grad = ROUTES[route][0](ro, act, x)
    out = {"x": x, "y1": y1, "value": ro.unpack(y1, len(x)), "slope": None if grad is None else ro.unpack(grad, len(x), ro.ins),
           "ro": ro, "grad": grad}
    return out


def _check(got, ref, site, quantity, x, what):
    """(a) and (b) for one array of read-outs; every figure is printed before it is asserted."""
    err = forms.measure(got, ref)
    MEASURED.setdefault((site, quantity), []).append((what, x, err))
    worst = int(np.argmax(err))
    print(f"{what}: {site}.{quantity} worst {err[worst]:.3e} at x = {x[worst]!r} (bound {forms.bound(site, quantity):.3e}, "
          f"E_form {forms.E_form(site, quantity):.3e})")
    assert np.all(np.isfinite(got)), (what, x[~np.isfinite(got)][:8])
    assert err[worst] <= forms.bound(site, quantity), (what, site, quantity, float(err[worst]), float(x[worst]),
                                                       forms.bound(site, quantity))


@pytest.mark.parametrize("route,d,hidden,act", CASES)
def test_hidden_activation_values_and_slopes_against_float64(route, d, hidden, act):
    run = _per_row(route, d, hidden, act)
    _, value_site, slope_site, _ = ROUTES[route]
    assert np.all(np.isfinite(run["y1"])) and (run["grad"] is None or np.all(np.isfinite(run["grad"])))           # (b)
    _check(run["value"], _reference(route, f"{act}.value"), value_site, f"{act}.value", run["x"], f"{route} ({d}, {hidden})")
    if slope_site is not None:
        _check(run["slope"], _reference(route, f"{act}.slope"), slope_site, f"{act}.slope", run["x"], f"{route} ({d}, {hidden})")


@pytest.mark.parametrize("act", ["tanh", "softplus"])
def test_every_user_of_activate_returns_the_same_bits(act):
    """(c): `activate` (perceptron sampling, which is also the forward pass of training; mlp_general) and `activate_with_slope`
    (the deep networks through `hidden_act`; the perceptron's reverse sweep and adjoint, whose recomputed hidden values reach
    dL/dW2) state one formula and must return one value."""
    want = _per_row("perceptron_sampling", 16, 16, act)["value"]
    for route, d, hidden, a in CASES:
        if a != act or route == "deep_rheun":
            continue
        got = _per_row(route, d, hidden, act)["value"]
        differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert differ.size == 0, (route, d, hidden, X[differ][:8], got[differ][:8], want[differ][:8])
    safe = _per_row("deep_rheun", 16, 16, act)["value"]
    assert np.array_equal(safe.view(np.uint32), want[STATE_SAFE].view(np.uint32))
    for adjoint in (False, True):
        got = _recomputed_hidden_values(act, adjoint)
        differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert differ.size == 0, ("adjoint" if adjoint else "training", X[differ][:8], got[differ][:8], want[differ][:8])


@functools.lru_cache(maxsize=None)
def _recomputed_hidden_values(act, adjoint):
    """The hidden values the perceptron's reverse sweep (`adjoint`: its stochastic adjoint) recomputes with
    `activate_with_slope`, read through dL/dW2 = sum over rows of lam (x) hid: row i has the cotangent 1 in ONE output channel
    (n + i), so that entry (n + i, pi(j)) of the gradient is hid[i, pi(j)] = act(x[i, j]) plus zeros. (64, 128): the whole grid
    in one launch."""
    import torchsde_amd
    d, hidden, n = 128, 128, 64
    assert len(X) <= n * n
    ro = ReadOut(d, hidden)
    sde = _perceptron_module(ro, act)
    y0n = np.zeros((n, d), dtype=np.float32)
    y0n[:, :n] = np.resize(X, n * n).reshape(n, n)
    y0 = _dev(y0n)
    bm = _bm(n, d)
    ts = torch.tensor([0.0, 1.0], device=DEV)
    if adjoint:
        ys = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method="euler", adjoint_method="euler", dt=1.0)
        assert type(ys.grad_fn).__name__.startswith("_MlpAdjointFn")
    else:
        ys = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method="euler", dt=1.0, options={"trajectory_kernel": True})
        assert "MlpTrajectoryFn" in type(ys.grad_fn).__name__
    rows = torch.arange(n, device=DEV)
    ys[-1][rows, n + rows].sum().backward()
    grad = sde.lin2.weight.grad.cpu().numpy()                       # (d, hidden)
    assert np.all(np.isfinite(grad))
    return np.ascontiguousarray(grad[n:2 * n][:, ro.pi]).reshape(-1)[:len(X)]


@pytest.mark.parametrize("route,d,hidden,act", CASES)
def test_each_output_holds_the_value_of_its_own_input(route, d, hidden, act):
    """(d): distinct dyadic samples within +-4, 1/32 apart (1/128 at 63 channels): a neighbour's value differs by at least
    tanh'(4) / 128 = 1e-5, twenty-five bounds; input channels pass through the step unchanged and channels that are neither stay
    exactly zero."""
    run = _per_row(route, d, hidden, act, dyadic=True)
    ro, x = run["ro"], run["x"]
    assert np.abs(x).max() <= 4.0 and len(np.unique(x)) == len(x)
    ref = forms.reference(x)
    value_site, slope_site = ROUTES[route][1], ROUTES[route][2]
    assert forms.measure(run["value"], ref[f"{act}.value"]).max() <= forms.bound(value_site, f"{act}.value")
    assert np.array_equal(run["y1"][:, ro.ins], ro.pack(x)[:, ro.ins])
    unused = [c for c in range(d) if c not in ro.ins and c not in ro.outs]
    assert np.all(run["y1"][:, unused] == 0.0)
    if slope_site is not None:
        assert forms.measure(run["slope"], ref[f"{act}.slope"]).max() <= forms.bound(slope_site, f"{act}.slope")
        assert np.all(run["grad"][:, ro.outs] == 1.0) and np.all(run["grad"][:, unused] == 0.0)


# ---- per channel: closing functions and the perceptron's sigmoid diffusion -----------------------------------------------------------
def _chunks(width):
    """The grid in pieces of `width` samples (the last one padded with its first sample)."""
    for lo in range(0, len(X), width):
        piece = X[lo:lo + width]
        yield lo, len(piece), np.resize(piece, width).astype(np.float32)


def _check_times_dw(y1, dw, ref, site, quantity, what):
    """y1 (rows, N) = g(x) * dW against reference * dW: the bound times |dW|, and half an ulp of y1 for the product."""
    got, dw = y1.astype(np.float64), dw.astype(np.float64)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - ref[None, :] * dw)
    allowed = forms.bound(site, quantity) * np.abs(dw) * np.maximum(1.0, np.abs(ref))[None, :] + 0.5 * np.spacing(np.abs(y1))
    ratio = err / allowed
    with np.errstate(divide="ignore", invalid="ignore"):
        per_point = np.where(dw != 0.0, err / np.abs(dw), 0.0).max(axis=0) / np.maximum(1.0, np.abs(ref))
    MEASURED.setdefault((site, quantity), []).append((what + " (through * dW)", X, per_point))
    r, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what}: {site}.{quantity} worst error / allowed {ratio[r, k]:.3f} at x = {X[k]!r}, dW = {dw[r, k]:.3f}")
    assert ratio[r, k] <= 1.0, (what, float(X[k]), float(err[r, k]), float(allowed[r, k]))


def test_perceptron_sigmoid_diffusion_value():
    """`diffusion_value` in the sampling kernel: g = 1 * sigmoid(1 * 0 + x), y1 = g * dW."""
    from torchsde_amd import kernels as K
    d, hidden, rows = 128, 16, 16
    bm = _bm(rows, d)
    schedule = _one_step(bm)
    dw_all = bm(0.0, 1.0).cpu().numpy()
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    y1, dw = np.zeros((rows, len(X)), dtype=np.float32), np.zeros((rows, len(X)), dtype=np.float32)
    for lo, count, piece in _chunks(d):
        ys = torch.empty(1, rows, d, device=DEV)
        K.trajectory_mlp_diag(ys, z(rows, d), z(d, hidden), z(hidden), z(hidden, d), z(d), torch.ones(d, device=DEV), _dev(piece),
                              0, (1, 1.0), 0, schedule, bm)
        y1[:, lo:lo + count], dw[:, lo:lo + count] = ys[0].cpu().numpy()[:, :count], dw_all[:, :count]
    _check_times_dw(y1, dw, REF["sigmoid.value"], "diffusion_value", "sigmoid.value", "perceptron sampling, sigmoid diffusion")


@pytest.mark.parametrize("adjoint", [False, True], ids=["reverse_sweep", "adjoint"])
def test_perceptron_sigmoid_diffusion_slope_q(adjoint):
    """q = g (1 - s) on ONE row: dL/d diff_shift[j] = (1 * dW_j) * q_j. Autograd through `sdeint` reaches `diffusion_value` in the
    reverse sweep (mlp_backward.hip); `sdeint_adjoint` reaches the adjoint kernel's OWN statement of the sigmoid diffusion
    (mlp_adjoint.hip), which evaluates it at the state it reconstructs, y1 = g dW: there the rate is 0, so that its argument
    0 * y1 + x is x exactly (and the terms with q' and the Ito correction, which carry the rate, are exactly 0). g is read
    through y1 of the same solve."""
    import torchsde_amd
    d, hidden = 128, 16
    ts = torch.tensor([0.0, 1.0], device=DEV)
    got, dw, y1 = (np.zeros((1, len(X)), dtype=np.float32) for _ in range(3))
    rate = torch.zeros(d) if adjoint else torch.ones(d)
    site = "adjoint_diffusion" if adjoint else "diffusion_value"
    for lo, count, piece in _chunks(d):
        sde = torchsde_amd.MLPDriftDiagonalSDE(d, hidden, activation="tanh", diff_rate=rate, diff_shift=_dev(piece).cpu(),
                                               diffusion="sigmoid", diff_scale=1.0).to(DEV)
        with torch.no_grad():
            for p in (sde.lin1.weight, sde.lin1.bias, sde.lin2.weight, sde.lin2.bias):
                p.zero_()
        bm = _bm(1, d)
        y0 = torch.zeros(1, d, device=DEV, requires_grad=True)
        if adjoint:
            ys = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method="euler", adjoint_method="euler", dt=1.0)
            assert type(ys.grad_fn).__name__.startswith("_MlpAdjointFn"), "the matrix-core adjoint was not taken"
        else:
            ys = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method="euler", dt=1.0, options={"trajectory_kernel": True})
            assert "MlpTrajectoryFn" in type(ys.grad_fn).__name__
        ys[-1].sum().backward()
        got[0, lo:lo + count] = sde.diff_shift.grad.cpu().numpy()[:count]
        y1[0, lo:lo + count] = ys[-1].detach().cpu().numpy()[0, :count]
        dw[0, lo:lo + count] = bm(0.0, 1.0).cpu().numpy()[0, :count]
    what = "perceptron adjoint" if adjoint else "perceptron reverse sweep"
    _check_times_dw(y1, dw, REF["sigmoid.value"], "diffusion_value", "sigmoid.value", what + ", g of the forward solve")
    _check_times_dw(got, dw, REF["sigmoid.slope"], site, "sigmoid.slope", what + ", q")


@pytest.mark.parametrize("noise", ["diagonal", "scalar"])
def test_mlp_general_closing_sigmoid(noise):
    """`finalise<true>`: zero weights, b2 carries x, y1 = sigmoid(x) * dW (scalar noise: one increment per row)."""
    from torchsde_amd import _native, kernels as K
    d, hidden, rows = 64, 16, 16
    m = d if noise == "diagonal" else 1
    bm = _bm(rows, m)
    schedule = _one_step(bm)
    dw_all = np.broadcast_to(bm(0.0, 1.0).cpu().numpy(), (rows, d))
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    fnet = K.NeuralNet(z(d, hidden), None, z(hidden), z(hidden, d), z(d), 0)
    y1, dw = np.zeros((rows, len(X)), dtype=np.float32), np.zeros((rows, len(X)), dtype=np.float32)
    for lo, count, piece in _chunks(d):
        gnet = K.NeuralNet(z(d, hidden), None, z(hidden), z(hidden, d), _dev(piece), 0, _native.FINAL_SIGMOID, 1.0)
        ys = torch.empty(1, rows, d, device=DEV)
        K.trajectory_mlp_general(ys, z(rows, d), fnet, gnet, _native.NOISE_DIAGONAL if noise == "diagonal" else _native.NOISE_SCALAR,
                                 m, _native.TRAJ_EULER, schedule, bm)
        y1[:, lo:lo + count], dw[:, lo:lo + count] = ys[0].cpu().numpy()[:, :count], dw_all[:, :count]
    _check_times_dw(y1, dw, REF["sigmoid.value"], "finalise", "sigmoid.value", f"mlp_general, {noise} noise, closing sigmoid")


@pytest.mark.parametrize("d,m", [(32, 8), (12, 4), (16, 16)])
def test_mlp_general_staged_bias_sigmoid(d, m):
    """General noise: the bias is staged as -log2(e) * b2 and enters exp2 through one fma. Output (c, j(c)) of the diffusion net
    has the bias x, every other output of the row -200 -- the kernel's sigmoid of that is exactly 0 -- so y1[c] = sigmoid(x) *
    dW[j(c)]."""
    from torchsde_amd import _native, kernels as K
    hidden, rows = 16, 16
    bm = _bm(rows, m)
    schedule = _one_step(bm)
    dw_all = bm(0.0, 1.0).cpu().numpy()                                   # (rows, m)
    j_of = np.array([(3 * c + 1) % m for c in range(d)])
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    fnet = K.NeuralNet(z(d, hidden), None, z(hidden), z(hidden, d), z(d), 0)
    y1, dw = np.zeros((rows, len(X)), dtype=np.float32), np.zeros((rows, len(X)), dtype=np.float32)
    for lo, count, piece in _chunks(d):
        b2 = np.full((d, m), -200.0, dtype=np.float32)
        b2[np.arange(d), j_of] = piece
        gnet = K.NeuralNet(z(d, hidden), None, z(hidden), z(hidden, d * m), _dev(b2.reshape(-1)), 0, _native.FINAL_SIGMOID, 1.0)
        ys = torch.empty(1, rows, d, device=DEV)
        K.trajectory_mlp_general(ys, z(rows, d), fnet, gnet, _native.NOISE_GENERAL, m, _native.TRAJ_EULER, schedule, bm)
        y1[:, lo:lo + count], dw[:, lo:lo + count] = ys[0].cpu().numpy()[:, :count], dw_all[:, j_of[:count]]
    _check_times_dw(y1, dw, REF["sigmoid.value"], "staged_bias", "sigmoid.value", f"mlp_general, general noise ({d}, {m})")


@pytest.mark.parametrize("final", ["sigmoid", "tanh"])
def test_deep_network_closing_functions_and_their_slopes(final):
    """`final_act` of the deep-network kernels: the drift's last layer has zero weights and the bias x, so that reversible Heun
    gives y1 = f/2 + f/2 = final(x); its slope is dL/db2 = s/2 + s/2 on ONE row (two evaluations, cotangent 1/2 each)."""
    from torchsde_amd import _native, neural_rheun
    d, hidden = 64, 16
    code = {"sigmoid": _native.FINAL_SIGMOID, "tanh": _native.FINAL_TANH}[final]
    bm = _bm(1, d)
    schedule = _one_step(bm)
    times = np.array([0.0, 1.0], dtype=np.float32)
    value, slope = np.zeros(len(X), dtype=np.float32), np.zeros(len(X), dtype=np.float32)
    zero = np.zeros((d, hidden), dtype=np.float32)
    for lo, count, piece in _chunks(d):
        b2 = _dev(piece).requires_grad_(True)
        f, g = _deep_nets(d, hidden, "tanh", zero, zero.T, b2=b2, final=code)
        ys = neural_rheun.solve(torch.zeros(1, d, device=DEV), f, g, _native.NOISE_DIAGONAL, d, schedule, times, bm)
        (grad,) = torch.autograd.grad(ys[-1].sum(), b2)
        value[lo:lo + count], slope[lo:lo + count] = ys[-1].detach().cpu().numpy()[0, :count], grad.cpu().numpy()[:count]
    _check(value, REF[f"{final}.value"], "final_act", f"{final}.value", X, "deep networks, closing function")
    _check(slope, REF[f"{final}.slope"], "final_act", f"{final}.slope", X, "deep networks, closing function")


@pytest.mark.parametrize("final", ["sigmoid", "tanh"])
def test_deep_network_general_noise_closing_slopes(final):
    """`final_slope` of csrc/rheun_grad.hip, the closing slopes stated once more for dL/dW2 and dL/db2 of a GENERAL-noise
    diffusion net: `tsde_rheun_last_layer_grad` on a stash of ONE row with p = 1, q = 0, wa = 1, wb = 0 and zero hidden values, so
    that the cotangent of output o is (1 * 1 + 0 * 0) * final'(0 + b2[o]) and dL/db2[o] = final'(x) plus zeros."""
    from torchsde_amd import _native, neural_rheun
    d, m, hidden = 16, 16, 16
    out = d * m
    code = {"sigmoid": _native.FINAL_SIGMOID, "tanh": _native.FINAL_TANH}[final]
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    hid, p, q, wa, wb = z(1, hidden), torch.ones(1, d, device=DEV), z(1, d), torch.ones(1, m, device=DEV), z(1, m)
    slope = np.zeros(len(X), dtype=np.float32)
    for lo, count, piece in _chunks(out):
        net = neural_rheun.DeepNet([(z(hidden, d), z(hidden)), (z(out, hidden), _dev(piece))], 0, 1.0, code, 1.0, False)
        acc_w, acc_b = z(out, hidden), z(out)
        neural_rheun._general_last_layer(net, acc_w, acc_b, hid, p, q, wa, wb, d, m)
        assert not acc_w.any()
        slope[lo:lo + count] = acc_b.cpu().numpy()[:count]
    _check(slope, REF[f"{final}.slope"], "final_slope", f"{final}.slope", X, "deep networks, general noise, last-layer gradient")


# ---- Milstein on mlp_general: slopes that cannot be isolated exactly ------------------------------------------------------------
def _milstein(fnet_zero, gnet, d, rows, bm, schedule):
    from torchsde_amd import _native, kernels as K
    ys = torch.empty(1, rows, d, device=DEV)
    K.trajectory_mlp_general(ys, torch.zeros(rows, d, device=DEV), fnet_zero, gnet, _native.NOISE_DIAGONAL, d,
                             _native.TRAJ_MILSTEIN_ITO, schedule, bm)
    return ys[0].cpu().numpy().astype(np.float64)


def _check_recovered_slope(y1, g, dw, ref, site, quantity, what, width, gdw=None):
    """y1 = g dW + (g/2) g' (dW^2 - 1): g' recovered in float64 from the kernel's own y1 and g (rows, N) on the rows with
    |dW^2 - 1| >= 1/2; the bound gains 2^-23 |y1| / |(g/2) (dW^2 - 1)| for the roundings of the step itself and nothing else.
    `gdw`: the kernel's own product g dW where that is what was read (an Euler step of the same net), subtracted as it is.
    A point whose g is zero in float32 admits no row (there is nothing to divide by): its step must be exactly zero."""
    gdw = g * dw if gdw is None else gdw
    v = dw * dw - 1.0
    half = 0.5 * g * v
    # (softplus(3e38) = 3e38 times an increment above 1.13 is no float32: the step overflows there, not the activation -- and
    #  the infinity then meets the zeros of the 0/1 matrices in the products back through the net: a row of a launch counts only
    #  where the step of EVERY channel of that launch is a float32)
    representable = np.abs(g * dw) + np.abs(half * ref[None, :]) < 3.0e38
    for lo in range(0, representable.shape[1], width):
        representable[:, lo:lo + width] = representable[:, lo:lo + width].all(axis=1, keepdims=True)
    assert np.all(np.isfinite(y1[representable])), what
    admitted = (np.abs(v) >= 0.5) & (half != 0.0) & representable
    no_g = np.all(g == 0.0, axis=0)
    assert np.all(admitted.any(axis=0) | no_g), (what, X[~(admitted.any(axis=0) | no_g)][:8])
    assert np.all(y1[:, no_g][representable[:, no_g]] == 0.0), what
    print(f"{what}: {int(no_g.sum())} of {len(no_g)} points have g = 0 in float32 (no slope to recover, step exactly 0)")
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (y1 - gdw) / half
        allowed = forms.bound(site, quantity) * np.maximum(1.0, np.abs(ref))[None, :] + 2.0 ** -23 * np.abs(y1) / np.abs(half)
        ratio = np.where(admitted, np.abs(slope - ref[None, :]) / np.where(admitted, allowed, 1.0), 0.0)
        per_point = np.where(admitted, np.abs(slope - ref[None, :]), 0.0).max(axis=0) / np.maximum(1.0, np.abs(ref))
        per_point = np.where(admitted.any(axis=0), per_point, np.nan)          # (not measured: "-" in the table)
    MEASURED.setdefault((site, quantity), []).append((what + " (recovered from a Milstein step)", X, per_point))
    r, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what}: {site}.{quantity} worst error / allowed {ratio[r, k]:.3f} at x = {X[k]!r}, dW = {dw[r, k]:.3f}")
    assert ratio[r, k] <= 1.0, (what, float(X[k]), float(slope[r, k]), float(ref[k]), float(allowed[r, k]))


@pytest.mark.parametrize("act", ["tanh", "softplus"])
def test_mlp_general_milstein_hidden_slopes(act):
    """`diffusion_hidden_with_slope`: channel c feeds hidden unit pi(c) whose bias is x and which feeds channel c back, so
    g = act(x) and dg/dy = act'(x): the slope forms 1 - v^2 and ex * rcp(1 + ex) of the Milstein instantiation."""
    from torchsde_amd import _native, kernels as K
    d, hidden, rows = 32, 32, 16
    bm = _bm(rows, d)
    schedule = _one_step(bm)
    dw_all = bm(0.0, 1.0).cpu().numpy().astype(np.float64)
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    fnet = K.NeuralNet(z(d, hidden), None, z(hidden), z(hidden, d), z(d), 0)
    pi = [(hidden - 1 - c) for c in range(d)]
    w1, w2 = np.zeros((d, hidden), dtype=np.float32), np.zeros((hidden, d), dtype=np.float32)
    w1[np.arange(d), pi], w2[pi, np.arange(d)] = 1.0, 1.0
    y1, g, dw = (np.zeros((rows, len(X))) for _ in range(3))
    for lo, count, piece in _chunks(d):
        b1 = np.zeros(hidden, dtype=np.float32)
        b1[pi] = piece
        gnet = K.NeuralNet(_dev(w1), None, _dev(b1), _dev(w2), z(d), ACTS[act])
        y1[:, lo:lo + count], dw[:, lo:lo + count] = _milstein(fnet, gnet, d, rows, bm, schedule)[:, :count], dw_all[:, :count]
    # the kernel's own g: the Euler read-out of the same formula (bit-equal across users, asserted above)
    g[:] = _per_row("mlp_general", 16, 16, act)["value"].astype(np.float64)[None, :]
    _check_recovered_slope(y1, g, dw, REF[f"{act}.slope"], "milstein_hidden", f"{act}.slope", f"mlp_general Milstein, {act}", d)


def test_mlp_general_milstein_closing_sigmoid_slope():
    """`diffusion_values_with_slope`: channel c feeds a tanh unit with bias 0 (value tanh(0) = 0, slope exactly 1) which feeds
    output c, whose bias is x: g = sigmoid(x), dg/dy = (1 * s) (1 - s)."""
    from torchsde_amd import _native, kernels as K
    d, hidden, rows = 32, 32, 16
    bm = _bm(rows, d)
    schedule = _one_step(bm)
    dw_all = bm(0.0, 1.0).cpu().numpy().astype(np.float64)
    z = lambda *shape: torch.zeros(*shape, device=DEV)                                            # noqa: E731
    fnet = K.NeuralNet(z(d, hidden), None, z(hidden), z(hidden, d), z(d), 0)
    pi = [(hidden - 1 - c) for c in range(d)]
    w1, w2 = np.zeros((d, hidden), dtype=np.float32), np.zeros((hidden, d), dtype=np.float32)
    w1[np.arange(d), pi], w2[pi, np.arange(d)] = 1.0, 1.0
    y1, g, dw, gdw = (np.zeros((rows, len(X))) for _ in range(4))
    for lo, count, piece in _chunks(d):
        gnet = K.NeuralNet(_dev(w1), None, z(hidden), _dev(w2), _dev(piece), 0, _native.FINAL_SIGMOID, 1.0)
        y1[:, lo:lo + count], dw[:, lo:lo + count] = _milstein(fnet, gnet, d, rows, bm, schedule)[:, :count], dw_all[:, :count]
        # the kernel's own g dW: the Euler step of the same net, the very product the Milstein step adds its correction to; it
        # is subtracted as it is, and g = (g dW) / dW enters only the divisor (half an ulp of g moves the quotient by 2^-24 of
        # a slope of at most 1/4: inside the allowance above)
        ys = torch.empty(1, rows, d, device=DEV)
        K.trajectory_mlp_general(ys, z(rows, d), fnet, gnet, _native.NOISE_DIAGONAL, d, _native.TRAJ_EULER, schedule, bm)
        gdw[:, lo:lo + count] = ys[0].cpu().numpy().astype(np.float64)[:, :count]
        g[:, lo:lo + count] = gdw[:, lo:lo + count] / dw_all[:, :count]
    _check_recovered_slope(y1, g, dw, REF["sigmoid.slope"], "milstein_closing", "sigmoid.slope",
                           "mlp_general Milstein, closing sigmoid", d, gdw=gdw)


# ---- the table of profiles/neural_activation_accuracy.txt --------------------------------------------------------------------------
def _torch_errors():
    """torch float32's own error on the device for the same functions (slopes: its autograd), in the same measure."""
    c = float(forms.LIPSWISH_C)
    fns = {"tanh": torch.tanh, "softplus": torch.nn.functional.softplus, "sigmoid": torch.sigmoid,
           "lipswish": lambda t: c * torch.nn.functional.silu(t)}
    out = {}
    for name, fn in fns.items():
        t = _dev(X).requires_grad_(True)
        v = fn(t)
        (grad,) = torch.autograd.grad(v.sum(), t)
        out[f"{name}.value"] = forms.measure(v.detach().cpu().numpy(), REF[f"{name}.value"])
        out[f"{name}.slope"] = forms.measure(grad.cpu().numpy(), REF[f"{name}.slope"])
    return out


def accuracy_table():
    MEASURED.clear()
    for case in CASES:
        test_hidden_activation_values_and_slopes_against_float64(*case)
    test_perceptron_sigmoid_diffusion_value()
    for adjoint in (False, True):
        test_perceptron_sigmoid_diffusion_slope_q(adjoint)
    for noise in ("diagonal", "scalar"):
        test_mlp_general_closing_sigmoid(noise)
    test_mlp_general_staged_bias_sigmoid(32, 8)
    for final in ("sigmoid", "tanh"):
        test_deep_network_closing_functions_and_their_slopes(final)
        test_deep_network_general_noise_closing_slopes(final)
    for act in ("tanh", "softplus"):
        test_mlp_general_milstein_hidden_slopes(act)
    test_mlp_general_milstein_closing_sigmoid_slope()
    e_torch = _torch_errors()
    labels = [forms.binade(v) for v in X]
    order = sorted(set(labels), key=lambda b: (b != "0", b[0] == "+", (1 if b[0] == "+" else -1) * int(b[3:] or 0) if b != "0" else 0))
    lines = [f"# device: {torch.cuda.get_device_properties(0).gcnArchName}; {len(X)} float32 sample points (tests/neural_activation_forms.py)",
             "# error = |got - float64 reference| / max(1, |reference|), worst over the points of a binade",
             "# E_kernel: the kernels on the device, worst over the routes that reach the site (listed under the site);",
             "# E_form: the CPU emulation of the site's formula with correctly rounded exp2 / rcp / log2; bound = 2 E_form(whole grid) + 2^-24;",
             "# E_torch: torch float32's operator (slope: its autograd) on the device, for information only",
             "# site quantity binade points E_kernel E_form E_torch bound"]
    for site in forms.SITES:
        emulated = forms.emulate(site, X)
        for quantity in forms.quantities(site):
            runs = MEASURED.get((site, quantity), [])
            lines.append(f"## {site} {quantity}: " + ("; ".join(sorted({w for w, _, _ in runs})) or "no route of a kernel reads this out"))
            e_form = forms.measure(emulated[quantity], REF[quantity])
            e_kernel = np.zeros(len(X))
            seen = np.zeros(len(X), dtype=bool)
            index = {float(v): k for k, v in enumerate(X)}
            for _, x, err in runs:
                at = np.array([index[float(v)] for v in x])
                measured = ~np.isnan(err)
                np.maximum.at(e_kernel, at[measured], err[measured])
                seen[at[measured]] = True
            for b in order:
                sel = np.array([lab == b for lab in labels])
                kernel = f"{e_kernel[sel & seen].max():.3e}" if (sel & seen).any() else "-"
                lines.append(f"{site:20s} {quantity:15s} {b:>7s} {int(sel.sum()):3d} {kernel:>10s} {e_form[sel].max():.3e} "
                             f"{e_torch[quantity][sel].max():.3e} {forms.bound(site, quantity):.3e}")
    return "\n".join(lines) + "\n"
