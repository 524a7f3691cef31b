"""Milstein (milstein.py:52-74) on the neural-SDE kernel `tsde_trajectory_mlp_general` for diagonal and scalar noise (``-m gpu``):
the derivative form -- the vector-Jacobian product of base_sde.py:127-155 as the diffusion net walked backwards on the matrix
cores -- and the derivative-free form (`options={"grad_free": True}`, milstein.py:58-67: a second pass of the diffusion net).

Pinned like tests/test_gpu_neural.py: against the stepwise route, through the C ABI against a float64 torch statement of the
scheme with autograd supplying the product, and against the oracle's restatement of the reference's loop on sampled rows."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import helpers
from workloads import problems

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = 2.0 ** -7

# (hidden above 64: the 128-unit instantiations; d = 3, 10, 37: rows that are not 16-byte groups; d = 37, 40: four state tiles
#  but three staged tiles of the diffusion net's output layer -- the padded channels are a contraction index of the way back)
SHAPES = ((8, 8), (20, 24), (64, 64), (16, 128), (64, 100), (3, 8), (10, 16), (37, 24), (40, 64))
PROBLEMS = ("netdiag_ito", "netdiag_strat", "netscalar_ito", "netscalar_strat")


def _bm(B, m, t1, entropy, row_offset=0):
    import torchsde_amd
    return torchsde_amd.BrownianInterval(0.0, t1, size=(B, m), dtype=torch.float32, device=DEV, entropy=entropy, dt=DT,
                                         row_offset=row_offset)


def _m(name, d):
    return 1 if name.startswith("netscalar") else d


OPT_IN = {"neural_milstein_kernel": True}      # (the route is off by default: its timings are not on file)


def _solve(sde, m, entropy, grad_free, B=96, d=None, steps=24, stepwise=False, y0=None, grad=False, extra=OPT_IN):
    import torchsde_amd
    y0 = torch.full((B, d), 0.1, device=DEV) if y0 is None else y0
    ts = torch.tensor([0.0, 7.5 * DT, steps * DT], device=DEV)
    options = dict(extra or {}, hip_graph=False, grad_free=grad_free)
    if stepwise:
        options["trajectory_kernel"] = False
    with torch.enable_grad() if grad else torch.no_grad():
        return torchsde_amd.sdeint(sde, y0, ts, bm=_bm(B, m, float(ts[-1]), entropy), method="milstein", dt=DT, options=options)


def _book(sde):
    from torchsde_amd import solvers
    return getattr(sde, solvers.BaseSDESolver._RECOGNISED_ATTR, {"trusted": {}, "refused": {}})


def _launches(fn):
    from torchsde_amd import kernels as K
    K.prof_begin(8, 64)
    out = fn()
    torch.cuda.synchronize()
    return out, K.prof_end()[1]


@pytest.mark.parametrize("grad_free", [False, True], ids=["derivative", "grad_free"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_milstein_is_one_launch_and_agrees_with_the_stepwise_route(name, grad_free):
    """NeuralDiagonal / NeuralScalar-style modules (softplus nets of cat([t, y]), g = 0.1 * sigmoid-closed net) under
    `method="milstein"`: the first solve verifies and returns the stepwise result, later ones are ONE launch; an output time
    inside a step."""
    from torchsde_amd import recognise
    for d, hidden in SHAPES:
        sde = problems.make(name, d=d, hidden=hidden).to(DEV)
        m = _m(name, d)
        first = _solve(sde, m, 1, grad_free, d=d)
        assert torch.equal(first, _solve(sde, m, 1, grad_free, d=d, stepwise=True))
        assert list(_book(sde)["trusted"].values()) == [True], _book(sde)
        for entropy in (2, 3):
            fast, launches = _launches(lambda: _solve(sde, m, entropy, grad_free, d=d))
            assert launches == 1, (d, hidden, _book(sde))
            slow = _solve(sde, m, entropy, grad_free, d=d, stepwise=True)
            torch.testing.assert_close(fast, slow, rtol=2e-5, atol=2e-6, msg=lambda s: f"d = {d}, hidden = {hidden}: {s}")
            assert not torch.equal(fast[-1], fast[0])
        assert any("trajectory kernel (tsde_trajectory_mlp_general)" in line for line in recognise.describe(sde))


@pytest.mark.parametrize("grad_free", [False, True], ids=["derivative", "grad_free"])
@pytest.mark.parametrize("name", ["netdiag_ito", "netscalar_strat"])
def test_a_partial_last_group_and_increments_by_global_row(name, grad_free):
    d, hidden = 20, 24
    sde = problems.make(name, d=d, hidden=hidden).to(DEV)
    m = _m(name, d)
    whole = [_solve(sde, m, 5, grad_free, B=200, d=d) for _ in range(2)][1]          # (the second solve: the kernel)
    (odd, launches) = [_launches(lambda: _solve(sde, m, 5, grad_free, B=77, d=d)) for _ in range(2)][1]
    assert launches == 1
    assert torch.equal(odd, whole[:, :77])


def test_the_two_forms_differ_and_each_earns_its_own_trust():
    d, hidden = 20, 24
    sde = problems.make("netdiag_ito", d=d, hidden=hidden).to(DEV)
    _solve(sde, d, 1, False, d=d)
    assert list(_book(sde)["trusted"].values()) == [True]
    derivative, launches = _launches(lambda: _solve(sde, d, 2, False, d=d))
    assert launches == 1
    # the derivative-free form on the same, already trusted module: its first solve runs both routes again
    first, launches = _launches(lambda: _solve(sde, d, 2, True, d=d))
    assert launches == 1 and torch.equal(first, _solve(sde, d, 2, True, d=d, stepwise=True))      # (the verifying launch)
    book = _book(sde)["trusted"]
    assert len(book) == 2 and all(v is True for v in book.values()), book
    assert sorted("grad_free" in key[7:] for key in book) == [False, True]
    free, launches = _launches(lambda: _solve(sde, d, 2, True, d=d))
    assert launches == 1
    assert not torch.equal(free, derivative)
    torch.testing.assert_close(derivative, _solve(sde, d, 2, False, d=d, stepwise=True), rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(free, first, rtol=2e-5, atol=2e-6)


# ---- the C ABI directly ------------------------------------------------------------------------------------------------------
def _abi_problem(noise, steps, B, d, hf, hg, act, final, timed):
    from torchsde_amd import _native, kernels as K
    mk = lambda *shape: (0.4 * torch.randn(*shape, device=DEV)).contiguous()      # noqa: E731
    fnet = K.NeuralNet(mk(d, hf), mk(hf) if timed else None, mk(hf), mk(hf, d), mk(d), act)
    gnet = K.NeuralNet(mk(d, hg), mk(hg) if timed else None, mk(hg), mk(hg, d), mk(d), act, final, 0.3)
    m = d if noise == _native.NOISE_DIAGONAL else 1
    bm = _bm(B, m, steps * DT, 11)
    grid = np.arange(steps + 1) * DT
    bm.adopt_grid(grid)
    cells = np.asarray(bm.match_grid(grid), dtype=np.int64)
    rows = np.zeros((steps, 8))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = DT, DT / 2, 1 / DT, np.sqrt(DT)
    rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7] = np.sqrt(DT), np.sqrt(DT / 12), DT, grid[:-1]
    schedule = K.TrajectorySchedule(rows, cells, [steps], [(0.0, 1.0)], torch.device(DEV), torch.float32)
    return fnet, gnet, m, bm, grid, schedule


def _float64_milstein(fnet, gnet, bm, grid, y0, act, final, ito, grad_free):
    """milstein.py:52-74 in float64 on the increments of `bm`; autograd supplies (dg/dy)^T (g v/2) (base_sde.py:127-155)."""
    from torchsde_amd import _native
    W = lambda t: None if t is None else t.double()                                # noqa: E731
    fw1, fwt, fb1, fw2, fb2 = map(W, fnet.tensors)
    gw1, gwt, gb1, gw2, gb2 = map(W, gnet.tensors)
    phi = torch.tanh if act == _native.ACT_TANH else nn.functional.softplus

    def f_of(t, y):
        return phi(y @ fw1 + fb1 + (0.0 if fwt is None else fwt * t)) @ fw2 + fb2

    def g_of(t, y):
        z = phi(y @ gw1 + gb1 + (0.0 if gwt is None else gwt * t)) @ gw2 + gb2
        return 0.3 * (torch.sigmoid(z) if final == _native.FINAL_SIGMOID else z)

    y = y0.double()
    sqrt_dt = float(np.sqrt(DT))
    for k in range(len(grid) - 1):
        t = float(grid[k])
        dW = bm(float(grid[k]), float(grid[k + 1])).double()                      # (B, d) or (B, 1): broadcasts over the channels
        v = dW ** 2 - DT if ito else dW ** 2
        f = f_of(t, y)
        if grad_free:
            g = g_of(t, y)
            y_prime = y + (DT * f if ito else 0.0) + g * sqrt_dt
            gdg = (g_of(t, y_prime) - g) * v / (2 * sqrt_dt)
        else:
            with torch.enable_grad():
                yy = y.detach().requires_grad_(True)
                g = g_of(t, yy)
                gdg, = torch.autograd.grad(g, yy, grad_outputs=g.detach() * (0.5 * v))
            g = g.detach()
        y = y + f * DT + g * dW + gdg
    return y


@pytest.mark.parametrize("code", ["TRAJ_MILSTEIN_ITO", "TRAJ_MILSTEIN_STRAT", "TRAJ_MILSTEIN_ITO_GF", "TRAJ_MILSTEIN_STRAT_GF"])
@pytest.mark.parametrize("noise", ["NOISE_DIAGONAL", "NOISE_SCALAR"])
def test_c_abi_against_a_float64_statement_of_the_scheme(noise, code):
    """tsde_trajectory_mlp_general called directly with the four Milstein codes: tanh and softplus nets, with and without a
    closing sigmoid, with and without a time input; materialised increments of the same generator."""
    from torchsde_amd import _native, kernels as K
    torch.manual_seed(0)
    B, d, hf, hg, steps = 40, 12, 16, 24, 8
    noise, method = getattr(_native, noise), getattr(_native, code)
    ito, grad_free = "ITO" in code, code.endswith("_GF")
    for act in (_native.ACT_TANH, _native.ACT_SOFTPLUS):
        for final in (_native.FINAL_NONE, _native.FINAL_SIGMOID):
            for timed in (False, True):
                fnet, gnet, m, bm, grid, schedule = _abi_problem(noise, steps, B, d, hf, hg, act, final, timed)
                y0 = torch.full((B, d), 0.1, device=DEV)
                ys = torch.empty(1, B, d, device=DEV)
                K.trajectory_mlp_general(ys, y0, fnet, gnet, noise, m, method, schedule, bm)
                want = _float64_milstein(fnet, gnet, bm, grid, y0, act, final, ito, grad_free)
                torch.testing.assert_close(ys[0].double(), want, rtol=2e-5, atol=2e-6,
                                           msg=lambda s: f"act {act}, final {final}, time input {timed}: {s}")


@pytest.mark.parametrize("code", ["TRAJ_MILSTEIN_ITO", "TRAJ_MILSTEIN_STRAT", "TRAJ_MILSTEIN_ITO_GF", "TRAJ_MILSTEIN_STRAT_GF"])
def test_c_abi_refuses_milstein_on_general_noise(code):
    from torchsde_amd import _native, kernels as K
    torch.manual_seed(0)
    B, d, m, h, steps = 40, 12, 4, 16, 8
    mk = lambda *shape: (0.4 * torch.randn(*shape, device=DEV)).contiguous()      # noqa: E731
    fnet = K.NeuralNet(mk(d, h), None, mk(h), mk(h, d), mk(d), _native.ACT_TANH)
    gnet = K.NeuralNet(mk(d, h), None, mk(h), mk(h, d * m), mk(d * m), _native.ACT_TANH, _native.FINAL_NONE, 0.3)
    _, _, _, _, grid, schedule = _abi_problem(_native.NOISE_SCALAR, steps, B, d, h, h, _native.ACT_TANH, _native.FINAL_NONE, False)
    bm = _bm(B, m, steps * DT, 11)
    bm.adopt_grid(grid)
    ys = torch.full((1, B, d), -7.0, device=DEV)
    with pytest.raises(_native.NativeLibraryError, match="Milstein takes diagonal or scalar noise"):
        K.trajectory_mlp_general(ys, torch.full((B, d), 0.1, device=DEV), fnet, gnet, _native.NOISE_GENERAL, m,
                                 getattr(_native, code), schedule, bm)
    torch.cuda.synchronize()
    assert bool((ys == -7.0).all())
    # (the same call under Euler is a launch: what is refused is the scheme, not the shape)
    K.trajectory_mlp_general(ys, torch.full((B, d), 0.1, device=DEV), fnet, gnet, _native.NOISE_GENERAL, m, _native.TRAJ_EULER,
                             schedule, bm)
    assert bool(torch.isfinite(ys).all()) and not bool((ys == -7.0).any())


# ---- rows against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_free", [False, True], ids=["derivative", "grad_free"])
@pytest.mark.parametrize("name,d", [("netdiag_ito", 32), ("netscalar_ito", 16)])
def test_rows_vs_oracle(name, d, grad_free):
    """4096 rows, 256 steps: sampled rows against the ORACLE's restatement of the reference's loop (milstein.py:52-94) on the same
    Brownian path in float32 and float64, the bound of tests/test_gpu_full_size_oracle.py."""
    import torchsde_amd
    from oracle import solvers_ref
    Bf, n, dt = 4096, 256, 2.0 ** -8
    m = _m(name, d)
    sde = problems.make(name, d=d, hidden=16).to(DEV)
    y0 = torch.full((Bf, d), 0.1, device=DEV)
    ts = torch.tensor([0.0, n * dt], device=DEV)
    options = dict(OPT_IN, grad_free=grad_free)

    def bm(entropy):
        return torchsde_amd.BrownianInterval(0.0, n * dt, size=(Bf, m), dtype=torch.float32, device=DEV, entropy=entropy, dt=dt)
    before = torch.get_num_threads()
    torch.set_num_threads(min(8, before))
    try:
        with torch.no_grad():
            torchsde_amd.sdeint(sde, y0, ts, bm=bm(5), method="milstein", dt=dt, options=dict(options))
            ys, launches = _launches(lambda: torchsde_amd.sdeint(sde, y0, ts, bm=bm(20240601), method="milstein", dt=dt,
                                                                 options=dict(options)))
        assert launches == 1 and list(_book(sde)["trusted"].values()) == [True], _book(sde)
        rows = helpers.sampled_rows(Bf, 48, seed=11, seams=(16, Bf - 16))
        edges = np.arange(n + 1) * dt
        ref = {}
        for dtype in (torch.float32, torch.float64):
            twin = copy.deepcopy(sde).cpu().to(dtype)                  # (the same parameter values, widened)
            path = helpers.counter_rows_bm(rows, m, 20240601, edges, dtype)
            with torch.no_grad():
                ref[dtype] = solvers_ref.integrate(twin, path, torch.full((len(rows), d), 0.1, dtype=dtype),
                                                   torch.tensor([0.0, n * dt], dtype=dtype), dt, "milstein",
                                                   options={"grad_free": grad_free})
        helpers.assert_within_reference_rounding(ys[-1][torch.from_numpy(rows).to(DEV)], ref[torch.float32][-1],
                                                 ref[torch.float64][-1], f"{name}, milstein {options}, neural-SDE kernel")
    finally:
        torch.set_num_threads(before)


# ---- what stays stepwise --------------------------------------------------------------------------------------------------------
def test_what_stays_stepwise():
    """General noise (the opt-in extension), diffusion nets deeper than two layers, and solves that autograd records."""
    # general noise with `options={"general_noise": True}`
    gen = problems.MLPGeneral(8, 4, "ito", hidden=8).to(DEV)
    for grad_free in (False, True):
        for _ in range(2):
            got, launches = _launches(lambda: _solve(gen, 4, 3, grad_free, d=8, extra=dict(OPT_IN, general_noise=True)))
            assert launches == 0
        assert torch.equal(got, _solve(gen, 4, 3, grad_free, d=8, stepwise=True, extra=dict(OPT_IN, general_noise=True)))
    # a three-layer diffusion net
    deep = problems.make("netdiag_ito", d=8, hidden=8).to(DEV)
    deep.g_net = problems._mlp(torch.Generator().manual_seed(9), (9, 8, 8, 8), torch.float32, final=nn.Sigmoid()).to(DEV)
    for grad_free in (False, True):
        for _ in range(2):
            got, launches = _launches(lambda: _solve(deep, 8, 3, grad_free, d=8))
            assert launches == 0
        assert torch.equal(got, _solve(deep, 8, 3, grad_free, d=8, stepwise=True))
    # the two-layer module with autograd recording: a start that requires a gradient
    sde = problems.make("netdiag_ito", d=8, hidden=8).to(DEV)
    _solve(sde, 8, 1, False, d=8)
    _, launches = _launches(lambda: _solve(sde, 8, 3, False, d=8))
    assert launches == 1
    # ... and the same module without the option: the route is off by default
    for grad_free in (False, True):
        got, launches = _launches(lambda: _solve(sde, 8, 3, grad_free, d=8, extra=None))
        assert launches == 0
        assert torch.equal(got, _solve(sde, 8, 3, grad_free, d=8, stepwise=True))
    for grad_free in (False, True):
        y0 = torch.full((96, 8), 0.1, device=DEV).requires_grad_()
        for _ in range(2):
            got, launches = _launches(lambda: _solve(sde, 8, 3, grad_free, d=8, y0=y0, grad=True))
            assert launches == 0 and got.requires_grad
        assert torch.equal(got.detach(), _solve(sde, 8, 3, grad_free, d=8, y0=y0, grad=True, stepwise=True).detach())
