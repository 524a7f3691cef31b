"""Small row-coupled systems with a diffusion MATRIX -- general, scalar and additive noise -- take ONE launch
(torchsde_amd/recognise_rows.py with `m`, specialise.source_rows_general, csrc/trajectory.hip trajectory_rows_general_kernel;
``-m gpu``): unchanged user modules (tests/helpers_rows_general.py) through `sdeint` under no_grad with Euler, midpoint, Heun
and Euler-Heun. float32 against the oracle's restatement of the reference's loop on the same Brownian path, with the
project's criterion; float64 against the stepwise route at the verifying solve's own tolerance."""
import unittest.mock as mock

import numpy as np
import pytest
import torch

from tests import helpers
from tests import helpers_rows_general as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, STEPS, DT = 300, 40, 2.0 ** -8            # (300 rows: a ragged last block)
TS = (0.0, 13.5 * DT, STEPS * DT)            # (one output interpolates inside a step)
# every module x every scheme of its SDE type (Heston is an Ito model; the others are written for either calculus)
CASES = [(name, method) for name in sorted(H.modules()) for sde_type in (("ito",) if name == "heston" else ("ito", "stratonovich"))
         for method in H.SCHEMES[sde_type]]


@pytest.fixture(autouse=True)
def _compile_in_the_calling_thread(monkeypatch, tmp_path_factory):
    from torchsde_amd import specialise
    monkeypatch.setattr(specialise, "MODE", "sync")
    monkeypatch.setenv("TSDE_SPECIALISE_CACHE", str(tmp_path_factory.getbasetemp() / "specialised"))
    before = torch.get_num_threads()
    torch.set_num_threads(min(8, before))     # (the oracle integrates a few dozen rows on the CPU)
    yield
    torch.set_num_threads(before)


def _sde_type(method):
    return "ito" if method in ("euler", "srk", "milstein") else "stratonovich"


def _make(name, method, dtype=torch.float32):
    return H.modules()[name](_sde_type(method)).to(DEV, dtype)


def _solve(sde, entropy, method, dtype=torch.float32, stepwise=False, rows=(0, B), levy="none", d=None, m=None, grad=False):
    import torchsde_amd
    d, m = d or sde.d, m or sde.m
    n = rows[1] - rows[0]
    y0 = torch.tensor(sde.y0 if d == sde.d else [0.3] * d, device=DEV, dtype=dtype).expand(n, d).contiguous()
    ts = torch.tensor(TS, device=DEV, dtype=dtype)
    bm = torchsde_amd.BrownianInterval(0.0, STEPS * DT, size=(n, m), device=DEV, dtype=dtype, entropy=entropy, dt=DT,
                                       levy_area_approximation=levy, row_offset=rows[0])
    options = {"hip_graph": False}
    if stepwise:
        options["trajectory_kernel"] = False
    if grad:
        return torchsde_amd.sdeint(sde, y0.requires_grad_(), ts, bm=bm, method=method, dt=DT, options=options)
    with torch.no_grad():
        return torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=DT, options=options)


def _book(sde):
    from torchsde_amd import solvers
    return getattr(sde, solvers.BaseSDESolver._RECOGNISED_ATTR, {"trusted": {}, "refused": {}})


def _launches(fn):
    from torchsde_amd import kernels as K
    K.prof_begin(8, 64)
    out = fn()
    torch.cuda.synchronize()
    return out, K.prof_end()[1]


_oracle_cache = {}


def _oracle(name, method, entropy, scale=None):
    """The sampled rows and the oracle's float32 and float64 runs (same parameter values, widened) of those rows on the
    counter-RNG Brownian path; computed once per case."""
    from oracle import solvers_ref
    key = (name, method, entropy, scale)
    if key not in _oracle_cache:
        rows = helpers.sampled_rows(B, 32, seams=(256,))
        out = []
        for dtype in (torch.float32, torch.float64):
            sde = H.modules()[name](_sde_type(method))
            if scale is not None:
                _change(sde, scale)
            sde = sde.to(dtype)
            bm = helpers.counter_rows_bm(rows, sde.m, entropy, np.arange(STEPS + 1) * DT, dtype)
            y0 = torch.tensor(sde.y0, dtype=dtype).expand(len(rows), sde.d).contiguous()
            with torch.no_grad():
                out.append(solvers_ref.integrate(sde, bm, y0, torch.tensor(TS, dtype=dtype), DT, method))
        _oracle_cache[key] = (rows, out[0], out[1])
    return _oracle_cache[key]


def _change(sde, scale):
    with torch.no_grad():                       # an optimiser step on Heston's correlation and vol-of-vol
        sde.rho.mul_(scale)
        sde.xi.mul_(2.0 - scale)


def _assert_float32_criterion(ys, name, method, entropy, scale=None):
    rows, ref32, ref64 = _oracle(name, method, entropy, scale)
    got = ys[:, torch.from_numpy(rows).to(DEV)]
    for k in range(len(TS)):
        helpers.assert_within_reference_rounding(got[k], ref32[k], ref64[k], f"{name}, {method}, output {k}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,method", CASES)
def test_one_launch_of_the_generated_row_kernel(name, method, dtype):
    sde = _make(name, method, dtype)
    first = _solve(sde, 1, method, dtype)
    assert torch.equal(first, _solve(sde, 1, method, dtype, stepwise=True))          # the verifying solve
    assert list(_book(sde)["trusted"].values()) == [True], _book(sde)
    fast, launches = _launches(lambda: _solve(sde, 2, method, dtype))
    assert launches == 1
    if dtype == torch.float32:
        _assert_float32_criterion(fast, name, method, 2)
    else:
        torch.testing.assert_close(fast, _solve(sde, 2, method, dtype, stepwise=True), rtol=1e-9, atol=1e-11)


def test_live_parameters():
    sde = _make("heston", "euler")
    _solve(sde, 1, "euler")
    before, launches = _launches(lambda: _solve(sde, 2, "euler"))
    assert launches == 1
    _change(sde, 0.5)
    after, launches = _launches(lambda: _solve(sde, 2, "euler"))
    assert launches == 1 and not torch.equal(after, before)
    _assert_float32_criterion(after, "heston", "euler", 2, scale=0.5)


@pytest.mark.parametrize("name", ["heston", "dense_2x4", "dense_3x5"])     # m = 2, 4 (one Philox quad per row), 5
def test_a_shard_draws_its_rows_of_the_field(name):
    method = "euler" if name == "heston" else "heun"
    sde = _make(name, method)
    _solve(sde, 1, method)
    full, launches = _launches(lambda: _solve(sde, 2, method))
    assert launches == 1
    _solve(sde, 1, method, rows=(150, 300))                    # (another batch size: its own verifying solve)
    assert list(_book(sde)["trusted"].values()) == [True, True], _book(sde)
    shard, launches = _launches(lambda: _solve(sde, 2, method, rows=(150, 300)))
    assert launches == 1 and torch.equal(shard, full[:, 150:300])


def _stays_stepwise(sde, method, levy="none", **kwargs):
    for entropy in (1, 2):
        out, launches = _launches(lambda: _solve(sde, entropy, method, levy=levy, **kwargs))
        assert launches == 0
    assert torch.equal(out, _solve(sde, 2, method, levy=levy, stepwise=True, **kwargs))


def test_what_stays_stepwise():
    from torchsde_amd import specialise
    # SRK and Milstein: the defaults of Ito scalar and additive noise, a later step
    _stays_stepwise(_make("scalar_vdp", "srk"), "srk", levy="space-time")
    _stays_stepwise(_make("langevin", "srk"), "srk", levy="space-time")
    _stays_stepwise(_make("scalar_vdp", "milstein"), "milstein")
    # more than 8 channels, more than 8 Brownian channels
    _stays_stepwise(H.Dense(9, 2, "ito").to(DEV), "euler")
    _stays_stepwise(H.Dense(2, 9, "ito").to(DEV), "euler")
    # no compiler: there is no interpreter for these systems, so nothing changes
    with mock.patch.object(specialise, "compiler", lambda: None):
        _stays_stepwise(_make("heston", "euler"), "euler")


def test_autograd_stays_stepwise():
    sde = _make("heston", "euler")
    for entropy in (1, 2):
        ys, launches = _launches(lambda: _solve(sde, entropy, "euler", grad=True))
        assert launches == 0 and ys.requires_grad
    assert torch.equal(ys.detach(), _solve(sde, 2, "euler", stepwise=True))
    assert not _book(sde)["trusted"]


def test_the_route_is_described():
    import torchsde_amd
    sde = _make("heston", "euler")
    _solve(sde, 1, "euler")
    lines = torchsde_amd.recognise.describe(sde)
    assert any("row-coupled system of 2 channels, 2 Brownian channels: trajectory kernel" in line for line in lines), lines
