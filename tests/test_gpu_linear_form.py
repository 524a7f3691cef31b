"""GPU parity of the LINEAR form of the affine trajectory kernel (``tsde_trajectory_affine_diag`` with null shifts:
f = rate * y, g = rate * y; run with ``-m gpu``): bit-identical to the stepwise route -- for `AffineDiagonalSDE` with zero
shifts and for a plain user module `mu * y`, `sigma * y` -- and equal to the general form fed explicit zero arrays."""
import pytest
import torch
from torch import nn

from tests.test_gpu_trajectory import METHODS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rates(d, dtype):
    gen = torch.Generator().manual_seed(7)
    mu = (torch.rand(d, generator=gen, dtype=torch.float64) * 0.6 - 0.3).to(dtype)
    sigma = (torch.rand(d, generator=gen, dtype=torch.float64) * 0.5 + 0.1).to(dtype)
    return mu, sigma


class _UserGBM(nn.Module):
    """A plain module, nothing of this package: drift mu * y, diffusion sigma * y."""
    noise_type = "diagonal"

    def __init__(self, mu, sigma, sde_type):
        super().__init__()
        self.mu, self.sigma, self.sde_type = nn.Parameter(mu), nn.Parameter(sigma), sde_type

    def f(self, t, y):
        return self.mu * y

    def g(self, t, y):
        return self.sigma * y


def _solve(sde, y0, ts, method, trajectory, launches=None):
    import torchsde_amd
    from torchsde_amd import kernels as K
    levy = "space-time" if method == "srk" else "none"
    bm = torchsde_amd.BrownianInterval(float(ts[0]), float(ts[-1]), size=tuple(y0.shape), dtype=y0.dtype, device=DEV,
                                       entropy=11, levy_area_approximation=levy)
    true_launch = K.trajectory_affine_diag

    def recording(*args, **kwargs):
        launches.append(bool(kwargs.get("linear", False)))
        return true_launch(*args, **kwargs)

    if launches is not None:
        K.trajectory_affine_diag = recording
    try:
        with torch.no_grad():
            return torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=0.05, options={"trajectory_kernel": trajectory})
    finally:
        K.trajectory_affine_diag = true_launch


def _problem(shape, dtype):
    B, d = shape
    y0 = torch.linspace(0.5, 1.5, B * d, dtype=dtype, device=DEV).reshape(B, d)
    # output times on and off the step grid (off-grid ones are interpolated inside a step), ragged last step
    ts = torch.tensor([0.0, 0.1, 0.25, 0.26, 0.7, 1.03], dtype=dtype, device=DEV)
    return y0, ts


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(8192, 64), (33, 5), (16, 8)])
@pytest.mark.parametrize("method,sde_type", METHODS)
def test_linear_form_is_bit_identical_to_stepwise_path_closed_form(method, sde_type, shape, dtype):
    import torchsde_amd
    mu, sigma = _rates(shape[1], dtype)
    sde = torchsde_amd.AffineDiagonalSDE(mu, torch.zeros(shape[1], dtype=dtype), sigma, 0.0, sde_type=sde_type, dtype=dtype,
                                         device=DEV)
    y0, ts = _problem(shape, dtype)
    launches = []
    a = _solve(sde, y0, ts, method, True, launches)
    b = _solve(sde, y0, ts, method, False)
    assert launches == [True]                            # one launch, of the linear form
    assert a.shape == (6,) + shape and torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(8192, 64), (33, 5), (16, 8)])
@pytest.mark.parametrize("method,sde_type", METHODS)
def test_linear_form_is_bit_identical_to_stepwise_path_user_module(method, sde_type, shape, dtype):
    mu, sigma = _rates(shape[1], dtype)
    sde = _UserGBM(mu, sigma, sde_type).to(DEV)
    y0, ts = _problem(shape, dtype)
    stepwise = _solve(sde, y0, ts, method, False)
    first = _solve(sde, y0, ts, method, True)            # the verifying solve of the recognised route: both routes
    launches = []
    a = _solve(sde, y0, ts, method, True, launches)      # trusted: one launch
    assert launches == [True]
    assert torch.equal(first, stepwise) and torch.equal(a, stepwise)


def test_a_non_zero_shift_keeps_the_general_form_and_an_update_is_seen():
    import torchsde_amd
    d, dtype = 8, torch.float32
    mu, sigma = _rates(d, dtype)
    sde = torchsde_amd.AffineDiagonalSDE(mu, torch.zeros(d), sigma, 0.0, dtype=dtype, device=DEV)
    y0, ts = _problem((16, d), dtype)
    launches = []
    _solve(sde, y0, ts, "euler", True, launches)
    with torch.no_grad():
        sde.drift_shift[3] = 0.25
    a = _solve(sde, y0, ts, "euler", True, launches)
    assert launches == [True, False]
    assert torch.equal(a, _solve(sde, y0, ts, "euler", False))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("rows", [8192, 33])
def test_c_abi_null_shifts_equal_explicit_zero_arrays(rows, dtype):
    """The entry itself: null shift pointers (linear form) against the same call with zero arrays (general form), every
    scheme; and one null pointer alone is rejected."""
    from torchsde_amd import _native
    from torchsde_amd import kernels as K
    lib = _native.load()
    d, n_steps = 64, 20
    mu, sigma = (c.to(DEV) for c in _rates(d, dtype))
    zero = torch.zeros(d, dtype=dtype, device=DEV)
    y0 = torch.linspace(0.5, 1.5, rows * d, dtype=dtype, device=DEV).reshape(rows, d)
    dt, h = 0.05, 0.05
    step_rows = [[dt, dt / 2, 1 / dt, dt ** 0.5, h ** 0.5, (h / 12) ** 0.5, h, k * dt] for k in range(n_steps)]
    schedule = K.TrajectorySchedule(step_rows, list(range(n_steps)), [7, 8, n_steps], [(0.0, 1.0), (0.4, 0.6), (0.0, 1.0)],
                                    y0.device, dtype)
    dt_code = _native.F32 if dtype == torch.float32 else _native.dtype_code(dtype)

    stream = torch.cuda.current_stream(y0.device).cuda_stream

    def call(method, b, e):
        ys = torch.full((3, rows, d), float("nan"), dtype=dtype, device=DEV)
        code = lib.tsde_trajectory_affine_diag(ys.data_ptr(), y0.data_ptr(), rows, d, mu.data_ptr(), b, sigma.data_ptr(), e,
                                               method, schedule.struct(), 2024, 0, None, dt_code, stream)
        torch.cuda.synchronize()
        return code, ys

    for method in range(7):
        code_l, linear = call(method, None, None)
        code_g, general = call(method, zero.data_ptr(), zero.data_ptr())
        assert code_l == 0 and code_g == 0
        assert torch.isfinite(linear).all() and torch.equal(linear, general), method
    for b, e in ((None, zero.data_ptr()), (zero.data_ptr(), None)):
        code, _ = call(0, b, e)
        assert code != 0 and b"shift" in lib.tsde_last_error()
