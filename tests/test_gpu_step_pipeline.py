"""GPU parity of the affine trajectory kernel's step loop (``tsde_trajectory_affine_diag``, the values-only forms with
constant coefficients; run with ``-m gpu``) at the step counts where a loop that reads its step data or draws its noise
ahead of the step would go wrong: bit-identical to the stepwise route with one step (the first step is also the last),
two, three, and seventeen -- for every scheme, both forms (with and without shifts), both widths (one 16-byte group per
lane, one element per lane) and both precisions; outputs at the end of the first step, inside a step, and at the end of the
last step. (Written with the step-ahead loop of profiles/pipeline_step_ahead_experiment.txt; the plain loop must pass it
as well, and so must any later attempt at that loop.)

The step grid is the one a fixed-step solve has: `dt` as accumulated in ``ts.dtype`` -- so neighbouring steps differ in
their low bits -- and a much shorter last step; every step has its own cell. A step that took its neighbour's row or cell
does not reproduce the stepwise route's bits."""
import numpy as np
import pytest
import torch

from tests.test_gpu_trajectory import METHODS

pytestmark = pytest.mark.gpu
DEV = "cuda"
T0, STEP = 0.072, 0.3445      # t0 + k * STEP is inexact in float32 and in float64: the rounded steps are not all equal


def _grid(n_steps, dtype):
    """Output times for a solve of `n_steps` steps (the last one 0.7 of a step): the start; the end of the first step (a
    step boundary: no interpolation); a time inside a step (the last step for n_steps <= 2); the end of the last step."""
    from torchsde_amd import timegrid
    np_dtype = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    t0 = np_dtype(T0)
    t_end = np_dtype(T0 + (n_steps - 0.3) * STEP)
    grid = timegrid.build(np.array([t0, t_end], dtype=np_dtype), STEP)
    assert grid.n_steps == n_steps
    if n_steps >= 2:       # the first two steps differ, and so do the last two: a row taken one step off is another row
        assert grid.dt[0] != grid.dt[1] and grid.dt[-2] != grid.dt[-1]
    inside = n_steps // 2
    times = [t0] + ([grid.t[1]] if n_steps > 1 else []) + [grid.t[inside] + np_dtype(0.4) * grid.dt[inside], t_end]
    ts = np.array(times, dtype=np_dtype)
    assert (np.diff(ts) > 0).all()
    full = timegrid.build(ts, STEP)
    assert full.n_steps == n_steps and np.array_equal(full.t, grid.t)
    weights = [(w0, w1) for (_, _, w0, w1) in full.outputs]
    if n_steps > 1:
        assert weights[0] == (0.0, 1.0) and full.outputs[0][1] == 1          # at the end of the first step
    assert 0.0 < weights[-2][1] < 1.0 and full.outputs[-2][1] == inside + 1   # inside a step
    assert weights[-1] == (0.0, 1.0) and full.outputs[-1][1] == n_steps       # at the end of the last step
    return torch.from_numpy(ts).to(DEV)


def _sde(d, dtype, sde_type, linear):
    import torchsde_amd
    gen = torch.Generator().manual_seed(7)
    rate_f, shift_f, rate_g, shift_g = (torch.rand(d, generator=gen, dtype=torch.float64) * s + o
                                        for s, o in ((0.6, -0.3), (0.4, -0.2), (0.5, 0.1), (0.2, -0.1)))
    if linear:
        return torchsde_amd.AffineDiagonalSDE(rate_f.to(dtype), torch.zeros(d, dtype=dtype), rate_g.to(dtype), 0.0,
                                              sde_type=sde_type, dtype=dtype, device=DEV)
    return torchsde_amd.AffineDiagonalSDE(rate_f, shift_f, rate_g, shift_g, sde_type=sde_type, dtype=dtype, device=DEV)


def _solve(sde, y0, ts, method, trajectory, launches=None):
    import torchsde_amd
    from torchsde_amd import kernels as K
    levy = "space-time" if method == "srk" else "none"
    bm = torchsde_amd.BrownianInterval(float(ts[0]), float(ts[-1]), size=tuple(y0.shape), dtype=y0.dtype, device=DEV,
                                       entropy=23, levy_area_approximation=levy)
    true_launch = K.trajectory_affine_diag

    def recording(*args, **kwargs):
        launches.append(bool(kwargs.get("linear", False)))
        return true_launch(*args, **kwargs)

    if launches is not None:
        K.trajectory_affine_diag = recording
    try:
        with torch.no_grad():
            return torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=STEP, options={"trajectory_kernel": trajectory})
    finally:
        K.trajectory_affine_diag = true_launch


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(8192, 64), (33, 5)])       # one 16-byte group per lane; one element per lane
@pytest.mark.parametrize("linear", [True, False])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 17])
@pytest.mark.parametrize("method,sde_type", METHODS)
def test_step_loop_is_bit_identical_to_stepwise_path_at_small_step_counts(method, sde_type, n_steps, linear, shape, dtype):
    B, d = shape
    sde = _sde(d, dtype, sde_type, linear)
    y0 = torch.linspace(0.5, 1.5, B * d, dtype=dtype, device=DEV).reshape(B, d)
    ts = _grid(n_steps, dtype)
    launches = []
    a = _solve(sde, y0, ts, method, True, launches)
    b = _solve(sde, y0, ts, method, False)
    assert launches == [linear]                          # one launch of the trajectory kernel, of the form meant
    assert a.shape == (ts.numel(), B, d) and torch.isfinite(a).all()
    assert torch.equal(a, b)

