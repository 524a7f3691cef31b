"""GPU parity of the affine trajectory kernel's rotated step loop (csrc/trajectory.hip `step_ahead_form`; run with ``-m gpu``):
the forms that load the row and the cell of step k + 1 during step k must return the bytes of the stepwise route
(``options={"trajectory_kernel": False}``), as the forms that keep the plain loop do. What a rotation by one step can get
wrong is which row a step uses (step counts 1, 2, 3, 17: the clamp, the last step, the first carried value; a grid whose
neighbouring steps differ) and what happens around an output step (interpolation inside a step, two outputs in one step,
an output at the last step, at every step, one output only).

Shapes: 69 x 4 takes one element per lane (W = 1); 131077 x 4 is `kTrajVecMinGroups` + 5 groups, the 16-byte-group form
(W = 4) with a ragged last wave; 300 x 64 is a d = 64 problem of a few hundred rows. The rotated loops are W = 4 float32 ones
with constant coefficients, so the forms are swept at the 131077 x 4 shape. A fixed-step grid does not clip its steps at the
output times, so "steps that differ" come from a step size that is no float32 number (dt = 0.1: neighbouring rows differ in
their last bits) and a short last step; a build that used row k + 1 for step k failed every case of
`test_steps_that_differ` and no other. Entropy read from device memory (`key_dev`) is handed over the way a graph
replay hands it over; replay itself is the business of tests/test_gpu_graph_auto.py."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda"

TRAJ_VEC_MIN_GROUPS = 256 * 8 * 64         # csrc/trajectory.hip kTrajVecMinGroups
ONE_PER_LANE, VECTOR, WIDE = (69, 4), (TRAJ_VEC_MIN_GROUPS + 5, 4), (300, 64)
METHODS = [("euler", "ito"), ("milstein", "ito"), ("milstein", "stratonovich"), ("midpoint", "stratonovich"), ("srk", "ito"),
           ("heun", "stratonovich"), ("euler_heun", "stratonovich")]
METHOD_IDS = [f"{m}-{t}" for m, t in METHODS]
DT = 0.125


def _sde(d, dtype, sde_type, shifts):
    import torchsde_amd
    gen = torch.Generator().manual_seed(7)
    rate, shift, vol, vol_shift = (torch.rand(d, generator=gen, dtype=torch.float64) * s + o
                                   for s, o in ((0.6, -0.3), (0.4, -0.2), (0.5, 0.1), (0.2, -0.1)))
    if not shifts:
        shift, vol_shift = torch.zeros(d, dtype=torch.float64), 0.0
    return torchsde_amd.AffineDiagonalSDE(rate, shift, vol, vol_shift, sde_type=sde_type, dtype=dtype, device=DEV)


def _y0(shape, dtype):
    return torch.linspace(-1.5, 1.5, shape[0] * shape[1], dtype=dtype, device=DEV).reshape(shape)


def _bm(y0, ts, method, entropy=23):
    import torchsde_amd
    return torchsde_amd.BrownianInterval(float(ts[0]), float(ts[-1]), size=tuple(y0.shape), dtype=y0.dtype, device=DEV,
                                         entropy=entropy, levy_area_approximation="space-time" if method == "srk" else "none")


def _solve(sde, y0, times, method, dt, trajectory):
    import torchsde_amd
    ts = torch.tensor(times, dtype=y0.dtype, device=DEV)
    with torch.no_grad():
        return torchsde_amd.sdeint(sde, y0, ts, bm=_bm(y0, ts, method), method=method, dt=dt,
                                   options={"trajectory_kernel": trajectory})


def _both_routes_agree(sde, y0, times, method, dt, where=""):
    kernel = _solve(sde, y0, times, method, dt, True)
    stepwise = _solve(sde, y0, times, method, dt, False)
    assert kernel.shape == (len(times),) + tuple(y0.shape) and torch.isfinite(kernel).all(), where
    assert torch.equal(kernel, stepwise), where
    return kernel


@pytest.mark.parametrize("shifts", [False, True], ids=["linear", "shifts"])
@pytest.mark.parametrize("method,sde_type", METHODS, ids=METHOD_IDS)
def test_step_counts(method, sde_type, shifts):
    """1 step: the row read ahead is row 0 again; 2 and 3: the first carried value is the last one; 17: a run of them."""
    for shape in (VECTOR, ONE_PER_LANE):
        sde, y0 = _sde(shape[1], torch.float32, sde_type, shifts), _y0(shape, torch.float32)
        for n_steps in (1, 2, 3, 17):
            _both_routes_agree(sde, y0, [0.0, n_steps * DT], method, DT, f"{shape} n_steps={n_steps}")


CLIPPED = [0.0, 0.3, 0.55, 1.0]        # dt = 0.125: outputs inside steps 2 and 4; a fixed-step grid does not clip at them
UNEVEN = [0.0, 0.3, 0.55, 1.03]        # dt = 0.1: the float32 grid's steps differ in their last bits, the last one is 0.03
DYADIC = [0.0, 0.25, 0.5, 1.0]         # dt = 0.125, outputs on the step grid: the schedule carries TSDE_TRAJ_POW2_STEPS


@pytest.mark.parametrize("shifts", [False, True], ids=["linear", "shifts"])
@pytest.mark.parametrize("method,sde_type", METHODS, ids=METHOD_IDS)
def test_steps_that_differ(method, sde_type, shifts, monkeypatch):
    """Every step has a Brownian cell of its own, and on the uneven grid neighbouring rows hold different dt and sqrt(h): a
    step that used the row of its neighbour would change bytes. The dyadic grid runs the folded step of Euler and midpoint,
    and with TSDE_POW2_STEPS=0 the plain one, all three the same bytes."""
    for shape in (VECTOR, ONE_PER_LANE):
        sde, y0 = _sde(shape[1], torch.float32, sde_type, shifts), _y0(shape, torch.float32)
        monkeypatch.delenv("TSDE_POW2_STEPS", raising=False)
        _both_routes_agree(sde, y0, CLIPPED, method, DT, f"{shape} clipped")
        _both_routes_agree(sde, y0, UNEVEN, method, 0.1, f"{shape} uneven")
        folded = _both_routes_agree(sde, y0, DYADIC, method, DT, f"{shape} dyadic")
        monkeypatch.setenv("TSDE_POW2_STEPS", "0")
        plain = _both_routes_agree(sde, y0, DYADIC, method, DT, f"{shape} dyadic, plain form")
        assert torch.equal(folded, plain), shape


def test_neighbouring_rows_of_the_uneven_grid_differ():
    """The grid above does what it is there for: dt changes between neighbouring steps in several places, the last included,
    and no two steps share a cell."""
    from torchsde_amd import kernels as K
    seen = []
    true_launch = K.trajectory_affine_diag

    def recording(ys, y0_, a, b, c, e, method_code, schedule, *args, **kwargs):
        seen.append(schedule)
        return true_launch(ys, y0_, a, b, c, e, method_code, schedule, *args, **kwargs)

    K.trajectory_affine_diag = recording
    try:
        _solve(_sde(4, torch.float32, "ito", False), _y0(ONE_PER_LANE, torch.float32), UNEVEN, "euler", 0.1, True)
    finally:
        K.trajectory_affine_diag = true_launch
    assert len(seen) == 1 and not seen[0].pow2_steps and seen[0].n_steps == 11
    dt, cells = seen[0].host_rows[:, 0], seen[0].host_cells
    changes = dt[1:] != dt[:-1]
    assert changes.sum() >= 4 and changes[-1] and len(set(cells.tolist())) == len(cells)


OUTPUT_GRIDS = {
    "inside a step": [0.0, 0.3125, 1.0],                      # 2.5 steps: interpolated between the state set aside and the new one
    "two inside one step": [0.0, 0.28125, 0.34375, 1.0],      # both inside step 2
    "inside the first and the last step": [0.0, 0.0625, 0.9375, 1.0],
    "at the last step": [0.0, 0.5, 1.0],
    "at every step": [k * DT for k in range(9)],
    "one output": [0.0, 1.0],
    "one output, one step": [0.0, DT],
    "consecutive steps": [0.0, 0.375, 0.5, 0.625, 1.0],       # output steps back to back, then a run of plain ones
}


@pytest.mark.parametrize("grid", sorted(OUTPUT_GRIDS))
@pytest.mark.parametrize("method,sde_type", METHODS, ids=METHOD_IDS)
def test_outputs(method, sde_type, grid):
    for shape in (VECTOR, ONE_PER_LANE):
        for shifts in (False, True):
            sde, y0 = _sde(shape[1], torch.float32, sde_type, shifts), _y0(shape, torch.float32)
            _both_routes_agree(sde, y0, OUTPUT_GRIDS[grid], method, DT, f"{shape} shifts={shifts}")


@pytest.mark.parametrize("method,sde_type", METHODS, ids=METHOD_IDS)
def test_a_wide_state_of_a_few_hundred_rows(method, sde_type):
    sde, y0 = _sde(WIDE[1], torch.float32, sde_type, True), _y0(WIDE, torch.float32)
    _both_routes_agree(sde, y0, UNEVEN, method, 0.1)
    _both_routes_agree(sde, y0, OUTPUT_GRIDS["two inside one step"], method, DT)


@pytest.mark.parametrize("shape", [VECTOR, ONE_PER_LANE], ids=["vector", "one_per_lane"])
@pytest.mark.parametrize("method,sde_type", [("euler", "ito"), ("srk", "ito")], ids=["euler", "srk"])
def test_float64(method, sde_type, shape):
    for shifts in (False, True):
        sde, y0 = _sde(shape[1], torch.float64, sde_type, shifts), _y0(shape, torch.float64)
        _both_routes_agree(sde, y0, UNEVEN, method, 0.1, f"shifts={shifts} uneven")
        for times in (OUTPUT_GRIDS["two inside one step"], [0.0, DT], [0.0, 3 * DT]):
            _both_routes_agree(sde, y0, times, method, DT, f"shifts={shifts} {times}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape", [VECTOR, ONE_PER_LANE], ids=["vector", "one_per_lane"])
@pytest.mark.parametrize("method,sde_type", [("euler", "ito"), ("srk", "ito")], ids=["euler", "srk"])
def test_the_sensitivity_route(method, sde_type, shape, dtype):
    """Parameters that require gradients: one launch carrying the path-wise sensitivities. Its values are the bytes of the
    stepwise route, and its gradients those of back-propagation through that route up to summation order."""
    import torchsde_amd
    sde = _sde(shape[1], dtype, sde_type, True)
    weight = torch.linspace(-1.0, 1.0, shape[0] * shape[1], dtype=dtype, device=DEV).reshape(shape)
    for times, dt in ((UNEVEN, 0.1), (OUTPUT_GRIDS["two inside one step"], DT), ([0.0, DT], DT)):
        ts = torch.tensor(times, dtype=dtype, device=DEV)
        out = {}
        for route in (True, False):
            y0 = _y0(shape, dtype).requires_grad_(True)
            sde.zero_grad()
            ys = torchsde_amd.sdeint(sde, y0, ts, bm=_bm(y0, ts, method), method=method, dt=dt,
                                     options={"trajectory_kernel": route})
            if route:
                assert type(ys.grad_fn).__name__ == "_TrajectoryFnBackward", ys.grad_fn
            (ys * weight).sum().backward()
            out[route] = (ys.detach(), y0.grad.clone(), [p.grad.clone() for p in sde.parameters()])
        # (the bytes to meet are those of the stepwise route without autograd: with autograd recording, the stepwise SRK solve
        #  itself returns other last bits when dt is no power of two, whichever loop the kernel runs)
        assert torch.equal(out[True][0], _solve(sde, _y0(shape, dtype), times, method, dt, False)), times
        if method != "srk":
            assert torch.equal(out[True][0], out[False][0]), times
        tol =dict(rtol=2e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=1e-9, atol=1e-11)
        torch.testing.assert_close(out[True][1], out[False][1], **tol)
        if dtype == torch.float64:       # (float32 sums over 5e5 elements depend on the order of the reduction)
            for a, b in zip(out[True][2], out[False][2]):
                torch.testing.assert_close(a, b, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("method,sde_type", [("euler", "ito"), ("heun", "stratonovich"), ("srk", "ito")],
                         ids=["euler", "heun", "srk"])
def test_entropy_read_from_device_memory(method, sde_type):
    """The word a graph replay hands over in place of the seed (`key_dev`): the key of every step's Philox head, the first
    step's, which is made before the loop, included."""
    sde, y0 = _sde(VECTOR[1], torch.float32, sde_type, False), _y0(VECTOR, torch.float32)
    ts = torch.tensor(UNEVEN, device=DEV)
    want = _solve(sde, y0, UNEVEN, method, 0.1, False)                  # stepwise, entropy 23
    import torchsde_amd
    bm = _bm(y0, ts, method, entropy=99)
    key = _bm(y0, ts, method)._key
    bm._entropy_dev = torch.tensor([key - (1 << 64) if key >= (1 << 63) else key], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        got = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=0.1, options={"trajectory_kernel": True})
    assert torch.equal(got, want)
    bm._entropy_dev = None                                               # (the control: the seed the object was made with)
    with torch.no_grad():
        other = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=0.1, options={"trajectory_kernel": True})
    assert not torch.equal(other, want)


class _Ramp(nn.Module):
    """f = (a0 + a1 t) y + b1 t, g = (c0 + c1 t) y + e0 with dyadic constants: on a dyadic step grid every coefficient row is
    exact in float32 however it is evaluated, so the rows of neighbouring steps differ and both routes see the same floats."""
    noise_type = "diagonal"

    def __init__(self, d, sde_type):
        super().__init__()
        self.sde_type = sde_type
        self.a0 = nn.Parameter(torch.linspace(-0.5, 0.25, d).mul(16).round().div(16))
        self.c0 = nn.Parameter(torch.linspace(0.125, 0.5, d).mul(16).round().div(16))

    def f(self, t, y):
        return (self.a0 + 0.5 * t) * y + 0.25 * t

    def g(self, t, y):
        return (self.c0 + 0.25 * t) * y + 0.125


@pytest.mark.parametrize("shape", [VECTOR, ONE_PER_LANE], ids=["vector", "one_per_lane"])
@pytest.mark.parametrize("method,sde_type", [("euler", "ito"), ("midpoint", "stratonovich")], ids=["euler", "midpoint"])
def test_coefficients_that_depend_on_time(method, sde_type, shape):
    """The forms with one coefficient row per stage time index those rows with k: it must stay this step's."""
    import torchsde_amd
    from torchsde_amd import kernels as K
    sde = _Ramp(shape[1], sde_type).to(DEV)
    y0 = _y0(shape, torch.float32)
    timed = []
    true_launch = K.trajectory_affine_diag

    def recording(ys, y0_, a, *args, **kwargs):
        timed.append(a.dim() == 2)
        return true_launch(ys, y0_, a, *args, **kwargs)

    K.trajectory_affine_diag = recording
    try:
        for times in ([0.0, 0.3125, 1.0], OUTPUT_GRIDS["two inside one step"], [0.0, DT], [0.0, 3 * DT]):
            ts = torch.tensor(times, device=DEV)
            with torch.no_grad():
                runs = [torchsde_amd.sdeint(sde, y0, ts, bm=_bm(y0, ts, method), method=method, dt=DT,
                                            options={"hip_graph": False, "trajectory_kernel": route})
                        for route in (True, True, False)]          # (the first solve of a module verifies the recognition)
            assert torch.equal(runs[1], runs[2]), times
            assert torch.equal(runs[0], runs[2]), times
    finally:
        K.trajectory_affine_diag = true_launch
    assert timed and all(timed), timed
