"""GPU parity of wave pacing in the affine trajectory kernel (TSDE_TRAJ_PACE_WAVES, csrc/trajectory.hip; run with ``-m gpu``):
a wave that lowers its own priority as it advances computes what it computed before. The paced launch, the launch with
``TSDE_WAVE_PACE=0`` and the stepwise route must give the same bytes.

Shapes: 3 x 4 (three lanes), 64 x 4 (one wave), 65 x 64 (two blocks, ragged last wave) and 1024 x 64 take one element per lane,
a form that carries the bit and ignores it; 8192 x 64 is the smallest at which a lane owns a 16-byte group (`kTrajVecMinGroups`),
the form that is paced. Step counts 1 .. 17: below 8 the thresholds coincide. Output grids: the final state; every step; and a
time inside every step at whose end the priority changes -- the change for threshold t is made at the latch of the step that
completes t steps, step t - 1, so the time lies in that step: the set-aside block, the output block and the pacing block in one
turn of the loop. dt = 2^-6 selects the folded (POW2) step of Euler and midpoint, dt = 0.01 the plain one. Methods: the three
that are paced (Euler, midpoint, Heun) and Milstein, which is not."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(3, 4), (64, 4), (65, 64), (1024, 64), (8192, 64)]
STEPS = [1, 2, 3, 7, 8, 9, 16, 17]
DTS = [2.0 ** -6, 0.01]
GRIDS = ["final", "every step", "inside the change steps"]
METHODS = [("euler", "ito"), ("midpoint", "stratonovich"), ("heun", "stratonovich"), ("milstein", "ito")]


def _sde(d, sde_type, shifts):
    import torchsde_amd
    gen = torch.Generator().manual_seed(7)
    rate, shift, vol, vol_shift = (torch.rand(d, generator=gen, dtype=torch.float64) * s + o
                                   for s, o in ((0.6, -0.3), (0.4, -0.2), (0.5, 0.1), (0.2, -0.1)))
    if not shifts:
        shift, vol_shift = torch.zeros(d, dtype=torch.float64), 0.0
    return torchsde_amd.AffineDiagonalSDE(rate, shift, vol, vol_shift, sde_type=sde_type, dtype=torch.float32, device=DEV)


def _change_steps(steps):
    """The steps at whose latch a wave changes its priority: step t - 1 for every threshold t >= 1 (a threshold at 0 is taken
    at kernel entry)."""
    from torchsde_amd import _native
    out = (ctypes.c_int32 * 4)()
    _native.load().tsde_wave_pace(steps, _native.TRAJ_PACE_WAVES, out)
    return sorted({t - 1 for t in out[:3] if t >= 1})


def _ts(steps, dt, grid):
    if grid == "final":
        times = [0.0, steps * dt]
    elif grid == "every step":
        times = [k * dt for k in range(steps + 1)]
    else:
        times = [0.0] + [(k + 0.625) * dt for k in _change_steps(steps)] + [steps * dt]
    return torch.tensor(times, dtype=torch.float32, device=DEV)


def _solve(monkeypatch, sde, y0, ts, method, dt, trajectory, flags=None):
    """`flags`: a list that receives the flags of every trajectory launch as the entry point gets them."""
    import torchsde_amd
    from torchsde_amd import kernels as K
    bm = torchsde_amd.BrownianInterval(float(ts[0]), float(ts[-1]), size=tuple(y0.shape), dtype=y0.dtype, device=DEV, entropy=29)
    true_launch = K.trajectory_affine_diag

    def recording(ys, y0_, a, b, c, e, method_code, schedule, *args, **kwargs):
        flags.append(schedule._launch.flags)
        return true_launch(ys, y0_, a, b, c, e, method_code, schedule, *args, **kwargs)

    with monkeypatch.context() as m:
        if flags is not None:
            m.setattr(K, "trajectory_affine_diag", recording)
        with torch.no_grad():
            return torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=dt, options={"trajectory_kernel": trajectory})


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_an_interior_output_time_meets_every_change_of_priority():
    """The third grid does what it says: for threshold t >= 1 the change is due when t steps are complete, `k + 1 == t` at the
    latch of step k = t - 1, and the grid holds a time strictly inside that step."""
    assert _change_steps(17) == [7, 12, 14]                 # thresholds 8, 13, 15
    assert _change_steps(8) == [3, 5, 6] and _change_steps(2) == [0] and _change_steps(1) == []
    dt = 2.0 ** -6
    inside = _ts(17, dt, "inside the change steps").tolist()[1:-1]
    assert [int(t / dt) for t in inside] == [7, 12, 14] and all((t / dt) % 1 == 0.625 for t in inside)


@pytest.mark.parametrize("method,sde_type", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_paced_launch_gives_the_bytes_of_the_unpaced_launch_and_of_the_stepwise_route(shape, method, sde_type, monkeypatch):
    from torchsde_amd import _native
    sde = _sde(shape[1], sde_type, shifts=shape[0] % 2 == 1)     # (3 and 65 rows: with shifts; the others: the linear form)
    y0 = torch.linspace(-1.5, 1.5, shape[0] * shape[1], dtype=torch.float32, device=DEV).reshape(shape)
    for steps in STEPS:
        for dt in DTS:
            for grid in GRIDS:
                ts = _ts(steps, dt, grid)
                where = f"steps={steps} dt={dt} grid={grid}"
                monkeypatch.delenv("TSDE_WAVE_PACE", raising=False)
                flags = []
                paced = _solve(monkeypatch, sde, y0, ts, method, dt, True, flags)
                assert len(flags) == 1 and flags[0] & _native.TRAJ_PACE_WAVES, where
                monkeypatch.setenv("TSDE_WAVE_PACE", "0")
                flags = []
                unpaced = _solve(monkeypatch, sde, y0, ts, method, dt, True, flags)
                assert len(flags) == 1 and not flags[0] & _native.TRAJ_PACE_WAVES, where
                monkeypatch.delenv("TSDE_WAVE_PACE")
                stepwise = _solve(monkeypatch, sde, y0, ts, method, dt, False)
                assert paced.shape == (len(ts),) + shape and torch.isfinite(paced).all(), where
                assert _same_bytes(paced, unpaced), where
                assert _same_bytes(paced, stepwise), where
