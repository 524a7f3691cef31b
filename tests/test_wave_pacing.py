"""Wave pacing of the affine trajectory kernel (TSDE_TRAJ_PACE_WAVES, csrc/tsde_common.h `wave_pace`), through the host
exports that share the kernel's definition: where the thresholds lie, which levels a wave walks, and the switch."""
import ctypes

import numpy as np
import pytest
import torch

from torchsde_amd import _native
from torchsde_amd import kernels as K

N_STEPS = list(range(1, 41)) + [63, 64, 65, 1000, 1023, 1024, 4097, 10 ** 6, 2 ** 31 - 1]


def _pace(n_steps, flags=_native.TRAJ_PACE_WAVES):
    out = (ctypes.c_int32 * 4)()
    _native.load().tsde_wave_pace(n_steps, flags, out)
    return list(out[:3]), out[3]


def _walk(n_steps, flags=_native.TRAJ_PACE_WAVES, limit=64):
    """The (step, level) sequence of a wave, as the kernel's loop makes it: it enters at level 3 if a change is due at all, and
    at the step that equals the carried step count it takes the change and carries the next."""
    lib = _native.load()
    at, nxt = _pace(n_steps, flags)
    walk = [(0, 3)] if nxt >= 0 else []
    while nxt >= 0:
        assert len(walk) < limit
        k, level = nxt, ctypes.c_int32(-1)
        nxt = lib.tsde_wave_pace_change(n_steps, k, ctypes.byref(level))
        assert nxt == -1 or k < nxt < n_steps             # the next change lies ahead, inside the loop
        walk.append((k, level.value))
    return walk


@pytest.mark.parametrize("n_steps", N_STEPS)
def test_thresholds_are_ordered_and_inside_the_solve(n_steps):
    (t1, t2, t3), first = _pace(n_steps)
    assert 0 <= t1 <= t2 <= t3 <= n_steps
    assert first == t1
    if n_steps >= 8:
        assert (t1, t2, t3) == (n_steps // 2, n_steps - n_steps // 4, n_steps - n_steps // 8)
    assert t3 <= n_steps - 1                               # the last step, at least, runs at priority 0


@pytest.mark.parametrize("n_steps", N_STEPS)
def test_levels_fall_and_end_at_zero(n_steps):
    walk = _walk(n_steps)
    steps, levels = [k for k, _ in walk], [lv for _, lv in walk]
    assert levels[0] == 3 and levels[-1] == 0
    assert all(a > b for a, b in zip(levels, levels[1:]))           # never repeated, never raised
    assert all(a <= b for a, b in zip(steps, steps[1:])) and steps[-1] <= n_steps - 1
    assert all(a < b for a, b in zip(steps[1:], steps[2:]))         # one change per step at the most
    at, _ = _pace(n_steps)
    for k, level in walk[1:]:
        assert level == 3 - sum(1 for t in at if t <= k)            # the level of step k by the thresholds' definition


def test_collisions_skip_levels():
    assert [lv for _, lv in _walk(1)] == [3, 0]                     # 0, 0, 0: straight to the last level
    assert [lv for _, lv in _walk(2)] == [3, 0]                     # 1, 1, 1
    assert [lv for _, lv in _walk(4)] == [3, 2, 0]                  # 2, 3, 3
    assert [lv for _, lv in _walk(7)] == [3, 2, 0]                  # 3, 6, 6
    assert [lv for _, lv in _walk(8)] == [3, 2, 1, 0]               # 4, 6, 7
    assert _walk(1000) == [(0, 3), (500, 2), (750, 1), (875, 0)]


@pytest.mark.parametrize("n_steps", N_STEPS)
def test_without_the_flag_no_change_is_ever_due(n_steps):
    for flags in (0, _native.TRAJ_POW2_STEPS):
        at, first = _pace(n_steps, flags)
        assert first == -1 and at == _pace(n_steps)[0]
        assert _walk(n_steps, flags) == []


def _schedule(n):
    rows = np.zeros((n, 8), dtype=np.float32)
    rows[:, 0] = rows[:, 6] = 2.0 ** -10
    rows[:, 1], rows[:, 4] = 2.0 ** -11, 2.0 ** -5
    return K.TrajectorySchedule.cached(rows, np.arange(n), [n], [(0.0, 1.0)], torch.device("cpu"), torch.float32)


def test_schedule_sets_the_bit_unless_switched_off(monkeypatch):
    assert _native.TRAJ_PACE_WAVES == 2 and _native.TRAJ_PACE_WAVES & _native.TRAJ_POW2_STEPS == 0
    monkeypatch.delenv("TSDE_WAVE_PACE", raising=False)
    monkeypatch.delenv("TSDE_POW2_STEPS", raising=False)
    on = _schedule(9)
    assert on.pace_waves and on._launch.flags == _native.TRAJ_POW2_STEPS | _native.TRAJ_PACE_WAVES
    assert on._struct.flags == _native.TRAJ_POW2_STEPS              # what is known of the rows stays what it was
    assert ctypes.addressof(on.struct()._obj) == ctypes.addressof(on._launch)
    assert (on._launch.step_rows, on._launch.cells, on._launch.n_steps, on._launch.n_out) == \
        (on._struct.step_rows, on._struct.cells, 9, 1)
    monkeypatch.setenv("TSDE_WAVE_PACE", "0")
    off = _schedule(9)
    assert off is not on and not off.pace_waves and off._launch.flags == _native.TRAJ_POW2_STEPS
    assert _schedule(9) is off
    monkeypatch.delenv("TSDE_WAVE_PACE")
    assert _schedule(9) is on
