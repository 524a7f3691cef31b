"""The output-time grids of the reversible-Heun gradient tests (tests/helpers.py, `RHEUN_GRIDS`) can tell a right gradient from
a wrong one -- on the CPU, with the oracle alone.

The wrong gradient is the one a backward sweep returns that never reads the interpolation weights: the whole cotangent of an
output inside a step lands on that step's right boundary. It is the gradient of the SNAPPED grid (`helpers.rheun_snapped`),
which the oracle can state exactly. The criterion of the GPU tests -- `helpers.assert_within_reference_rounding` with the
project's factor 6 and floor 2e-6 -- must reject it where the cotangent sits on the interpolated outputs, and must accept the
oracle's own float32 run on every grid (no grid needs an allowance of its own)."""
import pytest
import torch

from tests import helpers

B, ENTROPY = 24, 7


def _oracle(name, ts_list, cotangents):
    make, d, m = helpers.rheun_modules()[name]
    y0 = torch.full((B, d), 0.2)
    return helpers.grid_oracle(make(), m, ts_list, range(B), ENTROPY, y0, cotangents)


def _quantities(ref, label):
    return [ref[0]] + ref[1][label]


@pytest.mark.parametrize("name", ["sde_gan_2", "neural_diagonal"])
@pytest.mark.parametrize("grid", sorted(helpers.RHEUN_GRIDS))
def test_the_float32_oracle_run_is_accepted_on_every_grid(name, grid):
    d = helpers.rheun_modules()[name][1]
    ts_list = helpers.rheun_ts(grid)
    cotangents = helpers.rheun_cotangents(ts_list, B, d, seed=17)
    assert [label for label, _ in cotangents] == (["all", "inside"] if grid in ("inside", "crowded", "first_step") else ["all"])
    refs = _oracle(name, ts_list, cotangents)
    for label, _ in cotangents:
        r32, r64 = _quantities(refs[torch.float32], label), _quantities(refs[torch.float64], label)
        for i, (a32, a64) in enumerate(zip(r32, r64)):
            assert torch.isfinite(a64).all() and torch.isfinite(a32).all()
            # the oracle's two precisions agree to float32 rounding on every grid: the reference error the criterion
            # multiplies is rounding, not a difference between two grids
            err = (a32.double() - a64).abs().max().item()
            assert err <= 2e-6 * max(1.0, a64.abs().max().item()), (grid, label, i, err)
        # (a cotangent that is not all zero gives a gradient that is not: the comparison is not vacuous)
        assert r64[1].abs().max().item() > 1e-3


@pytest.mark.parametrize("name", ["sde_gan_2", "neural_diagonal"])
@pytest.mark.parametrize("grid", ["inside", "first_step", "crowded"])
def test_the_gradient_of_the_snapped_grid_is_rejected(name, grid):
    d = helpers.rheun_modules()[name][1]
    ts_list = helpers.rheun_ts(grid)
    snapped = helpers.rheun_snapped(ts_list)
    assert snapped != ts_list and len(snapped) == len(ts_list)
    cotangents = helpers.rheun_cotangents(ts_list, B, d, seed=17)
    true = _oracle(name, ts_list, cotangents)
    wrong = _oracle(name, snapped, cotangents)[torch.float64]
    want32, want64 = _quantities(true[torch.float32], "inside"), _quantities(true[torch.float64], "inside")
    got = _quantities(wrong, "inside")
    rejected = []
    for i in range(1, len(got)):                                       # dL/dy0 and every parameter gradient
        try:
            helpers.assert_within_reference_rounding(got[i], want32[i], want64[i], f"quantity {i}", factor=6.0, floor=2e-6)
        except AssertionError:
            rejected.append(i)
    assert 1 in rejected, "dL/dy0 of the snapped grid passed for the true grid's"
    assert len(rejected) == len(got) - 1, (rejected, len(got))
    # and by a wide margin: every gradient is wrong by thousands of times the allowance, the weights' by a large part of
    # their largest entry (dy/dy0 is close to the identity over one step, so dL/dy0 moves least)
    rel = [(got[i] - want64[i]).abs().max().item() / want64[i].abs().max().item() for i in range(1, len(got))]
    print(grid, name, " ".join(f"{r:.3g}" for r in rel))
    assert min(rel) > 1e-3 and max(rel) > 0.1, rel


def test_a_schedule_that_interpolates_is_refused_a_gradient_before_anything_is_launched():
    """`TrajectorySchedule.on_boundaries` on the host, and `neural_rheun.solve` reading it first: the refusal needs no GPU."""
    import numpy as np
    from torchsde_amd import _native, kernels as K, neural_rheun
    rows = np.zeros((4, 8))
    rows[:, 0] = helpers.RHEUN_DT
    cpu = torch.device("cpu")
    aligned = K.TrajectorySchedule(rows, np.arange(4), [2, 4], [(0.0, 1.0), (0.0, 1.0)], cpu, torch.float32)
    inside = K.TrajectorySchedule(rows, np.arange(4), [2, 4], [(0.5, 0.5), (0.0, 1.0)], cpu, torch.float32)
    assert aligned.on_boundaries and not inside.on_boundaries
    grid = helpers.rheun_grid(helpers.rheun_ts("crowded"))
    assert [(w0, w1) == (0.0, 1.0) for (_, _, w0, w1) in grid.outputs] == [False, False, False, True, True]
    d, hidden = 4, 8
    lin = lambda a, b: (torch.randn(b, a, requires_grad=True), None)                          # noqa: E731
    f = neural_rheun.DeepNet([lin(d, hidden), lin(hidden, d)], _native.ACT_TANH)
    g = neural_rheun.DeepNet([lin(d, hidden), lin(hidden, d)], _native.ACT_TANH)
    times = np.arange(5, dtype=np.float32) * np.float32(helpers.RHEUN_DT)
    with pytest.raises(ValueError, match="step boundaries"):
        neural_rheun.solve(torch.zeros(3, d), f, g, _native.NOISE_DIAGONAL, d, inside, times, None)
