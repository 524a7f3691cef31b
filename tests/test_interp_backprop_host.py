"""Outputs inside steps under autograd on the perceptron kernels, on the CPU with the oracle alone (no GPU):

1. the reverse step WITH interpolation weights that include/torchsde_amd.h documents for
   tsde_trajectory_mlp_diag_backward_weighted and tsde_trajectory_mlp_diag_logqp_backward_weighted
   (`helpers_interp_backprop.reverse_sweep`, float64 torch ops) is back-propagation through the oracle's stepwise solver;
2. the criterion of tests/test_gpu_interp_backprop.py (`helpers.assert_within_reference_rounding` with INTERP_FACTOR and
   INTERP_FLOOR against the float64 oracle) tells that gradient from three wrong ones: the snapped grid's (a sweep that never
   reads the weights), the one without the w0 share, the one with w0 and w1 exchanged;
3. and accepts the oracle's own float32 run on every grid.

What cannot differ is stated, not skipped: an output at the middle of its step has w0 = w1 (exchanging them is the identity:
`inside`, `first_step`), and the w0 share of an output inside step 1 reaches y0 alone (dropping it leaves every parameter
gradient as it is: `first_step`). Those mutants are held to the quantities they can change, and the exchange also runs on
`chunk_edges`, whose interior outputs sit at quarters."""
import functools

import pytest
import torch

from tests import helpers
from tests import helpers_interp_backprop as I

F32, F64 = torch.float32, torch.float64
SMALL = (6, 8, 16)
CRITERION_SHAPE = (24, 8, 16)
# method, sde type, diffusion: Euler with both diffusions, Milstein with the affine one
HOST_SCHEMES = (("euler", "ito", "affine"), ("euler", "ito", "sigmoid"), ("milstein", "ito", "affine"))


def _case(route, scheme, grid, shape, index=0):
    if route == "plain":
        return I.PlainCase(index, shape, scheme, "tanh" if index % 2 else "softplus", grid)
    return I.KlCase(index, shape, (scheme[0], None, scheme[2]), "tanh" if index % 2 else "softplus", grid)


@functools.lru_cache(maxsize=None)
def _oracle(route, scheme, grid, shape, index, snapped=False):
    case = _case(route, scheme, grid, shape, index)
    ts = helpers.rheun_snapped(case.ts(), I.DT) if snapped else None
    return I.oracle(case, ts=ts)


def _gradient_names(found):
    return [name for name in found if name not in ("ys", "log_ratio")]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", I.INSIDE_GRIDS)
@pytest.mark.parametrize("scheme", HOST_SCHEMES, ids=["-".join(s) for s in HOST_SCHEMES])
@pytest.mark.parametrize("route", ["plain", "logqp"])
def test_the_weighted_reverse_step_is_backpropagation_through_the_stepwise_solver(route, scheme, grid):
    index = HOST_SCHEMES.index(scheme)
    case = _case(route, scheme, grid, SMALL, index)
    ref = _oracle(route, scheme, grid, SMALL, index)
    if route == "logqp":
        assert ref["min_g"] > 0.05             # (the stated step divides by g as it is)
    for entry in case.cotangents():
        label = entry[0]
        want = ref[F64][label]
        got = I.stated_gradients(case, label)
        assert set(got) == set(_gradient_names(want)), (sorted(got), sorted(want))
        for name, value in got.items():
            scale = want[name].abs().max().item()
            assert scale > 0.0 or label == "log_ratio only", (label, name)
            err = (value - want[name]).abs().max().item()
            assert err <= 1e-10 * max(scale, 1e-30) or (scale == 0.0 and err == 0.0), (label, name, err, scale)


def test_the_stated_step_with_every_output_on_a_boundary_is_the_unweighted_one():
    """`aligned`: no weight other than (0, 1), the mutants change nothing."""
    case = _case("plain", HOST_SCHEMES[0], "aligned", SMALL)
    right = I.stated_gradients(case, "all")
    for mutant in ("drop_w0", "exchange"):
        wrong = I.stated_gradients(case, "all", mutant=mutant)
        assert all(torch.equal(wrong[name], right[name]) for name in right)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
CRITERION_CASES = (("plain", ("euler", "ito", "sigmoid")), ("logqp", ("euler", "ito", "sigmoid")))


def _rejected(got, want32, want64):
    """The gradients of `got` the GPU criterion refuses as those of the true grid, and each one's relative distance."""
    rejected, rel = [], {}
    for name in _gradient_names(want64):
        rel[name] = (got[name].double() - want64[name]).abs().max().item() / want64[name].abs().max().item()
        try:
            helpers.assert_within_reference_rounding(got[name], want32[name], want64[name], name, factor=I.INTERP_FACTOR,
                                                     floor=I.INTERP_FLOOR)
        except AssertionError:
            rejected.append(name)
    return rejected, rel


@pytest.mark.parametrize("grid", ["inside", "first_step", "crowded"])
@pytest.mark.parametrize("route,scheme", CRITERION_CASES, ids=[c[0] for c in CRITERION_CASES])
def test_the_gradient_of_the_snapped_grid_is_rejected(route, scheme, grid):
    true = _oracle(route, scheme, grid, CRITERION_SHAPE, 7)
    wrong = _oracle(route, scheme, grid, CRITERION_SHAPE, 7, snapped=True)[F64]["inside"]
    want32, want64 = true[F32]["inside"], true[F64]["inside"]
    rejected, rel = _rejected(wrong, want32, want64)
    print(route, grid, "snapped", " ".join(f"{name} {r:.3g}" for name, r in rel.items()))
    assert rejected == _gradient_names(want64), (rejected, rel)
    assert min(rel.values()) > 1e-3, rel          # (by a wide margin: thousands of times the allowance)


@pytest.mark.parametrize("grid", ["inside", "first_step", "crowded", "chunk_edges"])
@pytest.mark.parametrize("mutant", ["drop_w0", "exchange"])
@pytest.mark.parametrize("route,scheme", CRITERION_CASES, ids=[c[0] for c in CRITERION_CASES])
def test_a_sweep_that_misplaces_the_shares_is_rejected(route, scheme, mutant, grid):
    case = _case(route, scheme, grid, CRITERION_SHAPE, 7)
    true = _oracle(route, scheme, grid, CRITERION_SHAPE, 7)
    want32, want64 = true[F32]["inside"], true[F64]["inside"]
    right = I.stated_gradients(case, "inside")
    wrong = I.stated_gradients(case, "inside", mutant=mutant)
    names = _gradient_names(want64)
    # (the stated step itself passes: what is rejected below is the mutation, not the statement)
    assert _rejected(right, want32, want64)[0] == []
    weights = [(w0, w1) for (_, w0, w1) in I.output_map(case.ts()) if (w0, w1) != (0.0, 1.0)]
    if mutant == "exchange" and all(w0 == w1 for w0, w1 in weights):
        assert grid in ("inside", "first_step")                        # an output at the middle of its step: the identity
        assert all(torch.equal(wrong[name], right[name]) for name in names)
        return
    rejected, rel = _rejected(wrong, want32, want64)
    print(route, grid, mutant, " ".join(f"{name} {r:.3g}" for name, r in rel.items()))
    assert "y0" in rejected, rel
    if mutant == "drop_w0" and grid == "first_step":
        # the only interior output lies in step 1: its w0 share is added to dL/dy_0 after the last products
        assert all(torch.equal(wrong[name], right[name]) for name in names if name != "y0")
        return
    assert rejected == names, (rejected, rel)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(I.GRIDS))
@pytest.mark.parametrize("route,scheme", CRITERION_CASES, ids=[c[0] for c in CRITERION_CASES])
def test_the_float32_oracle_run_is_accepted_on_every_grid(route, scheme, grid):
    case = _case(route, scheme, grid, CRITERION_SHAPE, 7)
    labels = [entry[0] for entry in case.cotangents()]
    assert ("inside" in labels) == (grid in I.INSIDE_GRIDS)
    ref = _oracle(route, scheme, grid, CRITERION_SHAPE, 7)
    for label in labels:
        for name, r64 in ref[F64][label].items():
            r32 = ref[F32][label][name]
            assert torch.isfinite(r64).all() and torch.isfinite(r32).all()
            helpers.assert_within_reference_rounding(r32, r32, r64, f"{label} {name}", factor=I.INTERP_FACTOR,
                                                     floor=I.INTERP_FLOOR)
            # the reference error the criterion multiplies is rounding, not two different grids: float32 rounding through
            # sixteen steps is parts in a million of the quantity's scale, a misplaced output parts in a thousand (above)
            err = (r32.double() - r64).abs().max().item()
            assert err <= 1e-4 * max(1.0, r64.abs().max().item()), (grid, label, name, err)
        assert ref[F64][label]["y0"].abs().max().item() > 1e-3


# ---- the host side of the routes: one launch's output list ----------------------------------------------------------------------
@pytest.mark.parametrize("grid", sorted(I.GRIDS))
def test_the_merged_output_list_holds_every_boundary_and_every_interior_output(grid):
    from torchsde_amd import kernels as K
    outputs = I.output_map(I.grid_ts(grid))
    n_steps = helpers.rheun_grid(I.grid_ts(grid), I.DT).n_steps
    omap = K.OutputMap([k for k, _, _ in outputs], [(w0, w1) for _, w0, w1 in outputs])
    assert (omap.weights is None) == (grid not in I.INSIDE_GRIDS)
    for marks in (range(1, n_steps + 1), set(range(n_steps, 0, -5)) | omap.boundary_outputs()):
        out_step, out_w, row_of_boundary, out_rows = omap.layout(marks)
        assert out_step == sorted(out_step) and len(out_step) == len(out_w)          # the emitter walks ascending steps
        assert all(out_step[row_of_boundary[k] - 1] == k and out_w[row_of_boundary[k] - 1] == (0.0, 1.0) for k in marks)
        assert row_of_boundary[0] == 0 and out_rows[0] == 0
        for j, (k, w0, w1) in enumerate(outputs):
            row = out_rows[j + 1]
            assert out_step[row - 1] == k and out_w[row - 1] == (w0, w1)
        inside = sum((w0, w1) != (0.0, 1.0) for _, w0, w1 in outputs)
        assert len(out_step) == len(set(marks)) + inside
    if omap.weights is not None:
        rows = omap.boundary_rows(n_steps, "cpu")
        out_step = omap.layout(range(1, n_steps + 1))[0]
        assert rows[0] == 0 and [out_step[r - 1] for r in rows[1:].tolist()] == list(range(1, n_steps + 1))
        assert omap.grad_w("cpu").shape == (len(outputs) + 1, 2) and omap.grad_w("cpu")[0].tolist() == [0.0, 1.0]
    assert omap.grad_step("cpu").tolist() == [0] + [k for k, _, _ in outputs]
