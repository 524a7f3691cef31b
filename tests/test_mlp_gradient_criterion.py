"""The case table of the perceptron training kernels' gradient tests (tests/helpers.py, `mlp_grad_cases`) and the criterion
they are held to -- `helpers.assert_within_reference_rounding` with `MLP_GRAD_FACTOR` and `MLP_GRAD_FLOOR` -- can tell a right
gradient from a subtly wrong one: on the CPU, with the oracle alone.

The subtly wrong gradient is that of the module whose `lin1.weight` is larger by one part in ten thousand: what a slightly wrong
slope or constant in a kernel gives. The criterion must reject it for dL/dy0 and for every parameter gradient, on every case of
the table, where `2e-3 * max|want| + 1e-6` (the rule of tests/test_gpu_mlp_backward.py and tests/test_gpu_mlp_adjoint.py)
accepts it; it must reject the gradient of a grid whose middle output is one step late; and it must accept the oracle's own
float32 run on every case, with no allowance for any of them."""
import functools

import pytest
import torch

from tests import helpers

F32, F64 = torch.float32, torch.float64
CASES = helpers.mlp_grad_cases()
GRADIENTS = helpers.MLP_GRAD_QUANTITIES[1:]                  # dL/dy0 and the six parameter gradients
ids = [case.id for case in CASES]


@functools.lru_cache(maxsize=None)
def _oracle(index):
    return helpers.mlp_grad_oracle(CASES[index])


def _rejected(got, want32, want64):
    try:
        helpers.assert_within_reference_rounding(got, want32, want64, factor=helpers.MLP_GRAD_FACTOR,
                                                 floor=helpers.MLP_GRAD_FLOOR)
    except AssertionError:
        return True
    return False


def _old_rule_accepts(got, want):
    return (got - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-6


def test_the_table_is_what_the_gpu_tests_expect():
    assert len(CASES) == len(helpers.MLP_GRAD_SHAPES) * len(helpers.MLP_GRAD_SCHEMES) and len(set(ids)) == len(ids)
    assert 4.0 <= helpers.MLP_GRAD_FACTOR <= 8.0 and helpers.MLP_GRAD_FLOOR == 1e-6
    # both activations on every shape and under every scheme, without the full product
    for key in ("shape", "scheme"):
        seen = {}
        for case in CASES:
            k = (case.B, case.d, case.hidden) if key == "shape" else (case.route, case.method, case.adjoint_method,
                                                                      case.sde_type, case.diffusion)
            seen.setdefault(k, set()).add(case.activation)
        assert all(v == {"tanh", "softplus"} for v in seen.values()), seen
    # outputs on step boundaries only
    grid = helpers.rheun_grid(CASES[0].ts(), helpers.MLP_GRAD_DT)
    assert grid.n_steps == helpers.MLP_GRAD_STEPS and all((w0, w1) == (0.0, 1.0) for (_, _, w0, w1) in grid.outputs)
    y0 = CASES[1].y0()
    assert y0.unique().numel() == y0.numel()                 # never a constant start
    assert [label for label, _ in CASES[1].cotangents()] == ["all", "first", "middle", "last"]
    for case in helpers.mlp_grad_scalar_cases():
        module = case.module()
        assert module.diff_rate.shape == module.diff_shift.shape == ()


@pytest.mark.parametrize("index", range(len(CASES)), ids=ids)
def test_the_float32_oracle_run_is_accepted_on_every_case(index):
    ref = _oracle(index)
    for label, _ in CASES[index].cotangents():
        for name in helpers.MLP_GRAD_QUANTITIES:
            a32, a64 = ref[F32][label][name], ref[F64][label][name]
            assert a32.shape == a64.shape and torch.isfinite(a32).all() and torch.isfinite(a64).all()
            helpers.assert_within_reference_rounding(a32, a32, a64, f"{label} {name}", factor=helpers.MLP_GRAD_FACTOR,
                                                     floor=helpers.MLP_GRAD_FLOOR)
            # what the criterion multiplies is rounding: sixteen steps of a few float32 roundings (2**-24) each
            err = (a32.double() - a64).abs().max().item()
            assert err <= 2e-6 * max(1.0, a64.abs().max().item()), (label, name, err)
            # a cotangent that reaches a step gives no zero gradient: the comparison is not vacuous
            if label != "first" or name in ("ys", "y0"):
                assert a64.abs().max().item() > 1e-3, (label, name)


@pytest.mark.parametrize("index", range(len(CASES)), ids=ids)
def test_a_slope_wrong_by_one_part_in_ten_thousand_is_rejected_where_the_old_rule_accepts_it(index):
    case = CASES[index]
    true = _oracle(index)
    mutant = case.module()
    with torch.no_grad():
        mutant.lin1.weight.mul_(1.0 + 1e-4)
    wrong = helpers.mlp_grad_oracle(case, sde=mutant, cotangents=case.cotangents()[:1])[F64]["all"]
    for name in GRADIENTS:
        want32, want64 = true[F32]["all"][name], true[F64]["all"][name]
        assert _rejected(wrong[name], want32, want64), f"{name} of the mutant passed for the true module's"
        assert _old_rule_accepts(wrong[name], want64), f"{name}: the old rule sees this mutant after all"


@pytest.mark.parametrize("index", range(len(CASES)), ids=ids)
def test_the_gradient_of_a_middle_output_one_step_late_is_rejected(index):
    case = CASES[index]
    true = _oracle(index)
    j = len(helpers.MLP_GRAD_OUTPUTS) // 2
    shifted = list(helpers.MLP_GRAD_OUTPUTS)
    shifted[j] += 1
    assert shifted[j] < shifted[j + 1]
    middle = [c for c in case.cotangents() if c[0] == "middle"]
    wrong = helpers.mlp_grad_oracle(case, outputs=tuple(shifted), cotangents=middle)[F64]["middle"]
    for name in GRADIENTS:
        assert _rejected(wrong[name], true[F32]["middle"][name], true[F64]["middle"][name]), name


@pytest.mark.parametrize("index", range(len(CASES)), ids=ids)
def test_a_cotangent_on_the_start_alone_comes_back_unchanged(index):
    """L = <w, ys[0]> = <w, y0>: dL/dy0 is w bit for bit, and no parameter is reached."""
    case = CASES[index]
    ref = _oracle(index)
    w = dict(case.cotangents())["first"][0]
    for dtype in (F32, F64):
        got = ref[dtype]["first"]
        assert torch.equal(got["y0"], w.to(dtype))
        for name in GRADIENTS[1:]:
            assert got[name].abs().max().item() == 0.0, name
