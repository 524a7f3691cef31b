"""The reference machine of tests/prog_machine.py, pinned before it judges a kernel (CPU): against the user's own float64 code
and autograd on the named programs and the seeded random trees of tests/test_recognise.py, against itself (float64 torch
against the high-precision variant on every opcode's point set), and -- the arithmetic opcodes, rounded to float32 after each
instruction -- against numpy's float32 arithmetic bit for bit (53 >= 2 * 24 + 2 bits: the double rounding of + - * / sqrt is
innocuous)."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import prog_machine as pm
from tests.test_recognise import _M, PROGRAMS, _random_tree
from torchsde_amd import recognise
from torchsde_amd.sde import ForwardSDE

D = 6
TOL = dict(rtol=1e-12, atol=1e-12)


def _double(sde):
    sde = sde.double()
    sde.b = sde.b.double()
    return sde


def _check_against_the_users_code(sde, found, y, t, want_derivative):
    fw, gw, dgw = found.programs
    table = found.const_table()
    assert table.dtype == torch.float64
    rows = found.trainable_rows() or []
    params = list(sde.parameters())
    for words, fn in ((fw, sde.f), (gw, sde.g)):
        value, dy, drows = pm.reference_slopes(words, table, y, t, rows=rows)
        yy = y.clone().requires_grad_(True)
        out = fn(t, yy).reshape(y.shape[0], -1).expand_as(y)
        torch.testing.assert_close(value, out.detach(), **TOL)
        grads = torch.autograd.grad(out.sum(), [yy] + params, allow_unused=True)
        torch.testing.assert_close(dy, torch.zeros_like(y) if grads[0] is None else grads[0], **TOL)
        # the slopes with respect to the constant rows, carried on to the module's parameters through whatever the user's
        # code derived the rows from (`-s.mu ** 2.`), as kernels._ProgTrajectoryFn.backward does
        surrogate = sum((slope * found.consts[k].reshape(-1).expand(y.shape[1])).sum() for slope, k in zip(drows, rows))
        mine = torch.autograd.grad(surrogate, params, allow_unused=True, retain_graph=True) if rows else [None] * len(params)
        for a, b, p in zip(mine, grads[1:], params):
            zero = torch.zeros_like(p)
            torch.testing.assert_close(zero if a is None else a, zero if b is None else b, **TOL)
    if dgw and want_derivative:
        yy = y.clone().requires_grad_(True)
        dg, = torch.autograd.grad(sde.g(t, yy).reshape(y.shape[0], -1).expand_as(yy).sum(), yy)
        torch.testing.assert_close(pm.run_reference(dgw, table, y, t), dg, **TOL)


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_named_programs_reproduce_the_users_float64_code_and_autograd(name):
    noise, f, g = PROGRAMS[name]
    sde = _double(_M(f, g))
    sde.noise_type = noise
    gen = torch.Generator().manual_seed(3)
    y, t = 0.8 * torch.randn(16, D, generator=gen, dtype=torch.float64), torch.tensor(0.3, dtype=torch.float64)
    # (clamp is followed only where no gradient flows: its backward differs from relu's AT the boundary, which no point here meets)
    found = recognise.recognise_program(ForwardSDE(sde), t, y, noise, differentiable="clamp" not in name)
    _check_against_the_users_code(sde, found, y, t, name != "softplus and abs")


@pytest.mark.parametrize("seed", range(0, 120, 3))
def test_seeded_random_trees_reproduce_the_users_float64_code_and_autograd(seed):
    rng = random.Random(seed)
    src_f, src_g = _random_tree(rng, 5 if seed % 3 == 0 else 4), _random_tree(rng, 4 if seed % 3 == 0 else 3)
    if "y" not in src_f:
        src_f = f"({src_f}) * y"
    if "y" not in src_g:
        src_g = f"({src_g}) + torch.sin(y)"
    env = {"torch": torch, "F": F}
    sde = _double(_M(eval(f"lambda s, t, y: {src_f}", env), eval(f"lambda s, t, y: {src_g}", env)))
    gen = torch.Generator().manual_seed(seed)
    y, t = 2.0 * torch.rand(16, D, generator=gen, dtype=torch.float64) - 1.0, torch.tensor(0.3, dtype=torch.float64)
    try:
        found = recognise.recognise_program(ForwardSDE(sde), t, y, "diagonal", differentiable=True)
    except recognise.NotElementwise:
        return                                   # (tests/test_recognise.py holds the reasons)
    _check_against_the_users_code(sde, found, y, t, True)


def _program(op):
    if op in pm.BINARY:
        return [pm.word(pm.LOAD, pm.CONST, 0), pm.word(op, pm.CONST, 1)]
    return [pm.word(pm.LOAD, pm.CONST, 0), pm.word(op)]


def _finite_points(op):
    """The float64 point set of an opcode as constant rows (2, P), where its value and slopes are finite numbers."""
    if op in pm.FUNCTIONS:
        a = pm.function_points(op, torch.float64)[0]
        b = np.ones_like(a)
    else:
        a, b = pm.arithmetic_points(torch.float64)
    pts = np.stack([a, b])
    value, _, slopes = pm.reference_slopes(_program(op), pts, torch.zeros(pts.shape[1]), 0.0, rows=(0, 1))
    keep = torch.isfinite(value) & torch.isfinite(slopes[0]) & torch.isfinite(slopes[1]) & (value.abs() < 1e300) & \
        (slopes[0].abs() < 1e300) & (slopes[1].abs() < 1e300)
    return pts[:, keep.numpy()][:, ::3]


@pytest.mark.parametrize("op", pm.ARITHMETIC + pm.FUNCTIONS, ids=lambda op: pm.NAMES[op])
def test_float64_and_high_precision_variants_agree(op):
    """To 1e-13 of the value (slopes: of max(1, |slope|) -- autograd forms tanh' as 1 - tanh^2, as the kernels do, and that
    difference is exact to an absolute 1e-16 only)."""
    prog, pts = _program(op), _finite_points(op)
    value, _, slopes = pm.reference_slopes(prog, pts, torch.zeros(pts.shape[1]), 0.0, rows=(0, 1))
    hp_values, hp_slopes = pm.mp_values(prog, pts, seeds=(0, 1))
    assert len(hp_values) > 30
    for c in range(pts.shape[1]):
        hv = float(hp_values[c])
        assert abs(float(value[c]) - hv) <= 1e-13 * abs(hv), (pm.NAMES[op], pts[:, c], float(value[c]), hv)
        for s in (0, 1):
            hs = float(hp_slopes[c][s])
            assert abs(float(slopes[s][c]) - hs) <= 1e-13 * max(1.0, abs(hs)), (pm.NAMES[op], pts[:, c], float(slopes[s][c]), hs)


_NUMPY32 = {pm.ADD: lambda a, b: a + b, pm.SUB: lambda a, b: a - b, pm.RSUB: lambda a, b: b - a, pm.MUL: lambda a, b: a * b,
            pm.DIV: lambda a, b: a / b, pm.RDIV: lambda a, b: b / a, pm.NEG: lambda a, b: -a, pm.ABS: lambda a, b: np.abs(a),
            pm.RELU: lambda a, b: np.where(a > 0, a, np.float32(0)), pm.RECIP: lambda a, b: np.float32(1) / a,
            pm.SQUARE: lambda a, b: a * a, pm.CUBE: lambda a, b: (a * a) * a, pm.SQRT: lambda a, b: np.sqrt(a)}


@pytest.mark.parametrize("op", pm.ARITHMETIC, ids=lambda op: pm.NAMES[op])
def test_arithmetic_rounded_after_each_instruction_is_numpys_float32(op):
    a, b = pm.arithmetic_points(torch.float32)
    gen = np.random.default_rng(op)
    a = np.concatenate([a, pm._rounded(np.ldexp(1 + gen.random(20000), gen.integers(-40, 41, 20000)), torch.float32)])
    b = np.concatenate([b, pm._rounded(np.ldexp(-1 - gen.random(20000), gen.integers(-40, 41, 20000)), torch.float32)])
    pts = torch.from_numpy(np.stack([a, b]))
    got = pm.run_reference(_program(op), pts, torch.zeros(a.size, dtype=torch.float64), 0.0, after=pm.round_to_float32)
    with np.errstate(all="ignore"):
        want = _NUMPY32[op](a.astype(np.float32), b.astype(np.float32)).astype(np.float32)
    got32 = got.numpy().astype(np.float32)
    assert got32.dtype == want.dtype and np.array_equal(got32.view(np.uint32) | (np.isnan(got32) * 0xFFFFFFFF).astype(np.uint32),
                                                        want.view(np.uint32) | (np.isnan(want) * 0xFFFFFFFF).astype(np.uint32))


@pytest.mark.parametrize("op", pm.ARITHMETIC, ids=lambda op: pm.NAMES[op])
def test_float64_arithmetic_is_numpys_float64(op):
    """(sqrt: numpy's, the hardware's correctly rounded one -- torch's vectorised CPU sqrt is not.)"""
    a, b = pm.arithmetic_points(torch.float64)
    got = pm.run_reference(_program(op), torch.from_numpy(np.stack([a, b])), torch.zeros(a.size, dtype=torch.float64), 0.0).numpy()
    f64 = {k: (lambda a, b, fn=fn: fn(a, b)) for k, fn in _NUMPY32.items()}
    f64[pm.RELU], f64[pm.RECIP] = (lambda a, b: np.where(a > 0, a, 0.0)), (lambda a, b: 1.0 / a)
    with np.errstate(all="ignore"):
        want = f64[op](a, b)
    assert want.dtype == np.float64 and ((got == want) | (np.isnan(got) & np.isnan(want))).all()


def test_compare_measures_units_in_the_last_place_and_classes():
    one = np.float32(1)
    up = np.nextafter(one, np.float32(2))
    ulps, right = pm.compare(np.array([up, one, np.inf, np.nan, 0.0, 1.0], dtype=np.float32),
                             np.array([1.0, 1.0 + 2.0 ** -24, 1e39, np.nan, 1e-60, np.inf]), torch.float32)
    assert ulps[0] == 1.0 and ulps[1] == 0.5 and right.tolist() == [True, True, True, True, True, False]
    assert np.isnan(ulps[2:]).all()
    ulps, right = pm.compare(np.array([1.0 + 2.0 ** -52]), [pm.HP.num(1) + pm.HP.num(2) ** -54], torch.float64)
    assert right[0] and abs(ulps[0] - 0.75) < 1e-12
