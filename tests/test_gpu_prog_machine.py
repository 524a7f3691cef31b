"""The program machine of csrc/trajectory.hip -- `tsde_trajectory_prog_diag`, `.._sens`, `.._additive` and the units
torchsde_amd/specialise.py generates from the same words -- held to an independent statement of what every instruction word
means (``-m gpu``): tests/prog_machine.py, which tests/test_prog_machine_reference.py pins on the CPU. Hand-written words go
through the C ABI; a one-step solve with the noise scale set to zero reads a program's value, and a tangent plane the slope the
kernel formed, back exactly.

  a  structure, bit for bit on dyadic inputs: sources, operand order, the stack, constant rows, program offsets, steps, outputs,
     stage times of f, tangent planes
  b  the arithmetic opcodes, bit for bit: float32 = the float64 reference rounded after each instruction, float64 = IEEE
  c  the function opcodes, held to torch's operator of the same name on the device: per sign and binade the kernel's largest
     ulp error is at most max(1, 2 E_torch) (profiles/prog_machine_accuracy.txt is `accuracy_table()` of a run on the MI355X)
  d  generated units = the interpreter bit for bit on a 24-step solve with real noise, at both lane widths; the interpreter within
     1e-11 of the reference machine replayed through the oracle

Everything runs for float32 and float64, on the interpreter with one element per lane (ONE) and four (VEC), and on the
sensitivity kernel. The stage times of g cannot be seen with zero noise: they stay with
tests/test_gpu_programs.py::test_time_as_an_operand_of_the_programs."""
import concurrent.futures
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import prog_machine as pm
from tests.prog_machine import (ABS, ADD, CONST, COS, CUBE, DIV, DUP, EXP, LOAD, LOG, MUL, NEG, RDIV, RECIP, RELU, RSUB, SIGMOID,
                                SIN, SOFTPLUS, SQRT, SQUARE, STACK, STATE, SUB, TANH, TIME, ONE, VEC, word)

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float64]
TARGETS = [("values", ONE), ("values", VEC), ("sens", ONE)]
TARGET_IDS = ["one", "vec", "sens"]
both = pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
targets = pytest.mark.parametrize("target", TARGETS, ids=TARGET_IDS)


def _read(target, dtype, prog, points, **kw):
    got = pm.read_out(target[0], dtype, target[1], prog, points, **kw)
    return got[0] if target[0] == "sens" else got


def _exact(got, want):
    """Bit for bit, up to the sign of a zero."""
    got = np.ascontiguousarray(got).reshape(-1)
    with np.errstate(all="ignore"):
        want = np.asarray(want, dtype=np.float64)
        want = np.broadcast_to(want, got.shape if want.ndim == 0 else want.shape).astype(got.dtype).reshape(-1)
    assert got.shape == want.shape
    assert pm.same_bits(torch.from_numpy(got), torch.from_numpy(want)), \
        [(i, got[i], want[i]) for i in np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]]


# ---- a. structure --------------------------------------------------------------------------------------------------------------
# dyadic operands: multiples of 1/16 up to 4 in magnitude, never zero, and powers of two as divisors
_X = np.array([n / 16.0 for n in range(-64, 65) if n != 0][::3])
_Y = np.roll(_X, 7) * np.where(np.arange(_X.size) % 2 == 0, 1.0, -0.5)
_POW2 = np.array([(-1.0) ** k * 2.0 ** (k % 5 - 2) for k in range(_X.size)])
_EXPECT = {ADD: lambda a, b: a + b, SUB: lambda a, b: a - b, RSUB: lambda a, b: b - a, MUL: lambda a, b: a * b,
           DIV: lambda a, b: a / b, RDIV: lambda a, b: b / a}


def _operands(op):
    return (_X, _POW2) if op == DIV else ((_POW2, _X) if op == RDIV else (_X, _Y))


@both
@targets
@pytest.mark.parametrize("slot", ["f", "g", "dg"])
def test_load_from_every_source_through_every_slot(target, dtype, slot):
    _exact(_read(target, dtype, [word(LOAD, CONST, 1)], np.stack([_X, _Y]), slot=slot), _Y)
    _exact(_read(target, dtype, [word(LOAD, STATE)], _X[None], slot=slot, state=_Y), _Y + _Y)
    _exact(_read(target, dtype, [word(LOAD, TIME)], _X[None], slot=slot, t0=2.75), np.full(_X.size, 2.75))


@both
@targets
@pytest.mark.parametrize("op", pm.BINARY, ids=lambda op: pm.NAMES[op])
def test_binary_operators_take_a_from_the_stack_and_b_from_the_source(target, dtype, op):
    """A op B (RSUB, RDIV: B op A) with A the top of the stack and B the source; with the stack as the source A is the value
    BELOW the top. The operands are never interchangeable."""
    a, b = _operands(op)
    want = _EXPECT[op](a, b)
    assert op in (ADD, MUL) or not np.array_equal(want, _EXPECT[op](b, a))
    pts = np.stack([a, b])
    _exact(_read(target, dtype, [word(LOAD, CONST, 0), word(op, CONST, 1)], pts), want)
    _exact(_read(target, dtype, [word(LOAD, CONST, 0), word(LOAD, CONST, 1), word(op, STACK)], pts), want)
    _exact(_read(target, dtype, [word(LOAD, CONST, 0), word(op, STATE)], pts, state=b), b + want)
    t0 = 0.5
    _exact(_read(target, dtype, [word(LOAD, CONST, 0), word(op, TIME)], pts, t0=t0), _EXPECT[op](a, np.full_like(a, t0)))


@both
@targets
def test_dup_and_the_four_stack_slots(target, dtype):
    pts = np.stack([_X, _Y, _POW2, np.roll(_X, 3)])
    c0, c1, c2, c3 = pts
    for op in (ADD, SUB, MUL, DIV):
        _exact(_read(target, dtype, [word(LOAD, CONST, 0), word(DUP), word(op, STACK)], pts), _EXPECT[op](c0, c0))
    # DUP above another value: c1 + c0 * c0
    _exact(_read(target, dtype, [word(LOAD, CONST, 1), word(LOAD, CONST, 0), word(DUP), word(MUL, STACK), word(ADD, STACK)], pts),
           c1 + c0 * c0)
    # four slots, popped in order: the bottom one survives three pushes
    prog = [word(LOAD, CONST, k) for k in range(4)] + [word(SUB, STACK)] * 3
    _exact(_read(target, dtype, prog, pts), c0 - (c1 - (c2 - c3)))
    prog = [word(LOAD, CONST, 0), word(LOAD, CONST, 1), word(LOAD, CONST, 2), word(DUP), word(MUL, STACK), word(RSUB, STACK),
            word(MUL, STACK)]
    _exact(_read(target, dtype, prog, pts), c0 * (c2 * c2 - c1))


@both
@targets
def test_constant_rows_on_both_sides_of_the_register_boundary(target, dtype):
    """64 rows with distinct values; 0 and 7 live in registers, 8 and 63 are read through the cache. (Row 62 is the 0 and row 61
    the -2 of the read-out.)"""
    P = 70
    table = np.array([[((r * 5 + c * 3) % 61 + 1) / 16.0 for c in range(P)] for r in range(64)])
    table[62], table[61] = 0.0, -2.0
    for slot in ("f", "g", "dg"):
        for k in (0, 7, 8, 63):
            _exact(_read(target, dtype, [word(LOAD, CONST, k)], table, slot=slot, aux=(62, 61)), table[k])
    prog = [word(LOAD, CONST, 0), word(MUL, CONST, 7), word(ADD, CONST, 8), word(SUB, CONST, 63), word(RSUB, CONST, 9)]
    _exact(_read(target, dtype, prog, table, aux=(62, 61)), table[9] - (table[0] * table[7] + table[8] - table[63]))


def _chain(row, step_row, n):
    """n words: LOAD const(row), then n - 1 times ADD const(step_row)."""
    return [word(LOAD, CONST, row)] + [word(ADD, CONST, step_row)] * (n - 1)


@both
@targets
@pytest.mark.parametrize("lengths", [(1, 1, 94), (94, 1, 1), (32, 32, 32)], ids=str)
def test_programs_at_the_word_limit_start_at_their_own_offsets(target, dtype, lengths):
    """f, g and g' of a Milstein Ito step from 0 with W = 0: y1 = f + (g * (-1/2)) * g'; all three are read, every word counts."""
    kind, shape = target
    d = shape[1]
    consts = np.stack([1 + (np.arange(d) % 8) / 8.0, np.full(d, 1 / 16.0), -2 - (np.arange(d) % 4) / 4.0, np.full(d, 1 / 8.0),
                       0.5 + (np.arange(d) % 2), np.full(d, 1 / 32.0)])
    f, g, dg = (_chain(2 * i, 2 * i + 1, n) for i, n in enumerate(lengths))
    assert len(f) + len(g) + len(dg) == pm.MAX_WORDS
    ys, _, _ = pm.solve(kind, dtype, shape, f, g, dg, consts, method=pm.MILSTEIN_ITO)
    value = [consts[2 * i] + (n - 1) * consts[2 * i + 1] for i, n in enumerate(lengths)]
    want = value[0] + (value[1] * -0.5) * value[2]
    _exact(ys[0].cpu().numpy(), np.broadcast_to(want, shape))


@both
@pytest.mark.parametrize("kind", ["values", "sens", "additive"])
def test_97_words_are_refused_and_nothing_is_written(dtype, kind):
    consts = np.ones((2, ONE[1]))
    f = _chain(0, 1, 95 if kind != "additive" else 97)
    g = dg = [] if kind == "additive" else [word(LOAD, CONST, 0)]
    ys, sens, rc = pm.solve(kind, dtype, ONE, f, g, dg, consts, method=pm.EULER, check=False, fill=7.0)
    assert rc != 0 and bool((ys == 7.0).all()) and (sens is None or bool((sens == 7.0).all()))


@both
@targets
@pytest.mark.parametrize("scalar_noise", [0, 1])
def test_scalar_and_diagonal_noise_read_the_same_programs(target, dtype, scalar_noise):
    prog = [word(LOAD, CONST, 0), word(MUL, CONST, 1), word(SUB, TIME)]
    for slot in ("f", "g", "dg"):
        _exact(_read(target, dtype, prog, np.stack([_X, _Y]), slot=slot, t0=0.25, scalar_noise=scalar_noise), _X * _Y - 0.25)


@both
@targets
def test_the_state_is_carried_and_the_time_is_read_at_every_step(target, dtype):
    kind, shape = target
    consts = np.zeros((1, shape[1]))
    zero = [word(LOAD, CONST, 0)]
    ys, _, _ = pm.solve(kind, dtype, shape, [word(LOAD, TIME)], zero, zero, consts,
                        step_rows=[pm.read_row(t) for t in (1.0, 2.0, 4.0)], out_step=[1, 2, 3])
    for j, want in enumerate((1.0, 3.0, 7.0)):
        assert bool((ys[j] == want).all())


@both
@targets
def test_an_output_inside_the_step_interpolates_values_and_every_tangent_plane(target, dtype):
    """f = c0 y + c1 + c2 c3 from a non-zero state, one output at out_w = (1/4, 3/4) and one on the boundary."""
    kind, shape = target
    d = shape[1]
    c = np.stack([(np.arange(d) % 7 - 3) / 4.0, (np.arange(d) % 5) / 8.0, 1 + (np.arange(d) % 3) / 2.0, (np.arange(d) % 4 - 1.5) / 2.0,
                  np.zeros(d)])
    y0 = np.array(np.broadcast_to(0.5 + (np.arange(d) % 9) / 8.0, shape))
    f = [word(LOAD, CONST, 0), word(MUL, STATE), word(ADD, CONST, 1), word(LOAD, CONST, 2), word(MUL, CONST, 3), word(ADD, STACK)]
    zero = [word(LOAD, CONST, 4)]
    ys, sens, _ = pm.solve(kind, dtype, shape, f, zero, zero, c, y0=y0, out_step=[1, 1], out_w=[(0.25, 0.75), (0.0, 1.0)],
                           param_slot={0: 1, 1: 2, 2: 3, 3: 4})
    y1 = y0 + (c[0] * y0 + c[1] + c[2] * c[3])
    _exact(ys[0].cpu().numpy(), 0.25 * y0 + 0.75 * y1)
    _exact(ys[1].cpu().numpy(), y1)
    if sens is not None:
        planes = [1 + c[0], y0, np.ones(shape), c[3], c[2]]          # of y1; at the start of the step only plane 0 is set (to 1)
        for s, plane in enumerate(planes):
            plane = np.broadcast_to(plane, shape)
            _exact(sens[1, s].cpu().numpy(), plane)
            _exact(sens[0, s].cpu().numpy(), 0.25 * (1.0 if s == 0 else 0.0) + 0.75 * plane)


def _stage_time_expectation(method, T, t0, dt, additive):
    t0, dt = T(t0), T(dt)
    if method in (pm.EULER, pm.MILSTEIN_ITO, pm.MILSTEIN_STRAT, pm.EULER_HEUN):
        return t0 * dt
    if method == pm.MIDPOINT:
        return (t0 + T(0.5) * dt) * dt
    if method == pm.HEUN:
        return (dt * (t0 + (t0 + dt))) * T(0.5)
    assert method == pm.SRK
    if additive:                                     # SRA1: f at t0 and t0 + 3/4 dt, weights 1/3 and 2/3
        acc = T(0) + (T(1.0 / 3) * t0) * dt
        return acc + (T(2.0 / 3) * (t0 + T(0.75) * dt)) * dt
    acc = T(0)                                       # SRID2, in the order of srid2_final: slots t0, t0 + dt, t0 + dt/2
    for alpha, t in ((1.0 / 6, t0), (1.0 / 6, t0 + dt), (2.0 / 3, t0 + T(0.5) * dt)):
        acc = acc + (T(alpha) * t) * dt
    return acc


_METHODS = ["euler", "milstein_ito", "milstein_strat", "midpoint", "srk", "heun", "euler_heun"]
_STAGE_CASES = [(t, m) for t in TARGETS for m in range(7)] + \
    [(("additive", s), m) for s in (ONE, VEC) for m in (pm.EULER, pm.MIDPOINT, pm.SRK)]
_STAGE_IDS = [f"{i}-{_METHODS[m]}" for i in TARGET_IDS for m in range(7)] + \
    [f"additive-{s}-{_METHODS[m]}" for s in ("one", "vec") for m in (pm.EULER, pm.MIDPOINT, pm.SRK)]


@both
@pytest.mark.parametrize("target,method", _STAGE_CASES, ids=_STAGE_IDS)
def test_stage_times_of_the_drift(target, dtype, method):
    """f = LOAD time with t0 = 5 and dt = 1/4 and no noise: the step shows at which times the scheme evaluated f and with which
    weights. (Those of g cannot be seen with zero noise: tests/test_gpu_programs.py::test_time_as_an_operand_of_the_programs.)"""
    kind, shape = target
    t0, dt = 5.0, 0.25
    zero = [] if kind == "additive" else [word(LOAD, CONST, 0)]
    ys, _, _ = pm.solve(kind, dtype, shape, [word(LOAD, TIME)], zero, zero, np.zeros((1, shape[1])), method=method,
                        step_rows=[[dt, dt / 2, 1 / dt, 0.5, 0.0, 0.0, 0.0, t0]])
    want = _stage_time_expectation(method, pm.np_dtype(dtype), t0, dt, kind == "additive")
    assert want.dtype == pm.np_dtype(dtype)
    _exact(ys[0].cpu().numpy(), np.full(shape, want))


@both
def test_tangent_planes_of_rows_and_of_the_exact_operators(dtype):
    a, b = _X, _Y
    pts = np.zeros((12, a.size))
    pts[0], pts[3], pts[7], pts[9], pts[5] = a, b, np.roll(a, 5), np.roll(b, 2), 0.75
    slots = {0: 1, 3: 2, 9: 3, 7: 4, 5: -1}

    def planes(prog, state=None):
        return pm.read_out("sens", dtype, ONE, prog, pts, param_slot=slots, state=state)

    for k, s in slots.items():                       # a row's own plane is 1, every other 0; a row with -1 has none
        value, got = planes([word(LOAD, CONST, k)])
        _exact(value, pts[k])
        for plane in range(1, 5):
            _exact(got[plane], np.full(a.size, 1.0 if plane == s else 0.0))
        _exact(got[0], np.ones(a.size))              # d y1 / d y0 = 1 + df/dy
    _, got = planes([word(LOAD, CONST, 0), word(MUL, STATE)], state=b)
    _exact(got[0], 1 + a)
    _exact(got[1], b)
    _, got = planes([word(LOAD, CONST, 0), word(MUL, CONST, 3)])
    _exact(got[1], b), _exact(got[2], a)
    _, got = planes([word(LOAD, CONST, 0), word(LOAD, CONST, 3), word(MUL, STACK)])
    _exact(got[1], b), _exact(got[2], a)
    for op, sign in ((ADD, (1, 1)), (SUB, (1, -1)), (RSUB, (-1, 1))):
        for prog in ([word(LOAD, CONST, 0), word(op, CONST, 3)], [word(LOAD, CONST, 0), word(LOAD, CONST, 3), word(op, STACK)]):
            _, got = planes(prog)
            _exact(got[1], np.full(a.size, sign[0])), _exact(got[2], np.full(a.size, sign[1]))
    _, got = planes([word(LOAD, CONST, 0), word(DUP), word(MUL, STACK)])
    _exact(got[1], 2 * a)


@both
@pytest.mark.parametrize("stack", [False, True], ids=["const", "stack"])
@pytest.mark.parametrize("op", [DIV, RDIV], ids=["DIV", "RDIV"])
def test_quotient_tangents_within_three_ulp(dtype, op, stack):
    """d(a/b)/da = 1/b and d(a/b)/db = -(a/b)/b: three roundings (a/b, 1/b, their product), each half an ulp relative -- a whole
    one just above a power of two."""
    T = pm.np_dtype(dtype)
    rng = np.random.default_rng(5)
    num = pm._rounded((1 + rng.random(400)) * rng.choice([-1, 1], 400) * 2.0 ** rng.integers(-3, 4, 400), dtype)
    den = pm._rounded((1 + rng.random(400)) * rng.choice([-1, 1], 400) * 2.0 ** rng.integers(-3, 4, 400), dtype)
    den[:8] = [3, 5, 7, 1 + 2.0 ** -10, 3 / 16.0, -3, 0.75, 1.5]
    a, b = (num, den) if op == DIV else (den, num)      # row 0 is A (the top), row 1 is B
    prog = [word(LOAD, CONST, 0)] + ([word(LOAD, CONST, 1), word(op, STACK)] if stack else [word(op, CONST, 1)])
    value, got = pm.read_out("sens", dtype, ONE, prog, np.stack([a, b]), param_slot={0: 1, 1: 2})
    _exact(value, (num.astype(T) / den.astype(T)))
    H = pm.HP.num
    d_num = [1 / H(float(q)) for q in den]
    d_den = [-H(float(p)) / (H(float(q)) * H(float(q))) for p, q in zip(num, den)]
    if T is np.float32:
        d_num, d_den = [float(v) for v in d_num], [float(v) for v in d_den]
    for plane, ref in ((1, d_num if op == DIV else d_den), (2, d_den if op == DIV else d_num)):
        ulps, right = pm.compare(got[plane], ref, dtype)
        print(f"{pm.NAMES[op]} plane {plane}: max {np.nanmax(ulps):.3f} ulp")
        assert right.all() and np.nanmax(ulps) <= 3.0


# ---- b. arithmetic opcodes -----------------------------------------------------------------------------------------------------
def _program(op):
    return [word(LOAD, CONST, 0)] + ([word(op, CONST, 1)] if op in pm.BINARY else [word(op)])


_results = {}


def _result(op, dtype, target):
    """The kernel's values (and, on the sensitivity kernel, slopes) of one opcode on its point set: run once, shared."""
    key = (op, dtype, target)
    if key not in _results:
        if op in pm.FUNCTIONS:
            pts, extra = pm.function_points(op, dtype)
            pts = np.stack([np.concatenate([pts, [30.0, -30.0] + sorted(extra)]), np.ones(pts.size + 2 + len(extra))])
        else:
            pts = np.stack(pm.arithmetic_points(dtype))
        _results[key] = (pts, pm.read_out(target[0], dtype, target[1], _program(op), pts, param_slot={0: 1, 1: 2}))
    return _results[key]


@both
@pytest.mark.parametrize("op", pm.ARITHMETIC, ids=lambda op: pm.NAMES[op])
def test_arithmetic_opcodes_bit_for_bit(dtype, op):
    """float32: the float64 reference rounded after each instruction (tests/test_prog_machine_reference.py: that is IEEE float32
    arithmetic); float64: IEEE float64. On all three kernels; the edges give inf and NaN, read through the f slot."""
    pts, one = _result(op, dtype, TARGETS[0])
    after = pm.round_to_float32 if dtype == torch.float32 else None
    zeros = torch.zeros(pts.shape[1], dtype=torch.float64)
    want = pm.run_reference(_program(op), torch.from_numpy(pts), zeros, 0.0, after=after).numpy()
    assert op not in (SQRT, DIV, RDIV, RECIP, SQUARE, CUBE) or not np.isfinite(want.astype(pm.np_dtype(dtype))).all()
    _exact(one, want)
    _exact(_result(op, dtype, TARGETS[1])[1], want)
    _exact(_result(op, dtype, TARGETS[2])[1][0], want)


@both
@pytest.mark.parametrize("op", [NEG, ABS, RELU, SQUARE, CUBE, RECIP, SQRT], ids=lambda op: pm.NAMES[op])
def test_arithmetic_slopes(dtype, op):
    """NEG, ABS, RELU, SQUARE: exact, with abs'(0) = relu'(0) = 0. CUBE (3 (v v)), RECIP (-(r r)), SQRT (0.5 / r): two roundings,
    2 ulp."""
    pts, (_, planes) = _result(op, dtype, TARGETS[2])
    if dtype == torch.float32:
        ref = pm.reference_slopes(_program(op), pts, np.zeros(pts.shape[1]), 0.0, rows=(0,))[2][0].numpy()
    else:
        safe = pts.copy()                            # (where mpmath would divide by zero or leave the reals: stated by hand)
        if op in (SQRT, RECIP):
            safe[0, (pts[0] <= 0) if op == SQRT else (pts[0] == 0)] = 1.0
        ref = [d[0] for d in pm.mp_values(_program(op), safe, seeds=(0,))[1]]
        if op == SQRT:
            ref = [r if pts[0, i] > 0 else (float("inf") if pts[0, i] == 0 else float("nan")) for i, r in enumerate(ref)]
        if op == RECIP:
            ref = [r if pts[0, i] != 0 else -float("inf") for i, r in enumerate(ref)]
    ulps, right = pm.compare(planes[1], ref, dtype)
    assert (pts[0] == 0).any() and right.all(), np.flatnonzero(~right)[:5]
    print(f"{pm.NAMES[op]} slope: max {np.nanmax(ulps):.3f} ulp")
    assert np.nanmax(ulps) <= (2.0 if op in (CUBE, RECIP, SQRT) else 0.0)


# ---- c. function opcodes -------------------------------------------------------------------------------------------------------
_TORCH = {EXP: torch.exp, LOG: torch.log, SIN: torch.sin, COS: torch.cos, TANH: torch.tanh, SIGMOID: torch.sigmoid,
          SOFTPLUS: F.softplus}
_measured = {}


def _measure(op, dtype):
    """Per group (sign, binade): the largest ulp error of torch's operator on the device and of the three kernels, for the
    value and for the slope (where the slope is at least 2^-20), both against the reference -- float64 for float32 results, the
    high-precision machine for float64 ones. Nothing is taken from the kernels' own output."""
    key = (op, dtype)
    if key in _measured:
        return _measured[key]
    prog = _program(op)
    n = pm.function_points(op, dtype)[0].size
    pts, (sens_values, planes) = _result(op, dtype, TARGETS[2])
    x = pts[0, :n]
    if dtype == torch.float32:
        value, _, slopes = pm.reference_slopes(prog, pts[:, :n], np.zeros(n), 0.0, rows=(0,))
        ref_value, ref_slope = value.numpy(), slopes[0].numpy()
    else:
        ref_value, tangents = pm.mp_values(prog, pts[:, :n], seeds=(0,))
        ref_slope = [d[0] for d in tangents]
    xt = torch.from_numpy(x).to(dtype).to(pm.DEV).requires_grad_(True)
    yt = _TORCH[op](xt)
    gt, = torch.autograd.grad(yt.sum(), xt)
    got = {"torch": (yt.detach().cpu().numpy(), gt.cpu().numpy()), "sens": (sens_values[:n], planes[1, :n]),
           "one": (_result(op, dtype, TARGETS[0])[1][:n], None), "vec": (_result(op, dtype, TARGETS[1])[1][:n], None)}
    errors = {}
    for name, (v, s) in got.items():
        errors[name, "value"] = pm.compare(v, ref_value, dtype)
        if s is not None:
            errors[name, "slope"] = pm.compare(s, ref_slope, dtype)
    steep = np.array([abs(float(r)) >= 2.0 ** -20 for r in ref_slope])
    table = []
    for group, idx in sorted(pm.groups(x).items()):
        idx = np.array(idx)
        assert idx.size >= pm.PER_GROUP
        for what, names in (("value", ("one", "vec", "sens")), ("slope", ("sens",))):
            use = idx if what == "value" else idx[steep[idx]]
            if use.size == 0:
                continue
            e_torch = np.nanmax(np.append(errors["torch", what][0][use], 0.0))
            for name in names:
                ulps, right = errors[name, what]
                table.append(dict(op=pm.NAMES[op], dtype=str(dtype).split(".")[1], group=group, what=what, kernel=name, points=use.size,
                                  e_torch=float(e_torch), e_kernel=float(np.nanmax(np.append(ulps[use], 0.0))),
                                  bound=float(max(1.0, 2.0 * e_torch)), classes=bool(right[use].all() and errors["torch", what][1][use].all())))
    _measured[key] = table
    return table


@both
@pytest.mark.parametrize("op", pm.FUNCTIONS, ids=lambda op: pm.NAMES[op])
def test_function_opcodes_are_as_accurate_as_torchs_operator(dtype, op):
    """In every group the kernel's largest ulp error is at most max(1, 2 E_torch): 1, because a faithfully rounded function is off by
    one ulp where torch's happens to be exact; twice, because the kernel calls the device math library itself and need not round
    like torch's build of it. A wrong formula, threshold or operand is off by thousands of ulps at these points."""
    table = _measure(op, dtype)
    worst = {}
    for row in table:
        k = (row["what"], row["kernel"])
        if k not in worst or row["e_kernel"] / row["bound"] > worst[k]["e_kernel"] / worst[k]["bound"]:
            worst[k] = row
    for k, row in sorted(worst.items()):
        print(f"{row['op']} {row['dtype']} {k[0]:5s} {k[1]:4s}: worst group {row['group']}: kernel {row['e_kernel']:.3f} ulp, torch "
              f"{row['e_torch']:.3f} ulp, bound {row['bound']:.3f}")
    bad = [row for row in table if not row["classes"] or not row["e_kernel"] <= row["bound"]]
    assert not bad, bad[:6]


@both
@pytest.mark.parametrize("op", pm.FUNCTIONS, ids=lambda op: pm.NAMES[op])
def test_function_opcodes_at_the_ends_of_their_domains(dtype, op):
    """The inputs judged by class: overflow of exp, log of 0 and of a negative, large arguments of sin and cos; the slopes of tanh
    and sigmoid at |v| = 30 are finite and in [0, 1], and softplus has slope 1 above 20. VEC returns the bits of ONE."""
    n = pm.function_points(op, dtype)[0].size
    pts, (values, planes) = _result(op, dtype, TARGETS[2])
    one, vec = _result(op, dtype, TARGETS[0])[1], _result(op, dtype, TARGETS[1])[1]
    _exact(vec, one.astype(np.float64)), _exact(values, one.astype(np.float64))
    extra = pm.function_points(op, dtype)[1]
    for i in range(n, pts.shape[1]):
        x, slope = pts[0, i], float(planes[1, i])
        if abs(x) == 30.0:
            if op in (TANH, SIGMOID):
                assert 0.0 <= slope <= 1.0, (x, slope)
            if op == SOFTPLUS and x > 0:
                assert slope == 1.0 and one[i] == 30.0
            continue
        want = extra[x]
        if want == "unit":
            assert np.isfinite(one[i]) and abs(one[i]) <= 1.0 and abs(slope) <= 1.0
            close = 1e-6 if dtype == torch.float32 else 1e-11
            assert abs(float(one[i]) - float(_TORCH[op](torch.tensor(x, dtype=torch.float64)))) < close
        elif np.isnan(want):
            assert np.isnan(one[i])
        else:
            assert one[i] == want, (x, one[i])
    if op == SOFTPLUS:
        above = pts[0, :n] > 20
        assert above.sum() > 90 and np.array_equal(one[:n][above], pts[0, :n][above].astype(one.dtype))
        assert (planes[1, :n][above] == 1).all()


@both
@pytest.mark.parametrize("shape", [ONE, VEC], ids=["one", "vec"])
def test_the_additive_noise_kernel_runs_the_same_machine(dtype, shape):
    """`tsde_trajectory_prog_additive` (m = 1, a zero table, the f slot): every opcode on its point set, the bits of the diagonal
    kernel."""
    for op in pm.ARITHMETIC + pm.FUNCTIONS:
        pts, want = _result(op, dtype, TARGETS[0])
        _exact(pm.read_out("additive", dtype, shape, _program(op), pts), want.astype(np.float64))
    pts = np.stack([_X, _Y, _POW2, np.roll(_X, 3)])
    prog = [word(LOAD, CONST, 0), word(LOAD, CONST, 1), word(LOAD, CONST, 2), word(DUP), word(MUL, STACK), word(RSUB, STACK),
            word(MUL, STACK), word(ADD, TIME), word(SUB, STATE)]
    _exact(pm.read_out("additive", dtype, shape, prog, pts, t0=0.75, state=pts[3]),
           pts[3] + (pts[0] * (pts[2] * pts[2] - pts[1]) + 0.75 - pts[3]))


def accuracy_table():
    """The text of profiles/prog_machine_accuracy.txt: every row of `_measure` for every function opcode and dtype."""
    lines = [f"# reference of the float64 kernels: {pm.HP.name}; device: {torch.cuda.get_device_properties(0).gcnArchName}",
             "# E_torch: torch's operator of the same name (slope: its autograd) on the device; bound = max(1, 2 E_torch)",
             "# op dtype what kernel sign binade points E_torch[ulp] E_kernel[ulp] bound[ulp]"]
    for dtype in DTYPES:
        for op in pm.FUNCTIONS:
            for r in _measure(op, dtype):
                lines.append(f"{r['op']:8s} {r['dtype']} {r['what']} {r['kernel']:4s} {r['group'][0]:+d} {r['group'][1]:5d} {r['points']:3d} "
                             f"{r['e_torch']:10.3f} {r['e_kernel']:10.3f} {r['bound']:10.3f}")
    return "\n".join(lines) + "\n"


# ---- d. generated units --------------------------------------------------------------------------------------------------------
# Two triples (f, g, g') whose words hold every opcode with every source it can take, constant rows on both sides of 8, and DUP.
# The state lives in about [1, 3] (y0 = 2, drifts that revert to row 10 ~ 2, diffusions of about 0.3) and the time in [1, 1.19],
# so every divisor, logarithm and square root is taken well inside its domain. g' is the derivative of g (the oracle's Milstein
# differentiates g by autograd): rows 4 and 11 are the numbers 1 and 1/2 of those derivatives.
_C = lambda k: word(LOAD, CONST, k)          # noqa: E731
F_A = [word(LOAD, STATE), word(ADD, TIME), word(SUB, CONST, 2), word(LOAD, TIME), word(MUL, STATE), word(ADD, STACK),     # u = y + t - c2 + t y
       word(DIV, STATE), word(RSUB, TIME), _C(8), word(RDIV, STATE), word(SUB, STACK), word(MUL, TIME),             # (t - u/y - y/c8) t  < -1
       word(RDIV, CONST, 3), word(SIN), word(DUP), word(COS), word(DIV, STACK),                                     # s / cos s, s = sin(c3 / .)
       word(LOAD, STATE), word(LOG), word(RSUB, STACK), word(EXP), word(RDIV, TIME), word(SUB, STATE), word(SUB, TIME), word(TANH),
       word(MUL, CONST, 0), word(ADD, CONST, 10), word(SUB, STATE)]
G_A = [word(LOAD, STATE), word(SIGMOID), word(MUL, CONST, 1), word(ADD, CONST, 9)]                                  # c1 sigmoid(y) + c9
DG_A = [word(LOAD, STATE), word(SIGMOID), word(DUP), word(RSUB, CONST, 4), word(MUL, STACK), word(MUL, CONST, 1)]   # c1 s (1 - s)
F_B = [word(LOAD, STATE), word(SUB, CONST, 10), word(RELU), word(ADD, CONST, 11),                                   # D = relu(y - c10) + 1/2
       word(LOAD, STATE), word(MUL, CONST, 12), word(DUP), word(SOFTPLUS), word(RSUB, STACK),                       # r = softplus(x) - x, x = c12 y
       word(RSUB, STATE), word(DUP), word(ABS), word(ADD, STACK), word(RDIV, STACK), word(NEG), word(DIV, CONST, 8),  # -(q + |q|) / D / c8
       word(TANH), word(CUBE), word(ADD, CONST, 8), word(RECIP), word(MUL, CONST, 0), word(ADD, CONST, 10), word(SUB, STATE)]
G_B = [word(LOAD, STATE), word(SQRT), word(MUL, CONST, 1), word(LOAD, STATE), word(SQUARE), word(MUL, CONST, 9), word(DIV, TIME),
       word(ADD, STACK)]                                                                                            # c1 sqrt(y) + c9 y^2 / t
DG_B = [word(LOAD, STATE), word(SQRT), word(RDIV, CONST, 11), word(MUL, CONST, 1), word(LOAD, STATE), word(ADD, STATE),
        word(MUL, CONST, 9), word(DIV, TIME), word(ADD, STACK)]                                                     # c1 / (2 sqrt(y)) + 2 y c9 / t
TRIPLES = {"A": (F_A, G_A, DG_A), "B": (F_B, G_B, DG_B)}
PARAM_ROWS = {0: 1, 1: 2, 9: 3, 12: 4}
STEPS, DT, T_START, ENTROPY = 24, 2.0 ** -7, 1.0, 77
OUT_STEP, OUT_W = [10, 24], [(0.5, 0.5), (0.0, 1.0)]


def _unit_consts(d):
    c = np.arange(d)
    table = np.zeros((13, d))
    table[0] = 0.3 + (c * 7 % 16) / 40.0
    table[1] = 0.1 + (c * 5 % 8) / 80.0
    table[2] = 0.4 + (c * 3 % 8) / 32.0
    table[3] = 0.75 + (c * 11 % 16) / 32.0
    table[4] = 1.0
    table[5], table[6], table[7] = 3.0, -7.0, 11.0        # (never read)
    table[8] = 2.0 + (c % 4) / 8.0
    table[9] = 0.02 + (c * 13 % 16) / 512.0
    table[10] = 1.875 + (c * 9 % 16) / 64.0
    table[11] = 0.5
    table[12] = -3.0 + (c * 29 % 64) * (17.0 / 64)       # x = c12 y crosses the softplus threshold: many channels in (20, 30]
    return table


def test_the_two_triples_hold_every_opcode_with_every_source():
    seen = {pm.fields(w)[:2] for triple in TRIPLES.values() for prog in triple for w in prog}
    wanted = {(op, src) for op in pm.BINARY for src in (STACK, CONST, STATE, TIME)} | {(LOAD, src) for src in (CONST, STATE, TIME)} | \
        {(op, 0) for op in pm.UNARY + (DUP,)}
    assert seen == wanted, wanted ^ seen
    rows = {pm.fields(w)[2] for triple in TRIPLES.values() for prog in triple for w in prog if pm.fields(w)[1] == CONST}
    assert min(rows) < pm.REG_ROWS <= max(rows) and all(len(p) <= 32 for t in TRIPLES.values() for p in t)
    # g' is the derivative of g
    y = torch.linspace(1.0, 3.0, 67, dtype=torch.float64)
    for _, g, dg in TRIPLES.values():
        _, slope, _ = pm.reference_slopes(g, _unit_consts(67), y, 1.1)
        torch.testing.assert_close(pm.run_reference(dg, torch.from_numpy(_unit_consts(67)), y, 1.1), slope, rtol=1e-13, atol=0)


UNITS = [(name, kind, dtype) for name in TRIPLES for kind in ("values", "sens") for dtype in DTYPES] + \
    [("A", "additive4", torch.float32)]


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    """The nine units, compiled once, eight compilers at a time, into a cache of this session."""
    from torchsde_amd import specialise
    patch = pytest.MonkeyPatch()
    patch.setattr(specialise, "MODE", "sync")
    patch.setenv("TSDE_SPECIALISE_CACHE", str(tmp_path_factory.getbasetemp() / "specialised"))

    def make(unit):
        name, kind, dtype = unit
        f, g, dg = TRIPLES[name]
        if kind == "additive4":
            return pm.unit_for(kind, dtype, f, (), (), 13, pm.EULER)
        return pm.unit_for(kind, dtype, f, g, dg, 13, pm.MILSTEIN_ITO)
    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            yield dict(zip(UNITS, pool.map(make, UNITS)))
    finally:
        patch.undo()


def _solve_triple(name, kind, dtype, shape, scalar_noise, unit=None):
    f, g, dg = TRIPLES[name]
    return pm.solve(kind, dtype, shape, f, g, dg, _unit_consts(shape[1]), method=pm.MILSTEIN_ITO, y0=np.full(shape, 2.0),
                    step_rows=pm.noise_rows(STEPS, DT, T_START), out_step=OUT_STEP, out_w=OUT_W, scalar_noise=scalar_noise,
                    param_slot=PARAM_ROWS, entropy=ENTROPY, unit=unit)


@both
@pytest.mark.parametrize("scalar_noise", [0, 1], ids=["diagonal", "scalar"])
@pytest.mark.parametrize("target", TARGETS, ids=TARGET_IDS)
@pytest.mark.parametrize("name", sorted(TRIPLES))
def test_generated_units_equal_the_interpreter_bit_for_bit(units, name, target, scalar_noise, dtype):
    """One 24-step Milstein solve with real noise, dt = 2^-7: values, and on the sensitivity kernel every tangent plane with four
    parameter rows. Both lane widths of the same library are run."""
    kind, shape = target
    slow = _solve_triple(name, kind, dtype, shape, scalar_noise)
    fast = _solve_triple(name, kind, dtype, shape, scalar_noise, unit=units[name, kind, dtype])
    assert bool(torch.isfinite(slow[0]).all()) and (kind != "sens" or bool(torch.isfinite(slow[1]).all()))
    assert float(slow[0].min()) > 0.5 and not torch.equal(slow[0][0], slow[0][1])
    assert pm.same_bits(fast[0], slow[0])
    if kind == "sens":
        assert pm.same_bits(fast[1], slow[1])
        assert all(bool((slow[1][:, s] != 0).any()) for s in range(pm.SENS if name == "B" else pm.SENS - 1))   # (A has no row 12)


@pytest.mark.parametrize("shape", [ONE, VEC], ids=["one", "vec"])
def test_generated_additive_unit_equals_the_interpreter(units, shape):
    """The first drift as an `additive4` unit (Euler, float32), m = 3 channels with a constant (m, d) table."""
    d = shape[1]
    gtab = torch.from_numpy(np.array([[((j * 5 + c) % 16) / 64.0 for c in range(d)] for j in range(3)])).float().to(pm.DEV)
    kw = dict(method=pm.EULER, y0=np.full(shape, 2.0), step_rows=pm.noise_rows(STEPS, DT, T_START), out_step=OUT_STEP, out_w=OUT_W,
              entropy=ENTROPY, m=3, g_table=gtab)
    slow = pm.solve("additive", torch.float32, shape, F_A, [], [], _unit_consts(d), **kw)[0]
    unit = units["A", "additive4", torch.float32]
    fast = pm.solve("additive", torch.float32, shape, F_A, [], [], _unit_consts(d), unit=unit, **kw)[0]
    assert bool(torch.isfinite(slow).all()) and pm.same_bits(fast, slow) and not torch.equal(slow[0], slow[1])


class _MachineSDE:
    """The reference machine as the module the oracle's solvers take."""
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, f, g, consts):
        self.f_words, self.g_words, self.consts = f, g, torch.from_numpy(consts)

    def f(self, t, y):
        return pm.run_reference(self.f_words, self.consts, y, t)

    def g(self, t, y):
        return pm.run_reference(self.g_words, self.consts, y, t)


@pytest.mark.parametrize("scalar_noise", [0, 1], ids=["diagonal", "scalar"])
@pytest.mark.parametrize("target", TARGETS[:2], ids=TARGET_IDS[:2])
@pytest.mark.parametrize("name", sorted(TRIPLES))
def test_the_interpreter_follows_the_reference_machine_through_the_oracle(name, target, scalar_noise):
    """float64: the same solve by the oracle's Milstein loop (which differentiates g by autograd) on the reference machine, fed the
    increments of the oracle's twin of the generator. VEC: its first two and its last batch row."""
    from oracle import counter, solvers_ref
    kind, shape = target
    rows, d = shape
    got = _solve_triple(name, kind, torch.float64, shape, scalar_noise)[0].cpu()
    f, g, _ = TRIPLES[name]
    edges = T_START + np.arange(STEPS + 1) * DT
    ts = torch.tensor([T_START, T_START + 9.5 * DT, T_START + STEPS * DT], dtype=torch.float64)
    for lo, hi in ([(0, rows)] if shape == ONE else [(0, 2), (rows - 1, rows)]):
        width = 1 if scalar_noise else d

        def bm(ta, tb, return_U=False):
            w, _, _ = counter.query((hi - lo) * width, ENTROPY, edges, float(ta), float(tb), dtype=np.float64, elem0=lo * width)
            return torch.from_numpy(w).reshape(hi - lo, width)
        with torch.no_grad():
            y0 = torch.full((hi - lo, d), 2.0, dtype=torch.float64)
            want = solvers_ref.integrate(_MachineSDE(f, g, _unit_consts(d)), bm, y0, ts, DT, "milstein")
        torch.testing.assert_close(got[:, lo:hi], want[1:], rtol=1e-11, atol=0)
