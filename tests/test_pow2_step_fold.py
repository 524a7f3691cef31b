"""The folded step of the affine trajectory kernel (csrc/trajectory.hip, form POW2) on the CPU: no GPU involved.

When a step's dt and sqrt(h) are powers of two the kernel computes, per element and with z the unscaled standard normal,

    Euler     fma(g*z, sw, fma(f, dt, y))                                  in place of  (y + f*dt) + 1*(g*(z*sw))
    midpoint  the same twice, the predictor with dt/2 and sw/2             in place of  (y + f*dt/2) + 0.5*(g*(z*sw)), ...

and claims the same float32, bit for bit, as long as no product (f*dt, z*sw, g*z*sw, and their halves) is subnormal. Checked
here in exact arithmetic (rationals, every operation rounded to float32 by `rn32`) and in bulk with numpy, where a fused
multiply-add is emulated through float64: the product of two float32 is exact in float64, and adding a float32 to a
float32-representable product in float64 and rounding the sum again to float32 rounds like one float32 addition (53 >= 2*24 + 2
bits). So the emulation is exact wherever the product with the power of two is itself a float32, i.e. inside the domain.

Also: the host's decision (`kernels.pow2_steps`, the `flags` of `TrajectorySchedule`).
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from torchsde_amd import _native
from torchsde_amd import kernels as K

F32 = np.float32
# (dt, sqrt(h)): the step pairs of the change's own check plus dt = 2^-4
STEP_PAIRS = [(2.0 ** -10, 2.0 ** -5), (2.0 ** -6, 2.0 ** -3), (2.0 ** -20, 2.0 ** -10), (2.0 ** -4, 2.0 ** -2)]
SMALLEST_NORMAL = 2.0 ** -126


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------
def rn32(x):
    """The rational `x` rounded to the nearest float32 (ties to even, gradual underflow), as a Fraction."""
    x = Fraction(x)
    if x == 0:
        return x
    mag = abs(x)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    e = max(e, -126)                                   # below 2^-126 the spacing stays 2^-149
    unit = Fraction(2) ** (e - 23)
    n = round(mag / unit)                              # Fraction.__round__: ties to even
    return (n * unit) if x > 0 else -(n * unit)


def _frac(v):
    return Fraction(float(v))


def exact_plain(method, y, a, b, c, e, z, dt, sw):
    """The plain form's operations (tsde_schemes.h drift_diffusion_update), one rounding each."""
    mul = lambda p, q: rn32(p * q)
    add = lambda p, q: rn32(p + q)
    f = lambda x: add(mul(a, x), b) if b is not None else mul(a, x)
    g = lambda x: add(mul(c, x), e) if e is not None else mul(c, x)
    w = mul(z, sw)
    upd = lambda x, cf, cg: add(add(y, mul(f(x), cf)), mul(cg, mul(g(x), w)))
    if method == "euler":
        return upd(y, dt, Fraction(1))
    yp = upd(y, mul(Fraction(1, 2), dt), Fraction(1, 2))
    return upd(yp, dt, Fraction(1))


def exact_folded(method, y, a, b, c, e, z, dt, sw):
    """The folded form's operations (drift_diffusion_update_pow2): a product and two fused multiply-adds per update."""
    mul = lambda p, q: rn32(p * q)
    add = lambda p, q: rn32(p + q)
    fma = lambda p, q, r: rn32(p * q + r)
    f = lambda x: add(mul(a, x), b) if b is not None else mul(a, x)
    g = lambda x: add(mul(c, x), e) if e is not None else mul(c, x)
    upd = lambda x, cf, sz: fma(mul(g(x), z), sz, fma(f(x), cf, y))
    if method == "euler":
        return upd(y, dt, sw)
    yp = upd(y, dt / 2, sw / 2)
    return upd(yp, dt, sw)


def _signed_log_uniform(rng, n, lo, hi):
    return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(lo, hi, n)).astype(F32)


def _tuples(rng, n, shifts):
    """(y, a, b, c, e, z): signed states from 2^-60 to 2^60, rates of order one, normals with a few tiny ones and zeros."""
    y = _signed_log_uniform(rng, n, -60, 60)
    a = _signed_log_uniform(rng, n, -2, 1)
    c = _signed_log_uniform(rng, n, -2, 1)
    z = rng.standard_normal(n).astype(F32)
    z[::17] = _signed_log_uniform(rng, len(z[::17]), -46, -20)      # the generator's small nonzero normals
    z[::101] = 0.0
    if shifts:
        b, e = (y * rng.standard_normal(n)).astype(F32), (y * rng.standard_normal(n)).astype(F32)
    else:
        b = e = None
    return y, a, b, c, e, z


@pytest.mark.parametrize("shifts", [False, True], ids=["linear", "shifts"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
@pytest.mark.parametrize("dt,sw", STEP_PAIRS)
def test_fold_is_exact_in_rational_arithmetic(method, dt, sw, shifts):
    rng = np.random.default_rng(1234)
    y, a, b, c, e, z = _tuples(rng, 400, shifts)
    for i in range(len(y)):
        args = (_frac(y[i]), _frac(a[i]), None if b is None else _frac(b[i]), _frac(c[i]),
                None if e is None else _frac(e[i]), _frac(z[i]), Fraction(dt), Fraction(sw))
        assert exact_folded(method, *args) == exact_plain(method, *args), (method, dt, i)


# ---- the same in bulk (numpy float32; fused multiply-add through float64) ---------------------------------------------------
def _fma(p, q, r):
    return (p.astype(np.float64) * np.float64(q) + r.astype(np.float64)).astype(F32)


def bulk_plain(method, y, a, b, c, e, z, dt, sw):
    dt, sw = F32(dt), F32(sw)
    f = lambda x: a * x + b if b is not None else a * x
    g = lambda x: c * x + e if e is not None else c * x
    w = z * sw
    upd = lambda x, cf, cg: (y + f(x) * cf) + cg * (g(x) * w)
    if method == "euler":
        return upd(y, dt, F32(1))
    return upd(upd(y, F32(0.5) * dt, F32(0.5)), dt, F32(1))


def bulk_folded(method, y, a, b, c, e, z, dt, sw):
    dt, sw = F32(dt), F32(sw)
    f = lambda x: a * x + b if b is not None else a * x
    g = lambda x: c * x + e if e is not None else c * x
    upd = lambda x, cf, sz: _fma(g(x) * z, sz, _fma(f(x), cf, y))
    if method == "euler":
        return upd(y, dt, sw)
    return upd(upd(y, dt * F32(0.5), sw * F32(0.5)), dt, sw)


def _in_domain(method, y, a, b, c, e, z, dt, sw):
    """No product of the step subnormal: every |f*cf| and |g*z*sz| is zero or at least 2^-126 (checked in float64)."""
    f = lambda x: (a * x + b if b is not None else a * x).astype(np.float64)
    g = lambda x: (c * x + e if e is not None else c * x).astype(np.float64)
    ok_value = lambda v: (v == 0) | (np.abs(v) >= SMALLEST_NORMAL)
    stages = [(y, 1.0)] if method == "euler" else [(y, 0.5), (bulk_plain("euler", y, a, b, c, e, z, dt / 2, sw / 2), 1.0)]
    # (the midpoint predictor is an Euler step with dt/2 and, because 0.5*(g*(z*sw)) = g*(z*(sw/2)) in the domain, sw/2)
    ok = ok_value(z.astype(np.float64) * sw * (0.5 if method == "midpoint" else 1.0))
    for x, scale in stages:
        ok &= ok_value(f(x) * dt * scale) & ok_value(g(x) * z.astype(np.float64) * sw * scale)
    return ok


@pytest.mark.parametrize("shifts", [False, True], ids=["linear", "shifts"])
@pytest.mark.parametrize("method", ["euler", "midpoint"])
@pytest.mark.parametrize("dt,sw", STEP_PAIRS)
def test_fold_is_exact_in_bulk(method, dt, sw, shifts):
    rng = np.random.default_rng(99)
    with np.errstate(under="ignore"):
        t = _tuples(rng, 1_000_000, shifts)
        keep = _in_domain(method, *t, dt, sw)
        assert keep.mean() > 0.99                       # the sample lies inside the domain but for stray cancellations
        plain, folded = bulk_plain(method, *t, dt, sw), bulk_folded(method, *t, dt, sw)
    assert np.array_equal(plain[keep].view(np.uint32), folded[keep].view(np.uint32))


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_fold_differs_when_the_step_is_no_power_of_two(method):
    """dt = 1e-3: scaling is no longer exact and the folded form rounds differently -- the reason the host gates it."""
    rng = np.random.default_rng(5)
    y, a, _, c, _, z = _tuples(rng, 3000, False)
    dt = _frac(F32(1e-3))
    sw = _frac(np.sqrt(F32(1e-3)))
    differing = 0
    for i in range(len(y)):
        args = (_frac(y[i]), _frac(a[i]), None, _frac(c[i]), None, _frac(z[i]), dt, sw)
        differing += exact_folded(method, *args) != exact_plain(method, *args)
    assert differing > 0


@pytest.mark.parametrize("method,ulps", [("euler", 2), ("midpoint", 8)])
@pytest.mark.parametrize("exponent", [-140, -131, -122, -113])
def test_below_the_domain_the_forms_differ_by_a_few_ulps_at_most(method, ulps, exponent):
    """|c*y| z sw below 2^-126: the plain form rounds the subnormal products f*dt and g*w (an error of at most 2^-150 each)
    and the folded form does not. Euler: the two sums that follow see operands that differ by at most that, so each can
    land on the neighbouring float: at most 2 units in the last place of the state (2^-149 while the state is subnormal).
    Midpoint: the predictor differs by those 2 units; with |a|, |c|, |w| <= 1 the corrector's f and g carry them on scaled by
    at most 1 and round once more (2 + 1 units into the noise term, less into the drift term), and its own two sums add 2: 8
    units bounds it. The test holds |a|, |c| <= 1 and |z| sw <= 1."""
    rng = np.random.default_rng(exponent & 0xFFFF)
    dt, sw = Fraction(2) ** -10, Fraction(2) ** -5
    worst = 0
    for _ in range(300):
        y = float(F32(rng.choice([-1.0, 1.0]) * 2.0 ** (exponent + rng.uniform(0, 1))))
        a, c = (float(F32(v)) for v in rng.uniform(-1, 1, 2))
        z = float(F32(np.clip(rng.standard_normal(), -4, 4)))
        args = (_frac(y), _frac(a), None, _frac(c), None, _frac(z), dt, sw)
        plain, folded = exact_plain(method, *args), exact_folded(method, *args)
        ulp = Fraction(float(np.spacing(F32(max(abs(y), abs(float(plain)))))))
        assert abs(folded - plain) <= ulps * ulp
        worst = max(worst, abs(folded - plain) / ulp)
    print(f"{method} at 2^{exponent}: worst difference {float(worst)} ulp")


# ---- the host's decision ----------------------------------------------------------------------------------------------------
def _rows(dt, h, np_dtype):
    dt, h = np.asarray(dt, dtype=np.float64), np.asarray(h, dtype=np.float64)
    rows = np.zeros((len(dt), 8))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = dt, 0.5 * dt, 1.0 / dt, np.sqrt(dt)
    rows[:, 4], rows[:, 5], rows[:, 6] = np.sqrt(h), np.sqrt(h / 12.0), h
    return rows.astype(np_dtype)


def _schedule(rows, dtype, cached=False):
    make = K.TrajectorySchedule.cached if cached else K.TrajectorySchedule
    n = rows.shape[0]
    return make(rows, np.arange(n), [n], [(0.0, 1.0)], torch.device("cpu"), dtype)


BIT_CASES = {
    "2^-10": ([2.0 ** -10] * 5, [2.0 ** -10] * 5, True),
    "2^-4": ([2.0 ** -4] * 3, [2.0 ** -4] * 3, True),
    "mixed dyadic steps": ([2.0 ** -10, 2.0 ** -6, 2.0 ** -4], [2.0 ** -10, 2.0 ** -6, 2.0 ** -4], True),
    "1e-3": ([1e-3] * 5, [1e-3] * 5, False),
    "2^-9: the root is no power of two": ([2.0 ** -9] * 5, [2.0 ** -9] * 5, False),
    "2^-10 with one odd step": ([2.0 ** -10] * 4 + [3 * 2.0 ** -10], [2.0 ** -10] * 4 + [3 * 2.0 ** -10], False),
    "only dt dyadic": ([2.0 ** -10] * 3, [1e-3] * 3, False),
    "only h dyadic": ([1e-3] * 3, [2.0 ** -10] * 3, False),
    "below the exponent range": ([2.0 ** -54] * 3, [2.0 ** -54] * 3, False),
    "above the exponent range": ([2.0 ** 54] * 3, [2.0 ** 54] * 3, False),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", sorted(BIT_CASES))
def test_schedule_bit(case, dtype, monkeypatch):
    monkeypatch.delenv("TSDE_POW2_STEPS", raising=False)
    dt, h, expected = BIT_CASES[case]
    rows = _rows(dt, h, np.float32 if dtype == torch.float32 else np.float64)
    assert K.pow2_steps(rows) is expected
    schedule = _schedule(rows, dtype)
    assert schedule.pow2_steps is expected
    assert schedule._struct.flags == (_native.TRAJ_POW2_STEPS if expected else 0)


def test_exponent_range_edges():
    for e_dt, ok in [(-52, True), (52, True), (-53, False), (53, False)]:
        sw = 2.0 ** (e_dt // 2)                          # keep sqrt(h) inside its own range: only dt decides
        rows = _rows([2.0 ** e_dt], [sw * sw], np.float64)
        rows[:, 4] = 2.0 ** -1
        assert K.pow2_steps(rows) is ok, e_dt
    for e_sw, ok in [(-26, True), (26, True), (-27, False), (27, False)]:
        rows = _rows([2.0 ** -2], [2.0 ** -2], np.float64)
        rows[:, 4] = 2.0 ** e_sw
        assert K.pow2_steps(rows) is ok, e_sw
    rows = _rows([2.0 ** -10], [2.0 ** -10], np.float32)
    rows[:, 1] = np.float32(2.0 ** -10)                  # slot 1 is not dt/2
    assert K.pow2_steps(rows) is False
    assert K.pow2_steps(np.zeros((0, 8), dtype=np.float32)) is False


def test_struct_layout_appends_the_flags():
    assert _native.Traj.n_steps.offset == 32 and _native.Traj.n_out.offset == 36     # where they always were
    assert _native.Traj.flags.offset == 40 and _native.Traj().flags == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_switch_clears_the_bit_and_makes_a_distinct_cached_schedule(dtype, monkeypatch):
    rows = _rows([2.0 ** -10] * 7, [2.0 ** -10] * 7, np.float32 if dtype == torch.float32 else np.float64)
    monkeypatch.delenv("TSDE_POW2_STEPS", raising=False)
    on = _schedule(rows, dtype, cached=True)
    assert on.pow2_steps and _schedule(rows, dtype, cached=True) is on
    monkeypatch.setenv("TSDE_POW2_STEPS", "0")
    off = _schedule(rows, dtype, cached=True)
    assert off is not on and not off.pow2_steps and off._struct.flags == 0
    assert _schedule(rows, dtype, cached=True) is off
    monkeypatch.delenv("TSDE_POW2_STEPS")
    assert _schedule(rows, dtype, cached=True) is on
