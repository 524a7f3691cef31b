"""The small-radius series of the float32 Box-Muller (torchsde_amd/csrc/tsde_rng.h: `box_muller`, the branch taken for
a >= 0xF0000000) carries its factor 2 inside the Horner coefficients. The claim that this changes no bit -- doubling is
exact and commutes with the one rounding of every fused multiply-add -- is checked here in exact rational arithmetic with
correct round-to-nearest-even to float32, on the arguments the branch can see. No GPU involved."""
from fractions import Fraction

import numpy as np


def _round_f32(x: Fraction) -> Fraction:
    """x > 0 rounded to the nearest float32 (ties to even); normal range only."""
    assert x > 0
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1) and -126 <= e < 127
    ulp = Fraction(2) ** (e - 23)
    q = x / ulp
    m = q.numerator // q.denominator
    rest = q - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    return m * ulp


def _f32(x) -> Fraction:
    return Fraction(float(np.float32(x)))


def _fma(a, b, c):
    return _round_f32(a * b + c)


def _series_two_outside(w):       # 2 * w * p, p the Horner form of 1 + w/2 + w^2/3 + w^3/4 + w^4/5 + w^5/6
    p = _fma(w, _f32(1.0 / 6.0), _f32(0.2))
    for c in (_f32(0.25), _f32(1.0 / 3.0), _f32(0.5), _f32(1.0)):
        p = _fma(w, p, c)
    return _round_f32(_round_f32(2 * w) * p), p


def _series_two_folded(w):        # w * p', the coefficients doubled
    p = _fma(w, _f32(1.0 / 3.0), _f32(0.4))
    for c in (_f32(0.5), _f32(2.0 / 3.0), _f32(1.0), _f32(2.0)):
        p = _fma(w, p, c)
    return _round_f32(w * p), p


def test_doubled_coefficients_are_exactly_twice_the_plain_ones():
    for plain, doubled in ((1.0 / 6.0, 1.0 / 3.0), (0.2, 0.4), (0.25, 0.5), (1.0 / 3.0, 2.0 / 3.0), (0.5, 1.0), (1.0, 2.0)):
        assert 2 * _f32(plain) == _f32(doubled)


def test_folded_series_equals_the_series_with_the_factor_outside_bit_for_bit():
    rng = np.random.default_rng(20240601)
    # the branch sees ~a in [0, 2^28): w = fma(float(~a), 2^-32, 2^-33); the ends, powers of two and their neighbours, a sample
    na = {0, 1, 2, 3, (1 << 28) - 1, (1 << 28) - 2}
    for k in range(2, 28):
        na.update({(1 << k) - 1, 1 << k, (1 << k) + 1})
    na.update(int(v) for v in rng.integers(0, 1 << 28, size=1500))
    for v in sorted(na):
        w = _fma(_f32(np.float32(np.uint32(v))), Fraction(1, 1 << 32), Fraction(1, 1 << 33))
        outside, p = _series_two_outside(w)
        folded, p2 = _series_two_folded(w)
        assert p2 == 2 * p and folded == outside, hex(v)
