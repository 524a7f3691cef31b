"""The activation formulas of the matrix-core kernels, emulated on the CPU (tests/neural_activation_forms.py): the float64
reference against mpmath, the bound of tests/test_gpu_neural_activations.py shown to be one a kernel CAN meet, and the forms that
break the "absolute error <= 3e-7" the header of csrc/tsde_mlp.h used to claim."""
import numpy as np
import pytest

from tests import neural_activation_forms as forms

SITE_QUANTITIES = [(s, q) for s in forms.SITES for q in forms.quantities(s)]


def test_the_grid_is_what_the_bound_is_stated_over():
    x = forms.sample_grid()
    assert x.dtype == np.float32 and len(np.unique(x)) == len(x) == 38 * 64 + 7 + 2 * len(forms.EDGES)
    assert np.all(np.isfinite(x)) and np.all((x == 0) | (np.abs(x) >= np.finfo(np.float32).tiny))      # no subnormal inputs
    twenty = np.float32(20.0)
    for v in (0.0, 2.0 ** -100, -2.0 ** -100, twenty, np.nextafter(twenty, np.float32(30)), np.nextafter(twenty, np.float32(0)),
              -twenty, 8.5, -9.1, 16.6, -17.4, 44.0, -88.0, 89.0, -104.0, 127.0, 1e4, -1e4, 3e38, -3e38):
        assert np.float32(v) in x
    exponents = np.floor(np.log2(np.abs(x[:38 * 64].astype(np.float64)))).astype(int)
    for e in range(-30, 8):                                                          # 32 of either sign in every binade
        assert np.sum((exponents == e) & (x[:38 * 64] > 0)) == 32 and np.sum((exponents == e) & (x[:38 * 64] < 0)) == 32


def test_the_float64_reference_agrees_with_mpmath_at_50_digits():
    import mpmath
    x = forms.sample_grid()
    ref, exact = forms.reference(x), forms.reference_mp(x, digits=50)
    for q in forms.QUANTITIES:
        assert np.all(np.isfinite(ref[q])), q
        worst = max(float(abs(mpmath.mpf(float(r)) - m) / max(1, abs(m))) for r, m in zip(ref[q], exact[q]))
        assert worst <= 1e-15, (q, worst)


@pytest.mark.parametrize("site,quantity", SITE_QUANTITIES)
def test_no_form_returns_a_nan_or_an_infinity(site, quantity):
    x = forms.sample_grid()
    assert np.all(np.isfinite(forms.reference(x)[quantity]))
    for seed in (None, 1, 2, 3):
        got = forms.emulate(site, x, seed)[quantity]
        assert got.dtype == np.float32 and np.all(np.isfinite(got)), (site, quantity, seed, x[~np.isfinite(got)])


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("site,quantity", SITE_QUANTITIES)
def test_primitives_one_ulp_off_stay_inside_the_bound(site, quantity, seed):
    """The bound 2 * E_form + 2^-24 can be met: every exp2, reciprocal and log2 result moved by a random -1, 0 or +1 ulp."""
    x = forms.sample_grid()
    err = forms.measure(forms.emulate(site, x, seed)[quantity], forms.reference(x)[quantity])
    assert forms.E_form(site, quantity) > 0.0
    assert err.max() <= forms.bound(site, quantity), (site, quantity, float(err.max()), forms.bound(site, quantity),
                                                      float(x[err.argmax()]))


def test_the_lipswish_slope_rests_on_an_exact_reciprocal_of_one():
    """c * s * (1 + x * (1 - s)) with s = rcp(1 + exp2(-x log2 e)): from x = 17.4 on, 1 + exp2(.) IS 1 and the form is right only
    because rcp(1) is exactly 1 -- a reciprocal one ulp off THERE puts x * 2^-24 into the slope (6e-4 at x = 1e4). Every other
    form stays inside its bound even then. The perturbation above therefore leaves exactly representable results alone, and
    tests/test_gpu_neural_activations.py holds the hardware to the bound at those points."""
    x = forms.sample_grid()
    ref = forms.reference(x)
    over = set()
    for seed in (1, 2, 3):
        for site in forms.SITES:
            for q, v in forms.emulate(site, x, seed, move_exact=True).items():
                bad = forms.measure(v, ref[q]) > forms.bound(site, q)
                if bad.any():
                    over.add((site, q))
                    assert np.all(x[bad] > 17.4)
    assert over == {("hidden_act", "lipswish.slope")}


def test_forms_that_break_the_three_e_minus_seven_of_the_old_header_comment():
    """"Absolute error <= 3e-7" (csrc/tsde_mlp.h, before): with IDEAL primitives already, the tanh slope 1 - v^2 is off by 3.4e-7
    and the LipSwish slope by 8.6e-7 (absolute below 1, relative above); softplus and LipSwish values are within 1.5e-7 of the
    VALUE but 1.6e-6 / 1.2e-6 off absolutely (near x = 11 .. 16, where an ulp of the value is 1e-6)."""
    listed = forms.over_the_header_claim()
    print()
    for site, q, e_form, e_abs in listed:
        print(f"  {site:22s}{q:18s} E_form {e_form:.3e}   worst absolute error over |x| <= 20 {e_abs:.3e}")
    by_measure = {(s, q) for s, q, e_form, _ in listed if e_form > forms.HEADER_CLAIM}
    by_absolute = {(s, q) for s, q, _, e_abs in listed if e_abs > forms.HEADER_CLAIM}
    tanh_slopes = {(s, "tanh.slope") for s in ("activate_with_slope", "milstein_hidden", "hidden_act", "final_act",
                                              "final_slope")}
    assert by_measure == tanh_slopes | {("hidden_act", "lipswish.slope")}
    assert by_absolute - by_measure == {(s, "softplus.value") for s in ("activate", "activate_with_slope", "milstein_hidden",
                                                                        "hidden_act")} | {("hidden_act", "lipswish.value")}
    # and nothing is worse than what the corrected comment states
    assert all(forms.E_form(s, q) <= 1.8e-7 for s in forms.SITES for q in forms.quantities(s) if q.endswith(".value"))
    assert all(forms.E_form(s, "tanh.slope") <= 3.5e-7 for s, _ in tanh_slopes)
    assert all(forms.E_form(s, q) <= 8e-8 for s in forms.SITES for q in forms.quantities(s)
               if q in ("sigmoid.slope", "softplus.slope"))
    assert forms.E_form("hidden_act", "lipswish.slope") <= 9e-7


def test_the_two_softplus_slope_forms():
    """1 - rcp(1 + ex) (tsde_mlp.h) and ex * rcp(1 + ex) (mlp_general.hip, Milstein) coexist: the same worst error in the measure
    of this module, but the product keeps its RELATIVE accuracy where the slope is small (x < 0) and the difference does not."""
    x = forms.sample_grid()
    ref = forms.reference(x)["softplus.slope"]
    diff = forms.emulate("activate_with_slope", x)["softplus.slope"].astype(np.float64)
    prod = forms.emulate("milstein_hidden", x)["softplus.slope"].astype(np.float64)
    assert abs(forms.E_form("activate_with_slope", "softplus.slope") - forms.E_form("milstein_hidden", "softplus.slope")) < 1e-8
    deep = (x < -1) & (x > -80)
    # (the rounding of x * log2(e), 2^-24 of an argument of up to 115, is a relative 115 * ln 2 * 2^-24 = 4.8e-6 of exp2)
    assert (np.abs(prod - ref)[deep] / ref[deep]).max() < 1e-5
    assert (np.abs(diff - ref)[deep] / ref[deep]).max() > 0.5            # (1 - rcp(1 + ex) is 0 or 2^-24 from x = -17 down)
    assert np.all(np.abs(prod - ref) <= np.abs(diff - ref) + 2.0 ** -24)
