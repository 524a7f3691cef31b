"""What tests/test_neural_activation_forms.py, tests/test_gpu_neural_activations.py and tools/neural_activation_accuracy.py
share (a helper: nothing here is collected, and nothing here touches a GPU).

The matrix-core kernels evaluate their activations with hand-written formulas on the raw hardware transcendentals (v_exp_f32,
v_rcp_f32, v_log_f32), written out at eleven places in four algebraic forms. This module states

  the reference   float64 tanh, 1/(1+exp(-x)), x*sigmoid(x), softplus with the module's own semantics (x above 20, log1p(exp(x))
                  otherwise, slope 1 above 20) and their analytic derivatives -- `reference`; `reference_mp` is the same at 50
                  digits (mpmath), the check of the float64 statement;
  the forms       every site's formula exactly as its source has it, in numpy float32 -- `SITES`. Every exp2, reciprocal and
                  log2 is computed in float64 and rounded ONCE (`Primitives`); every other operation is a float32 operation. A
                  seeded `Primitives` moves each primitive result by a random -1, 0 or +1 ulp: the hardware's are specified to
                  1 ulp, not correctly rounded;
  the grid        `sample_grid`: 32 seeded mantissas in every binade 2^-30 .. 2^7 of both signs, and the edges at which a form
                  changes character (0, +-2^-100, the softplus threshold and its neighbours, the saturation points of tanh and
                  sigmoid in float32, the overflow of exp2, the largest floats). No subnormal inputs;
  the measure     `measure`: |got - ref| / max(1, |ref|) -- absolute below 1, relative above (relative error of tanh near 0 is
                  unbounded for any form that goes through exp);
  the bound       `bound(site, quantity)` = 2 * E_form + 2^-24, E_form the worst measure of the correctly rounded emulation over
                  the grid: the factor 2 for primitives that are 1 ulp instead of correctly rounded, 2^-24 for the read-out's own
                  half ulp. A condition on the kernel that comes from the formula and the float64 reference, never from the
                  kernel."""
import functools

import numpy as np

F = np.float32
LOG2E = F(1.4426950408889634)
LN2 = F(0.6931471805599453)
NEG_LOG2E = F(-1.4426950408889634)
TWO_LOG2E = F(2.0) * LOG2E                # `2.0f * kLog2e`, folded by the compiler in float
ONE, TWO, THRESHOLD = F(1.0), F(2.0), F(20.0)
LIPSWISH_C = F(0.909)                     # examples/sde_gan.py:44-47
HEADER_CLAIM = 3e-7                       # "Absolute error <= 3e-7", csrc/tsde_mlp.h before this module existed
READ_OUT = 2.0 ** -24
TINY = np.finfo(F).tiny


# ---- the grid ----------------------------------------------------------------------------------------------------------------
EDGES = (8.5, 9.1, 16.6, 17.4, 44.0, 88.0, 89.0, 104.0, 127.0, 1e4, 3e38)


@functools.lru_cache(maxsize=None)
def _grid(seed):
    rng = np.random.default_rng(seed)
    parts = []
    for e in range(-30, 8):
        mantissa = rng.integers(0, 1 << 23, size=32, dtype=np.uint32)
        v = (np.uint32((e + 127) << 23) | mantissa).view(F)
        parts += [v, -v]
    twenty = F(20.0)
    edges = [0.0, 2.0 ** -100, -2.0 ** -100, twenty, np.nextafter(twenty, F(np.inf)), np.nextafter(twenty, F(-np.inf)), -twenty]
    for v in EDGES:
        edges += [v, -v]
    x = np.concatenate(parts + [np.asarray(edges, dtype=F)])
    x.setflags(write=False)
    return x


def sample_grid(seed=20):
    """The float32 sample points (read-only; the same array for the same seed)."""
    return _grid(seed)


def binade(x):
    """Label of a sample for the accuracy table: sign and floor(log2 |x|), or "0"."""
    if x == 0:
        return "0"
    return ("-" if x < 0 else "+") + f"2^{int(np.floor(np.log2(abs(float(x))))):+d}"


# ---- the reference -----------------------------------------------------------------------------------------------------------
QUANTITIES = ("tanh.value", "tanh.slope", "softplus.value", "softplus.slope", "sigmoid.value", "sigmoid.slope",
              "lipswish.value", "lipswish.slope")


def reference(x, c=LIPSWISH_C):
    """{quantity: float64 array} at the float32 points x. lipswish = c * x * sigmoid(x)."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    c = float(F(c))
    with np.errstate(over="ignore", under="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
        s_neg = 1.0 / (1.0 + np.exp(x))                       # 1 - s without the cancellation
        inside = x <= 20.0
        soft = np.where(inside, np.log1p(np.exp(np.where(inside, x, 0.0))), x)
        sech = 1.0 / np.cosh(x)
    return {"tanh.value": np.tanh(x), "tanh.slope": sech * sech,
            "softplus.value": soft, "softplus.slope": np.where(inside, s, 1.0),
            "sigmoid.value": s, "sigmoid.slope": s * s_neg,
            "lipswish.value": c * (x * s), "lipswish.slope": c * (s * (1.0 + x * s_neg))}


def reference_mp(x, c=LIPSWISH_C, digits=50):
    """The same at `digits` digits (mpmath), returned as lists of mpf: the yardstick of `reference`."""
    import mpmath
    out = {q: [] for q in QUANTITIES}
    with mpmath.workprec(int(digits * 3.33) + 8):
        cm = mpmath.mpf(float(F(c)))
        for v in np.asarray(x, dtype=F):
            t = mpmath.mpf(float(v))
            s = 1 / (1 + mpmath.exp(-t))
            s_neg = 1 / (1 + mpmath.exp(t))
            above = float(v) > 20.0
            out["tanh.value"].append(mpmath.tanh(t))
            out["tanh.slope"].append(mpmath.sech(t) ** 2)
            out["softplus.value"].append(t if above else mpmath.log1p(mpmath.exp(t)))
            out["softplus.slope"].append(mpmath.mpf(1) if above else s)
            out["sigmoid.value"].append(s)
            out["sigmoid.slope"].append(s * s_neg)
            out["lipswish.value"].append(cm * t * s)
            out["lipswish.slope"].append(cm * s * (1 + t * s_neg))
    return out


def measure(got, ref):
    """|got - ref| / max(1, |ref|), in float64; a `got` that is not finite measures infinite."""
    got = np.asarray(got).astype(np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return np.where(np.isfinite(got), err, np.inf)


# ---- the hardware primitives -------------------------------------------------------------------------------------------------
class Primitives:
    """exp2, reciprocal and log2 in float64, rounded once to float32; with a seed, each result then moves by a random -1, 0 or
    +1 ulp. Zeros, infinities and results at the edge of the normal range stay; so does -- unless `move_exact` -- a result that
    IS a float32 (exp2(0) = 1, 1/1 = 1, 1/2^k): no implementation misses those, and one form depends on it -- the LipSwish slope
    multiplies x by 1 - rcp(1 + 0), see tests/test_neural_activation_forms.py."""

    def __init__(self, seed=None, move_exact=False):
        self.rng = None if seed is None else np.random.default_rng(seed)
        self.move_exact = move_exact

    def _round(self, r64):
        with np.errstate(over="ignore", under="ignore"):
            r = np.asarray(r64).astype(F)
        if self.rng is not None:
            k = self.rng.integers(-1, 2, size=r.shape)
            up, down = np.nextafter(r, F(np.inf)), np.nextafter(r, F(-np.inf))
            moved = np.where(k > 0, up, np.where(k < 0, down, r)).astype(F)
            ok = np.isfinite(r) & (np.abs(r) >= TINY) & np.isfinite(moved) & (np.abs(moved) >= TINY)
            if not self.move_exact:
                ok &= r.astype(np.float64) != np.asarray(r64, dtype=np.float64)
            r = np.where(ok, moved, r).astype(F)
        return r

    def exp2(self, a):
        with np.errstate(over="ignore", under="ignore"):
            return self._round(np.exp2(np.asarray(a, dtype=F).astype(np.float64)))

    def rcp(self, a):
        with np.errstate(divide="ignore", over="ignore"):
            return self._round(1.0 / np.asarray(a, dtype=F).astype(np.float64))

    def log2(self, a):
        with np.errstate(divide="ignore"):
            return self._round(np.log2(np.asarray(a, dtype=F).astype(np.float64)))


# ---- the eleven sites, each exactly as its source states it ------------------------------------------------------------------------
# Every function takes float32 points and returns {quantity: float32 array}; `hw` supplies the three primitives.
def _f32(x):
    return np.asarray(x, dtype=F)


def _tanh_value(x, hw, factor=TWO_LOG2E):
    e2x = hw.exp2(x * factor)
    return ONE - TWO * hw.rcp(e2x + ONE)


def _softplus_value(x, hw):
    ex = hw.exp2(x * LOG2E)
    sp = hw.log2(ONE + ex) * LN2
    return ex, np.where(x > THRESHOLD, x, sp).astype(F)


def _sigmoid(x, hw):
    return hw.rcp(ONE + hw.exp2(x * NEG_LOG2E))


def form_activate(x, hw):
    """csrc/tsde_mlp.h `activate<ACT>`."""
    x = _f32(x)
    return {"tanh.value": _tanh_value(x, hw), "softplus.value": _softplus_value(x, hw)[1]}


def form_activate_with_slope(x, hw):
    """csrc/tsde_mlp.h `activate_with_slope<ACT>`."""
    x = _f32(x)
    value = _tanh_value(x, hw)
    ex, soft = _softplus_value(x, hw)
    slope = np.where(x > THRESHOLD, ONE, ONE - hw.rcp(ONE + ex)).astype(F)
    return {"tanh.value": value, "tanh.slope": ONE - value * value, "softplus.value": soft, "softplus.slope": slope}


def form_diffusion_value(x, hw, amp=ONE):
    """csrc/tsde_mlp.h `diffusion_value` with the sample as the argument u = c*y + e (y = 0, e = x)."""
    x = _f32(x)
    s = _sigmoid(x, hw)
    g = F(amp) * s
    return {"sigmoid.value": g, "sigmoid.slope": g * (ONE - s)}


def form_finalise(x, hw):
    """csrc/mlp_general.hip `finalise<true>`: the closing sigmoid for diagonal and scalar noise."""
    return {"sigmoid.value": _sigmoid(_f32(x), hw)}


def form_staged_bias(x, hw, acc=F(0.0)):
    """csrc/mlp_general.hip `close_tile`: the closing sigmoid for general noise. The bias is staged as b2 * -log2(e) (a float32
    product); the argument of exp2 is fmaf(acc, -log2(e), staged): the product in float64, one rounding."""
    x = _f32(x)
    staged = x * NEG_LOG2E
    with np.errstate(over="ignore", invalid="ignore"):
        arg = (np.float64(acc) * np.float64(NEG_LOG2E) + staged.astype(np.float64)).astype(F)
    return {"sigmoid.value": hw.rcp(ONE + hw.exp2(arg))}


def form_milstein_hidden(x, hw):
    """csrc/mlp_general.hip `diffusion_hidden_with_slope`: values through `activate`, slopes 1 - v^2 and ex * rcp(1 + ex)."""
    x = _f32(x)
    v = _tanh_value(x, hw)
    _, soft = _softplus_value(x, hw)
    ex = hw.exp2(x * LOG2E)                                  # (a second exponential in the source, too)
    slope = np.where(x > THRESHOLD, ONE, ex * hw.rcp(ONE + ex)).astype(F)
    return {"tanh.value": v, "tanh.slope": ONE - v * v, "softplus.value": soft, "softplus.slope": slope}


def form_milstein_closing(x, hw, scale=ONE):
    """csrc/mlp_general.hip `diffusion_values_with_slope`: g = scale * s, dg = (scale * s) * (1 - s)."""
    s = _sigmoid(_f32(x), hw)
    g = F(scale) * s
    return {"sigmoid.value": g, "sigmoid.slope": g * (ONE - s)}


def form_hidden_act(x, hw, c=LIPSWISH_C):
    """csrc/tsde_neural_rheun.h `hidden_act<ACT>`: LipSwish c * (x * s) with slope c * (s * (1 + x * (1 - s))); tanh and softplus
    through `activate_with_slope` (their act_scale is 1 in this table: multiplying by 1 rounds nothing)."""
    x = _f32(x)
    c = F(c)
    s = _sigmoid(x, hw)
    with np.errstate(invalid="ignore", over="ignore"):
        out = {"lipswish.value": c * (x * s), "lipswish.slope": c * (s * (ONE + x * (ONE - s)))}
    out.update(form_activate_with_slope(x, hw))
    return out


def form_final_act(x, hw):
    """csrc/tsde_neural_rheun.h `final_act<FINAL>`."""
    x = _f32(x)
    s = _sigmoid(x, hw)
    v = _tanh_value(x, hw)
    return {"sigmoid.value": s, "sigmoid.slope": s * (ONE - s), "tanh.value": v, "tanh.slope": ONE - v * v}


def form_adjoint_diffusion(x, hw, amp=ONE):
    """csrc/mlp_adjoint.hip, the elementwise phase of the stochastic adjoint: its own statement of the sigmoid diffusion (not
    `diffusion_value`), sg = rcp(1 + exp2(-u log2 e)), g = amp * sg, q = g * (1 - sg). (Its q' = q * (1 - 2 sg) reaches the
    outputs only in products with the rate c and the Ito correction: no read-out isolates it.)"""
    s = _sigmoid(_f32(x), hw)
    g = F(amp) * s
    return {"sigmoid.value": g, "sigmoid.slope": g * (ONE - s)}


def form_final_slope(x, hw):
    """csrc/rheun_grad.hip `final_slope<FINAL>`: the closing slopes once more, for dL/dW2 and dL/db2 of a general-noise net."""
    x = _f32(x)
    s = _sigmoid(x, hw)
    v = _tanh_value(x, hw)
    return {"sigmoid.slope": s * (ONE - s), "tanh.slope": ONE - v * v}


SITES = {
    "activate": form_activate,
    "activate_with_slope": form_activate_with_slope,
    "diffusion_value": form_diffusion_value,
    "finalise": form_finalise,
    "staged_bias": form_staged_bias,
    "milstein_hidden": form_milstein_hidden,
    "milstein_closing": form_milstein_closing,
    "hidden_act": form_hidden_act,
    "final_act": form_final_act,
    "adjoint_diffusion": form_adjoint_diffusion,
    "final_slope": form_final_slope,
}


def emulate(site, x, seed=None, move_exact=False):
    """{quantity: float32 array} of `site` at x; `seed`: perturb every primitive result by -1, 0 or +1 ulp."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return SITES[site](x, Primitives(seed, move_exact))


@functools.lru_cache(maxsize=None)
def _worst(site, seed):
    x = sample_grid(seed)
    ref = reference(x)
    got = emulate(site, x)
    near = np.abs(x) <= 20.0                    # (absolute error means something only where the values are of order one)
    return {q: (float(measure(v, ref[q]).max()), float(np.abs(v.astype(np.float64) - ref[q])[near].max()))
            for q, v in got.items()}


def quantities(site):
    return tuple(_worst(site, 20))


def E_form(site, quantity, seed=20):
    """Worst measure of the correctly rounded emulation of (site, quantity) over the sample grid."""
    return _worst(site, seed)[quantity][0]


def E_abs(site, quantity, seed=20):
    """Its worst ABSOLUTE error over |x| <= 20 (the measure the old header comment claimed 3e-7 in)."""
    return _worst(site, seed)[quantity][1]


def bound(site, quantity):
    """The most a kernel's value may be off at a point, in `measure`."""
    return 2.0 * E_form(site, quantity) + READ_OUT


def over_the_header_claim():
    """[(site, quantity, E_form, worst absolute error)] of the forms whose ideal-primitive emulation already exceeds the 3e-7
    that csrc/tsde_mlp.h used to claim, in the measure of this module or (as the comment had it) absolutely."""
    return [(s, q, E_form(s, q), E_abs(s, q)) for s in SITES for q in quantities(s)
            if max(E_form(s, q), E_abs(s, q)) > HEADER_CLAIM]
