"""tests/adaptive_model.py (the host model the device's controller tables are compared with, tests/test_gpu_adaptive_controller.py)
against what it restates: the REAL reference's `update_step_size` (recorded: tests/golden/adaptive_controller_reference.npz),
the host-driven adaptive loop of this package (`solvers._integrate_adaptive`, which tests/test_oracle_solvers.py and the
adaptive_*.npz fixtures pin to the reference's loop), and the oracle's C statement of the generator's merge. No GPU."""
import math
import os
import types

import numpy as np
import pytest

from oracle import counter
from tests import adaptive_model as M
from torchsde_amd import _native as N
from torchsde_amd import solvers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adaptive_controller_reference.npz")


def _bits(x):
    return np.asarray(x).view(np.uint64 if np.asarray(x).dtype == np.float64 else np.uint32)


def test_step_size_function_reproduces_the_reference_bit_for_bit():
    z = np.load(GOLDEN)
    n = len(z["error_estimate"])
    assert n >= 300
    errs = z["error_estimate"]
    assert errs.min() <= 1e-7 and errs.max() >= 1e6 and (errs == 1.0).any()
    assert (errs == np.nextafter(1.0, 0.0)).any() and (errs == np.nextafter(1.0, 2.0)).any()
    factors = z["new_step_size"] / z["prev_step_size"]
    assert (np.abs(factors - 0.2) < 1e-15).any() and (np.abs(factors - 1.4) < 1e-15).any() and (factors == 1.0).any()
    assert ((factors > 0.21) & (factors < 0.99)).any() and ((factors > 1.01) & (factors < 1.39)).any()
    for i in range(n):
        per = float(z["prev_error_ratio"][i])
        step, ratio = M.update_step_size(float(errs[i]), float(z["prev_step_size"][i]), None if per != per else per)
        want_ratio = float(z["new_prev_error_ratio"][i])
        # both sides are CPython doubles computed by the same expressions: exact equality
        assert step == float(z["new_step_size"][i]), i
        assert (ratio is None and want_ratio != want_ratio) or ratio == want_ratio, i
        # ... and the package's own host controller is the same function
        step2, ratio2 = solvers._update_step_size(float(errs[i]), float(z["prev_step_size"][i]), None if per != per else per)
        assert step2 == step and ratio2 == ratio, i


def test_clamp_predicate_agrees_with_the_fixture():
    z = np.load(GOLDEN)
    seen = 0
    for i in range(len(z["error_estimate"])):
        per = float(z["prev_error_ratio"][i])
        e, s = float(z["error_estimate"][i]), float(z["prev_step_size"][i])
        if M.factor_is_clamped(e, None if per != per else per):
            facmin = 0.2 if e > 1 else 1.0
            assert float(z["new_step_size"][i]) in (s * facmin, s * 1.4), i
            seen += 1
    assert seen >= 100


def _host_loop(np_dtype, ts, dt, dt_min, fracs, errors):
    """`solvers._integrate_adaptive`'s loop (the lines between the step launches), fed scripted error estimates: one record per
    attempt, and per output time the attempt count at which it was interpolated with its weights."""
    me = types.SimpleNamespace(stage_fracs=fracs)
    ts_host = np.asarray(ts, dtype=np_dtype)
    t_end = ts_host[-1]
    step_size, prev_error_ratio = dt, None
    prev_t = curr_t = ts_host[0]
    errors = iter(errors)
    attempts, outputs, hits = [], [], 0
    for out_t in ts_host[1:]:
        while curr_t < out_t:
            nxt = curr_t + np_dtype(step_size)
            next_t = nxt if nxt <= t_end else t_end
            midpoint_t = np_dtype(0.5) * (curr_t + next_t)
            times = (solvers.BaseSDESolver._stage_times_host(me, curr_t, next_t),
                     solvers.BaseSDESolver._stage_times_host(me, curr_t, midpoint_t),
                     solvers.BaseSDESolver._stage_times_host(me, midpoint_t, next_t))
            try:
                error_estimate = next(errors)
            except StopIteration:
                return attempts, outputs
            step_size, prev_error_ratio = solvers._update_step_size(error_estimate, step_size, prev_error_ratio)
            if step_size < dt_min:
                hits += 1
                step_size = dt_min
                prev_error_ratio = None
            accepted = error_estimate <= 1 or step_size <= dt_min
            if accepted:
                prev_t, curr_t = curr_t, next_t
            attempts.append(dict(times=times, t0=times[0][0], mid=midpoint_t, t1=next_t, step_size=step_size,
                                 ratio=prev_error_ratio, accepted=accepted, curr_t=curr_t, prev_t=prev_t, hits=hits))
        w0 = (curr_t - out_t) / (curr_t - prev_t) if curr_t > prev_t else np_dtype(0)
        w1 = (out_t - prev_t) / (curr_t - prev_t) if curr_t > prev_t else np_dtype(1)
        outputs.append((len(attempts), w0, w1))
    return attempts, outputs


ERRORS = [0.5, 0.2, 3.0, 1.7, 0.9, 1.0, float(np.nextafter(1.0, 2.0)), 1e-7, 0.4, 1e6, 1e6, 0.3, 0.6, 0.05, 40.0, 0.8, 0.7, 0.2,
          0.9, 0.95, 5.0, 0.5, 0.1, 0.3, 0.2, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1] * 2


@pytest.mark.parametrize("fracs", [(0,), (0, 0.5), (0, 0.25, 0.5, 0.75, 1)])
@pytest.mark.parametrize("np_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ts,dt,dt_min", [((0.0, 0.3, 0.35, 1.0), 0.1, 0.0), ((0.25, 0.26, 0.27, 0.27, 1.5), 0.07, 0.03),
                                          ((0.0, 0.0, 2.5), 0.3, 1e-3)])
def test_model_follows_the_host_loop(np_dtype, fracs, ts, dt, dt_min):
    attempts, outputs = _host_loop(np_dtype, ts, dt, dt_min, fracs, ERRORS)
    assert len(attempts) >= 8 and any(not a["accepted"] for a in attempts)
    model = M.ControllerModel(np_dtype, fracs)
    ts_host = np.asarray(ts, dtype=np_dtype)
    model.load(float(ts_host[0]), float(ts_host[-1]), dt, dt_min)
    model.begin([float(t) for t in ts_host[1:]])
    emitted = []

    def collect(n_attempts):
        rows = model.emit_rows(np.array([1, 0], dtype=np_dtype), np.array([0, 1], dtype=np_dtype))
        for j in sorted(rows):
            emitted.append((n_attempts, rows[j][0], rows[j][1]))
    collect(0)
    for k, (att, err) in enumerate(zip(attempts, ERRORS)):
        assert model.ctl[N.CTL_ACTIVE] == 1.0
        # what the attempt about to be judged ran with
        for sub, want in enumerate(att["times"]):
            row = model.scal[sub * N.SUB_STRIDE:(sub + 1) * N.SUB_STRIDE]
            got = row[N.SUB_TIMES:N.SUB_TIMES + len(want)]
            assert _bits(got).tolist() == _bits(np.array(want, dtype=np_dtype)).tolist(), (k, sub)
            dt_sub = np_dtype(want[-1] - want[0])
            assert row[N.SUB_DT] == dt_sub and row[N.SUB_HALF_DT] == np_dtype(0.5) * dt_sub
            assert row[N.SUB_SQRT_DT] == np.sqrt(dt_sub) and row[N.SUB_RDT] == np_dtype(1) / dt_sub
        assert model.ctl[N.CTL_BOUNDS_A] == float(att["t0"]) and model.ctl[N.CTL_BOUNDS_A + 1] == float(att["mid"])
        assert model.ctl[N.CTL_BOUNDS_B] == float(att["mid"]) and model.ctl[N.CTL_BOUNDS_B + 1] == float(att["t1"])
        assert model.ctl[N.CTL_WIDTHS] == float(att["mid"]) - float(att["t0"])
        assert model.ctl[N.CTL_WIDTHS + 1] == float(att["t1"]) - float(att["mid"])
        model.control(err)
        assert model.ctl[N.CTL_STEP_SIZE] == att["step_size"], k
        assert model.prev_error_ratio == att["ratio"], k
        assert model.ctl[N.CTL_CURR_T] == float(att["curr_t"]) and model.ctl[N.CTL_PREV_T] == float(att["prev_t"]), k
        assert bool(model.scal[N.SCAL_ACCEPT]) == att["accepted"], k
        assert model.ctl[N.CTL_ATTEMPTS] == k + 1 and model.ctl[N.CTL_DT_MIN_HITS] == att["hits"]
        assert model.ctl[N.CTL_ACCEPTED] == sum(a["accepted"] for a in attempts[:k + 1])
        collect(k + 1)
    want = [(n, w0, w1) for n, w0, w1 in outputs]
    assert len(emitted) == len(want)
    for (n_got, g0, g1), (n_want, w0, w1) in zip(emitted, want):
        assert n_got == n_want and _bits(np_dtype(g0)) == _bits(np_dtype(w0)) and _bits(np_dtype(g1)) == _bits(np_dtype(w1))
    if len(outputs) == len(ts) - 1:       # the script of errors carried the loop to the end
        assert model.ctl[N.CTL_ACTIVE] == 0.0 and model.ctl[N.CTL_OUT_IDX] == model.ctl[N.CTL_N_OUT] == len(ts) - 1
        assert model.ctl[N.CTL_CURR_T] == float(ts_host[-1])
        before = (model.ctl.copy(), model.scal.copy())
        model.control(0.5)                # nothing is attempted any more
        assert model.ctl[N.CTL_ATTEMPTS] == before[0][N.CTL_ATTEMPTS] and model.scal[N.SCAL_ACCEPT] == 0
    log = model.accept_log[:2 * int(model.ctl[N.CTL_ACCEPTED])].reshape(-1, 2)
    assert log.tolist() == [[float(a["t0"]), float(a["t1"])] for a in attempts if a["accepted"]]


def test_model_reaches_the_end_in_every_case():
    """(the scripted errors are long enough for the parametrised cases above to finish)"""
    for np_dtype in (np.float32, np.float64):
        for ts, dt, dt_min in [((0.0, 0.3, 0.35, 1.0), 0.1, 0.0), ((0.25, 0.26, 0.27, 0.27, 1.5), 0.07, 0.03),
                               ((0.0, 0.0, 2.5), 0.3, 1e-3)]:
            _, outputs = _host_loop(np_dtype, ts, dt, dt_min, (0,), ERRORS)
            assert len(outputs) == len(ts) - 1


def test_model_raises_on_a_nan_error_like_the_host():
    model = M.ControllerModel(np.float64, (0,))
    model.load(0.0, 1.0, 0.1, 0.0)
    model.begin([1.0])
    with pytest.raises(AssertionError, match="Found nans in the error estimate"):
        model.control(float("nan"))


@pytest.mark.parametrize("np_dtype", [np.float32, np.float64])
def test_merge_equals_the_oracles_interval_merge(np_dtype):
    rng = np.random.default_rng(5)
    n = 64
    Wa, Ha, Wb, Hb = (rng.standard_normal(n).astype(np_dtype) for _ in range(4))
    for ha, hb in [(0.05, 0.05), (0.0123, 0.3), (2.0 ** -9, 2.0 ** -9), (1e-5, 0.7)]:
        W, U = M.merge_halves(Wa, Ha, Wb, Hb, ha, hb)
        W_only, none = M.merge_halves(Wa, Ha, Wb, Hb, ha, hb, want_U=False)
        assert none is None and _bits(W_only).tolist() == _bits(W).tolist()
        hsum = np_dtype(ha + hb)
        for i in range(n):
            w, h = counter.interval_merge(float(Wa[i]), float(Ha[i]), ha, float(Wb[i]), float(Hb[i]), hb, True, dtype=np_dtype)
            assert _bits(np_dtype(w)) == _bits(W[i]), (i, ha, hb)
            # U = (t - s) (W / 2 + H)  (brownian_interval.py:102-103)
            assert _bits(hsum * (np_dtype(0.5) * np_dtype(w) + np_dtype(h))) == _bits(U[i]), (i, ha, hb)


def test_error_norm_model_is_the_reference_formula():
    """adaptive_stepping.py:42-76 with torch on the CPU (float64, where its sum is good to a few ulps)."""
    import torch
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(1000), rng.standard_normal(1000)
    rtol, atol, eps = 1e-3, 1e-4, 1e-7
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    tol = (rtol * torch.max(ta.abs(), tb.abs()) + atol).clamp_min(eps)
    want = torch.sqrt((((ta - tb) / tol) ** 2.).sum() / ta.numel()).clamp_min(eps).item()
    assert M.error_norm(a, b, rtol, atol, eps) == pytest.approx(want, rel=1e-13)
    assert M.error_norm(a, a, 0.0, 0.0, eps) == eps
    assert math.isnan(M.error_norm(np.array([np.inf, 1.0]), np.array([1.0, 1.0]), rtol, atol, eps))
