"""Host model of the adaptive controller tables (test infrastructure: plain Python and numpy, no GPU, no package code).

Written from the reference's own lines, not from csrc/adaptive.hip:
  * `_core/base_solver.py:117-145`        the stepping loop: next_t, the midpoint, accept / reject, dt_min, the output loop;
  * `_core/adaptive_stepping.py:21-39`    `update_step_size`, the PI controller;
  * `_core/interp.py:15-18`               the interpolation weights of an output row;
  * `_brownian/brownian_interval.py:647-672`   how the increments of two adjacent intervals are joined.

What the model keeps is what the device keeps: a 22-word float64 `ctl` and a `scal` array of the solve's dtype T, laid out as
`include/torchsde_amd.h` says (`_native.CTL_*`, `SUB_*`, `SCAL_*` -- the layout constants are the only thing taken from the
package). Times are advanced in numpy scalars of T, as `solvers._integrate_adaptive` advances them; the step size, the error
ratio and the controller's powers are Python floats; stage times follow `BaseSDESolver._stage_times_host`; sqrt is `np.sqrt`
in T and 1/dt is `T(1) / dt`.

A model can be seeded from any (ctl, scal) pair (`seed`), so that a test can apply ONE controller call to the state the
device is in and compare the two results word by word.
"""
import numpy as np

from torchsde_amd import _native as N

NAN_MESSAGE = "Found nans in the error estimate. Try increasing the tolerance or regularizing the dynamics."


def update_step_size(error_estimate, prev_step_size, prev_error_ratio=None, safety=0.9, facmin=0.2, facmax=1.4):
    """adaptive_stepping.py:21-39 on Python floats. `prev_error_ratio` None: no accepted step yet."""
    if error_estimate > 1:
        pfactor = 0
        ifactor = 1 / 1.5
    else:
        pfactor = 0.13
        ifactor = 1 / 4.5
    error_ratio = safety / error_estimate
    if prev_error_ratio is None:
        prev_error_ratio = error_ratio
    factor = error_ratio ** ifactor * (error_ratio / prev_error_ratio) ** pfactor
    if error_estimate <= 1:
        prev_error_ratio = error_ratio
        facmin = 1.0
    factor = min(facmax, max(facmin, factor))
    return prev_step_size * factor, prev_error_ratio


def factor_is_clamped(error_estimate, prev_error_ratio=None, safety=0.9, facmin=0.2, facmax=1.4, margin=1e-9):
    """True where `update_step_size` returns prev_step_size times facmin or facmax whatever the last place of its two powers
    (the unclamped factor is further than `margin`, relatively, beyond the clamp): the result involves no `pow` rounding."""
    if error_estimate > 1:
        pfactor, ifactor = 0, 1 / 1.5
    else:
        pfactor, ifactor, facmin = 0.13, 1 / 4.5, 1.0
    error_ratio = safety / error_estimate
    if prev_error_ratio is None:
        prev_error_ratio = error_ratio
    factor = error_ratio ** ifactor * (error_ratio / prev_error_ratio) ** pfactor
    return factor >= facmax * (1 + margin) or factor <= facmin * (1 - margin)


def stage_times(t0, t1, stage_fracs):
    """`BaseSDESolver._stage_times_host`: t0 + frac * dt per stage (t0 itself where frac is 0), then t1."""
    T = type(t0)
    dt = T(t1 - t0)
    return [t0 if frac == 0 else t0 + T(frac) * dt for frac in stage_fracs] + [t1]


def interp_weights(prev_t, curr_t, out_t):
    """interp.py:15-18 in T: ((t1 - t) / (t1 - t0), (t - t0) / (t1 - t0)); a state that has not moved gives (0, 1)."""
    T = type(curr_t)
    if curr_t > prev_t:
        return (curr_t - out_t) / (curr_t - prev_t), (out_t - prev_t) / (curr_t - prev_t)
    return T(0), T(1)


def merge_halves(Wa, Ha, Wb, Hb, ha, hb, want_U=True):
    """(W, U) of [s, t] from the (W, H) of [s, u] and [u, t] (brownian_interval.py:647-672, then `_H_to_U`:102-103): arrays of
    T, widths ha = u - s and hb = t - u doubles that meet the arrays as T, their sum formed in double first."""
    T = Wa.dtype.type
    with np.errstate(all="ignore"):
        W = Wa + Wb
        if not want_U:
            return W, None
        tha, thb, tsum = T(ha), T(hb), T(ha + hb)
        term1 = thb * (Hb + T(0.5) * Wa)
        term2 = tha * (Ha - T(0.5) * Wb)
        H = (term1 + term2) / tsum
        return W, tsum * (T(0.5) * W + H)


def error_norm_terms(yf, yh, rtol, atol, eps):
    """The per-element terms ((yf - yh) / tol)^2 of adaptive_stepping.py:42-76 in T, tol = max(eps, rtol max(|yf|, |yh|) + atol),
    written with comparisons (a NaN passes through every one of them the way it does through the selects of a kernel)."""
    T = yf.dtype.type
    rtol, atol, eps = T(rtol), T(atol), T(eps)
    with np.errstate(all="ignore"):
        fa = np.where(yf < 0, -yf, yf)
        fb = np.where(yh < 0, -yh, yh)
        tol = rtol * np.where(fa > fb, fa, fb) + atol
        tol = np.where(tol < eps, eps, tol)
        ratio = (yf - yh) / tol
        return (ratio * ratio).astype(np.float64)


def error_norm(yf, yh, rtol, atol, eps):
    """max(eps, sqrt(sum(terms) / n)) with the sum taken exactly (`math.fsum`); a NaN or an infinite term gives what IEEE
    addition gives."""
    import math
    terms = error_norm_terms(yf, yh, rtol, atol, eps)
    if not np.isfinite(terms).all():
        total = float(np.sum(terms))
    else:
        total = math.fsum(terms.tolist())
    err = math.sqrt(total / terms.size) if total == total else float("nan")
    eps_t = float(yf.dtype.type(eps))
    return eps_t if err < eps_t else err


class ControllerModel:
    def __init__(self, dtype, stage_fracs, log_capacity=8192):
        self.T = np.dtype(dtype).type
        self.stage_fracs = tuple(stage_fracs)
        assert len(self.stage_fracs) <= N.ADAPTIVE_MAX_STAGES - 1
        self.ctl = np.zeros(N.CTL_SIZE, dtype=np.float64)
        self.scal = np.zeros(N.SCAL_SIZE, dtype=self.T)
        self.out_times = np.zeros(0, dtype=np.float64)
        self.log_capacity = log_capacity
        self.accept_log = np.zeros(2 * log_capacity, dtype=np.float64)

    # ---- state ---------------------------------------------------------------------------------------------------------
    def load(self, t0, t_end, step_size, dt_min):
        self.ctl[:] = 0.0
        self.ctl[N.CTL_CURR_T] = self.ctl[N.CTL_PREV_T] = t0
        self.ctl[N.CTL_STEP_SIZE] = step_size
        self.ctl[N.CTL_PREV_ERROR_RATIO] = np.nan
        self.ctl[N.CTL_T_END] = t_end
        self.ctl[N.CTL_DT_MIN] = dt_min

    def seed(self, ctl, scal, accept_log=None):
        """Take over a state (copies)."""
        self.ctl[:] = ctl
        self.scal[:] = scal
        if accept_log is not None:
            self.accept_log[:] = accept_log

    def _t(self, word):
        return self.T(self.ctl[word])

    @property
    def prev_error_ratio(self):
        value = float(self.ctl[N.CTL_PREV_ERROR_RATIO])
        return None if value != value else value

    # ---- the pieces --------------------------------------------------------------------------------------------------------
    def _next_t(self):
        """base_solver.py:116 with numpy scalars of T: min(curr_t + step_size, ts[-1])."""
        curr_t, t_end = self._t(N.CTL_CURR_T), self._t(N.CTL_T_END)
        nxt = curr_t + self.T(float(self.ctl[N.CTL_STEP_SIZE]))
        return nxt if nxt <= t_end else t_end

    def _write_sub(self, sub, t0, t1):
        T = self.T
        row = self.scal[sub * N.SUB_STRIDE:(sub + 1) * N.SUB_STRIDE]
        with np.errstate(all="ignore"):
            dt = T(t1 - t0)
            row[N.SUB_DT] = dt
            row[N.SUB_HALF_DT] = T(0.5) * dt
            row[N.SUB_SQRT_DT] = np.sqrt(dt)
            row[N.SUB_RDT] = T(1) / dt
            times = stage_times(t0, t1, self.stage_fracs)
        row[N.SUB_TIMES:N.SUB_TIMES + len(times)] = times

    def _advance_outputs(self):
        """The output loop (base_solver.py:114-115, 147): every output time that `curr_t < out_t` no longer holds for is
        reached, its row is due, and the loop aims at the next one."""
        n_out = len(self.out_times)
        idx = first = int(self.ctl[N.CTL_OUT_IDX])
        curr_t = self._t(N.CTL_CURR_T)
        while idx < n_out and not curr_t < self.T(self.out_times[idx]):
            idx += 1
        self.ctl[N.CTL_EMIT_FIRST] = first
        self.ctl[N.CTL_EMIT_COUNT] = idx - first
        self.ctl[N.CTL_OUT_IDX] = idx
        if n_out > 0:
            self.ctl[N.CTL_OUT_T] = self.out_times[min(idx, n_out - 1)]

    def refresh(self):
        """Everything the next attempt reads: the three sub-steps' rows of `scal`, the bounds and widths of the two
        half-step queries; or, with the last output time reached, the weights of its row."""
        curr_t, prev_t, out_t = self._t(N.CTL_CURR_T), self._t(N.CTL_PREV_T), self._t(N.CTL_OUT_T)
        active = bool(curr_t < out_t)
        self.ctl[N.CTL_ACTIVE] = 1.0 if active else 0.0
        if active:
            next_t = self._next_t()
            mid = self.T(0.5) * (curr_t + next_t)
            self._write_sub(0, curr_t, next_t)
            self._write_sub(1, curr_t, mid)
            self._write_sub(2, mid, next_t)
            self.ctl[N.CTL_BOUNDS_A:N.CTL_BOUNDS_A + 2] = float(curr_t), float(mid)
            self.ctl[N.CTL_BOUNDS_B:N.CTL_BOUNDS_B + 2] = float(mid), float(next_t)
            # solvers._step_doubling_noise: widths of the halves from the times as Python floats
            self.ctl[N.CTL_WIDTHS] = float(mid) - float(curr_t)
            self.ctl[N.CTL_WIDTHS + 1] = float(next_t) - float(mid)
        else:
            with np.errstate(all="ignore"):
                w0, w1 = interp_weights(prev_t, curr_t, out_t)
            self.scal[N.SCAL_W0], self.scal[N.SCAL_W1] = w0, w1

    # ---- the calls ---------------------------------------------------------------------------------------------------------
    def begin(self, out_times):
        self.out_times = np.array(out_times, dtype=np.float64)
        self.scal[N.SCAL_ACCEPT] = 0
        self.ctl[N.CTL_N_OUT] = len(self.out_times)
        self.ctl[N.CTL_OUT_IDX] = 0.0
        self._advance_outputs()
        self.refresh()

    def propose(self, err):
        """base_solver.py:128-137: (next step size, next prev_error_ratio or None, whether dt_min was hit)."""
        dt_min = float(self.ctl[N.CTL_DT_MIN])
        step_size, prev_error_ratio = update_step_size(float(err), float(self.ctl[N.CTL_STEP_SIZE]), self.prev_error_ratio)
        if step_size < dt_min:
            return dt_min, None, True
        return step_size, prev_error_ratio, False

    def control(self, err, proposal=None):
        """One pass of base_solver.py:125-142 after an attempt whose error estimate is `err`. `proposal`: what `propose`
        returns, or the same triple from elsewhere (a device whose `pow` may differ from CPython's in the last place):
        the decision, the times and the tables follow from it."""
        err = float(err)
        self.scal[N.SCAL_ACCEPT] = 0
        self.ctl[N.CTL_EMIT_COUNT] = 0.0
        if self.ctl[N.CTL_ACTIVE] == 0.0:
            return                      # the outer loop is over: nothing is attempted any more
        if err != err:
            raise AssertionError(NAN_MESSAGE)
        dt_min = float(self.ctl[N.CTL_DT_MIN])
        next_t = self._next_t()         # of the attempt that was just made, with the step size it was made with
        step_size, prev_error_ratio, hit = self.propose(err) if proposal is None else proposal
        if hit:
            self.ctl[N.CTL_DT_MIN_HITS] += 1.0
        self.ctl[N.CTL_ATTEMPTS] += 1.0
        if err <= 1 or step_size <= dt_min:
            self.ctl[N.CTL_PREV_T] = self.ctl[N.CTL_CURR_T]
            self.ctl[N.CTL_CURR_T] = float(next_t)
            k = int(self.ctl[N.CTL_ACCEPTED])
            if k < self.log_capacity:
                self.accept_log[2 * k] = self.ctl[N.CTL_PREV_T]
                self.accept_log[2 * k + 1] = self.ctl[N.CTL_CURR_T]
            self.ctl[N.CTL_ACCEPTED] += 1.0
            self.scal[N.SCAL_ACCEPT] = 1
        self.ctl[N.CTL_STEP_SIZE] = step_size
        self.ctl[N.CTL_PREV_ERROR_RATIO] = np.nan if prev_error_ratio is None else prev_error_ratio
        self._advance_outputs()
        self.refresh()

    def emit_rows(self, prev_y, curr_y):
        """{row index: w0 * prev_y + w1 * curr_y in T} for the rows the last call marked."""
        first, count = int(self.ctl[N.CTL_EMIT_FIRST]), int(self.ctl[N.CTL_EMIT_COUNT])
        prev_t, curr_t = self._t(N.CTL_PREV_T), self._t(N.CTL_CURR_T)
        rows = {}
        with np.errstate(all="ignore"):
            for j in range(first, first + count):
                w0, w1 = interp_weights(prev_t, curr_t, self.T(self.out_times[j]))
                rows[j] = w0 * prev_y + w1 * curr_y
        return rows

    def commit(self, prev_y, curr_y, y_next):
        """prev_y <- curr_y, curr_y <- y_next (in place) iff the last call accepted its attempt."""
        if self.scal[N.SCAL_ACCEPT] != 0:
            prev_y[...] = curr_y
            curr_y[...] = y_next

    def merge_halves(self, Wa, Ha, Wb, Hb, want_U=True):
        return merge_halves(Wa, Ha, Wb, Hb, float(self.ctl[N.CTL_WIDTHS]), float(self.ctl[N.CTL_WIDTHS + 1]), want_U)
