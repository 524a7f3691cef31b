"""The device side of adaptive stepping, kernel by kernel (``-m gpu``), against tests/adaptive_model.py -- a host model written
from the reference's lines (base_solver.py:117-145, adaptive_stepping.py:21-39, interp.py:15-18, brownian_interval.py:647-672)
and pinned to them on the CPU by tests/test_adaptive_model.py:

  2. `adaptive_begin_kernel` / `adaptive_control_kernel` driven directly through `adaptive.DeviceController` with scripted error
     estimates, no SDE and no solve, `ctl` and `scal` read back after every call;
  3. `tsde_adaptive_commit`, `tsde_adaptive_emit`, `tsde_merge_halves` bit for bit, inside guarded allocations;
  4. `tsde_brownian_query_dev` (the interval read from device memory, the cells located on the device) on grids of several cells;
  5. `tsde_error_norm` on the inputs tests/test_gpu_wrappers.py does not give it.

tests/test_gpu_adaptive_device.py compares whole solves; the words of the tables are only looked at here.
profiles/adaptive_controller_pow_ulps.txt: the measured distance behind `POW_ULPS_MEASURED` (tools/adaptive_controller_pow_ulps.py);
profiles/adaptive_controller_mutations.txt: one-line mutants of the kernels against this module.
"""
import math

import numpy as np
import pytest
import torch

from oracle import counter
from tests import adaptive_model as M
from torchsde_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
INT = {torch.float32: torch.int32, torch.float64: torch.int64}
DTYPES = [torch.float32, torch.float64]


# ------------------------------------------------------------------------------------------------------------------------------
# 2. The controller kernels
# ------------------------------------------------------------------------------------------------------------------------------
def stage_frac_tuples():
    """The tuples the solvers really carry, and one of ADAPTIVE_MAX_STAGES - 1 entries with a zero that is not first."""
    from torchsde_amd import solvers
    found = {tuple(cls.stage_fracs) for cls in vars(solvers).values()
             if isinstance(cls, type) and issubclass(cls, solvers.BaseSDESolver)}
    found = sorted(f for f in found if len(f) <= N.ADAPTIVE_MAX_STAGES - 1)
    extra = (0, 0.3, 0, 0.75, 1)
    assert len(extra) == N.ADAPTIVE_MAX_STAGES - 1 and (0,) in found and len(found) >= 3
    return found + [extra]


STAGE_FRACS = stage_frac_tuples()
ONE_UP = float(np.nextafter(1.0, 2.0))
NAN = float("nan")

# The worst distance between the device's and CPython's proposed step size over every unclamped call of every sequence below
# (profiles/adaptive_controller_pow_ulps.txt). The assertion is the usual "twice the worst measured, floored".
POW_ULPS_MEASURED = 1
POW_ULPS_BOUND = max(4, 2 * POW_ULPS_MEASURED)

# name -> (t0, t_end, first step size, dt_min, output times, error estimates)
SEQUENCES = {
    # dt_min == 0; first call with no previous ratio; growth capped at 1.4; error exactly 1 (accepted) and its upper neighbour
    # (rejected); 1e6 clamped at 0.2; 1e-7; reject, reject, accept; unclamped factors on both branches
    "regimes": (0.0, 10.0, 0.01, 0.0, [10.0],
                [1e-3, 1e-7, 0.5, 0.9, 1.0, ONE_UP, 1e6, 3.0, 2.0, 0.7, 0.95, 0.3, 1.2, 0.8, 10.0, 0.6, 0.45, 1.05, 0.55, 0.65,
                 0.35, 4.0, 1.5, 0.75, 0.5, 0.62, 0.58, 0.41, 7.0, 0.52, 0.48, 0.66]),
    # the proposal falls below dt_min: hit counted, ratio forgotten (the next call starts from none), accepted with error > 1
    "dt_min": (0.0, 1.0, 0.1, 0.05, [1.0], [0.5, 50.0, 0.4, 5.0, 0.6, 0.7, 1e6, 0.5, 0.5, 0.3, 0.5, 0.6, 0.5, 0.4, 0.5, 0.5]),
    # the proposal EQUALS dt_min (0.25 * 0.2 is the double 0.05): not a hit, the ratio survives, and the attempt is accepted
    "dt_min_equal": (0.0, 2.0, 0.25, 0.05, [2.0], [1.0, 1e6, 0.3, 0.3, 1.2, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),
    # a step that would pass t_end is clamped to it; then the calls after completion
    "t_end": (0.0, 0.3, 0.2, 0.0, [0.3], [0.5, 2.0, 0.5, 0.5, 0.7, 2.0, 0.5]),
    # output times: equal to t0; landed on exactly (0.1); passed (0.15); three inside one step; two equal; the last one
    "outputs": (0.0, 0.9, 0.1, 0.0, [0.0, 0.1, 0.15, 0.31, 0.32, 0.33, 0.5, 0.5, 0.9],
                [0.95, 0.96, 0.97, 0.95, 0.96, 0.95, 0.97, 0.95, 0.96, 0.95, 0.5, 0.5, 0.5]),
    # the same on a grid that does not start at 0, with steps that grow
    "outputs_offset": (0.25, 1.5, 0.07, 0.03, [0.26, 0.27, 0.27, 0.9, 1.5],
                       [0.5, 0.2, 3.0, 30.0, 0.9, 0.4, 0.3, 1.7, 0.2, 0.1, 0.3, 0.2, 0.1, 0.2, 0.3, 0.1, 0.2, 0.2]),
    # times on both sides of zero: the half widths are NOT exact differences in float32 there (no Sterbenz lemma), so the
    # double differences of the table differ from differences formed in T
    "straddling_zero": (-0.1, 1.0, 0.3, 0.0, [0.05, 1.0], [0.5, 0.6, 2.0, 0.5, 0.4, 0.5, 0.5, 0.5]),
    # a NaN error estimate in the middle
    "nan": (0.0, 1.0, 0.1, 0.0, [1.0], [0.5, NAN, 0.5, 2.0, 0.4]),
}

pow_records = []        # (error, previous step size, previous ratio, device's step size, model's step size)


def ulps_apart(a, b):
    """Distance of two finite doubles of one sign in units of the last place."""
    ia, ib = (int(np.array(x, dtype=np.float64).view(np.int64)) for x in (a, b))
    return abs(ia - ib)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


CTL_NAMES = {getattr(N, k): k for k in dir(N) if k.startswith("CTL_") and k != "CTL_SIZE"}


def assert_tables_equal(got_ctl, got_scal, got_log, model, where, skip=()):
    """Every word of ctl, scal and the accept log as bit patterns (the one NaN the tables hold, 'no previous ratio', as NaN)."""
    for w in range(N.CTL_SIZE):
        if w in skip:
            continue
        g, m = got_ctl[w], model.ctl[w]
        same = (g != g and m != m) if w == N.CTL_PREV_ERROR_RATIO and (g != g or m != m) else _bits(g) == _bits(m)
        assert same, f"{where}: ctl[{CTL_NAMES.get(w, w)}] device {g!r} ({float(g).hex()}) model {m!r} ({float(m).hex()})"
    gb, mb = _bits(got_scal), _bits(model.scal)
    for w in np.nonzero(gb != mb)[0]:
        sub, word = divmod(int(w), N.SUB_STRIDE)
        raise AssertionError(f"{where}: scal[{w}] (sub-step {sub} word {word}; W0 = {N.SCAL_W0}) device {got_scal[w]!r} "
                             f"model {model.scal[w]!r}")
    n = len(got_log)
    assert _bits(got_log).tolist() == _bits(model.accept_log[:n]).tolist(), f"{where}: accept log"


class Driver:
    """`adaptive.DeviceController` with its state read back after every call, next to a model seeded from it."""
    LOG_WORDS = 96

    def __init__(self, dtype, fracs, seq, log_capacity=None):
        from torchsde_amd import adaptive
        self.t0, self.t_end, self.dt, self.dt_min, self.outs, self.errors = seq
        self.dtype, self.fracs = dtype, fracs
        # (the output times of a solve are values of its dtype: adaptive.integrate hands over ts_host as float64)
        self.outs = [float(NP[dtype](t)) for t in self.outs]
        self.ctrl = adaptive.DeviceController(DEV, dtype, fracs)
        self.model = M.ControllerModel(NP[dtype], fracs, log_capacity=log_capacity or self.ctrl.LOG_CAPACITY)
        self.err = torch.zeros(1, dtype=torch.float64, device=DEV)
        self.ys = torch.full((len(self.outs), 5), -777.0, dtype=dtype, device=DEV)
        self.log_capacity = log_capacity
        self.after_nan = False
        if log_capacity is not None:
            self.log = torch.full((16,), -5.0, dtype=torch.float64, device=DEV)
            self.model.accept_log = np.full(16, -5.0)

    def state(self):
        torch.cuda.synchronize()
        log = self.log if self.log_capacity is not None else self.ctrl.accept_log[:self.LOG_WORDS]
        return self.ctrl.ctl.cpu().numpy().copy(), self.ctrl.scal.cpu().numpy().copy(), log.cpu().numpy().copy()

    def begin(self):
        t0, t_end = float(NP[self.dtype](self.t0)), float(NP[self.dtype](self.t_end))
        self.ctrl.load(t0, t_end, self.dt, self.dt_min)
        self.ctrl.accept_log.zero_()
        self.ctrl.begin(self.outs, self.ys)
        self.model.load(t0, t_end, self.dt, self.dt_min)
        self.model.begin(self.outs)
        ctl, scal, log = self.state()
        assert_tables_equal(ctl, scal, log, self.model, "begin")
        return ctl, scal, log

    def launch_control(self, err):
        self.err.fill_(err)
        if self.log_capacity is None:
            self.ctrl.control(self.err)
            return
        c = self.ctrl
        code = N.load().tsde_adaptive_control_outputs(c.ctl.data_ptr(), c.scal.data_ptr(), self.err.data_ptr(),
                                                      c.out_times.data_ptr(), self.log.data_ptr(), self.log_capacity, c._fracs,
                                                      c.n_fracs, c._dt_code, c._stream())
        N.check(code, "tsde_adaptive_control_outputs")

    def control(self, err, where):
        """One call on the device and the same call on the model seeded from the device's state before it. Returns
        (ctl before, ctl after, scal after, log after, kind) with kind in {"inert", "nan", "after_nan", "clamped", "pow"}."""
        ctl0, scal0, log0 = self.state()
        self.launch_control(err)
        ctl1, scal1, log1 = self.state()
        model = self.model
        if self.after_nan:              # nothing is asserted about the numeric state after a NaN error
            return ctl0, ctl1, scal1, log1, "after_nan"
        model.seed(ctl0, scal0)
        model.accept_log[:len(log0)] = log0
        if ctl0[N.CTL_ACTIVE] == 0.0:
            model.control(err)
            assert_tables_equal(ctl1, scal1, log1, model, where + " (inert)")
            return ctl0, ctl1, scal1, log1, "inert"
        if err != err:
            with pytest.raises(AssertionError, match="Found nans in the error estimate"):
                model.control(err)
            self.after_nan = True
            return ctl0, ctl1, scal1, log1, "nan"
        # (a) the proposal
        step_m, ratio_m, hit_m = model.propose(err)
        step_d, ratio_d = float(ctl1[N.CTL_STEP_SIZE]), float(ctl1[N.CTL_PREV_ERROR_RATIO])
        clamped = hit_m or M.factor_is_clamped(err, model.prev_error_ratio)
        if clamped:
            assert step_d == step_m, f"{where}: clamped step size: device {step_d.hex()} model {step_m.hex()}"
        else:
            pow_records.append((err, float(ctl0[N.CTL_STEP_SIZE]), model.prev_error_ratio, step_d, step_m))
            assert ulps_apart(step_d, step_m) <= POW_ULPS_BOUND, \
                f"{where}: step size device {step_d.hex()} model {step_m.hex()}: {ulps_apart(step_d, step_m)} ulps"
        # the ratio is 0.9 / err (one IEEE division), the previous one, or none: no `pow` in it
        assert (ratio_m is None and ratio_d != ratio_d) or ratio_d == ratio_m, f"{where}: ratio {ratio_d!r} vs {ratio_m!r}"
        # (b) everything else, given the device's own step size
        model.control(err, proposal=(step_d, ratio_m, hit_m))
        assert_tables_equal(ctl1, scal1, log1, model, where)
        return ctl0, ctl1, scal1, log1, "clamped" if clamped else "pow"


def run_sequence(dtype, fracs, name, log_capacity=None):
    drv = Driver(dtype, fracs, SEQUENCES[name], log_capacity)
    trace = [("begin", None) + drv.begin()]
    for k, err in enumerate(drv.errors):
        ctl0, ctl1, scal1, log1, kind = drv.control(err, f"{name}[{k}] err={err!r}")
        trace.append((kind, err, ctl1, scal1, log1, ctl0))
    return drv, trace


def _factor(entry):
    return entry[2][N.CTL_STEP_SIZE] / entry[5][N.CTL_STEP_SIZE]


@pytest.mark.parametrize("fracs", STAGE_FRACS, ids=lambda f: "fracs" + "-".join(str(x) for x in f))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_controller_regimes(dtype, fracs):
    _, trace = run_sequence(dtype, fracs, "regimes")
    calls = trace[1:]
    errs = SEQUENCES["regimes"][5]
    accept = [c[3][N.SCAL_ACCEPT] == 1 for c in calls]
    ratio = [c[2][N.CTL_PREV_ERROR_RATIO] for c in calls]
    assert trace[0][2][N.CTL_PREV_ERROR_RATIO] != trace[0][2][N.CTL_PREV_ERROR_RATIO]       # none before the first call
    assert accept[0] and _factor(calls[0]) == 1.4 and ratio[0] == 0.9 / 1e-3                  # growth capped
    assert accept[1] and _factor(calls[1]) == 1.4                                             # 1e-7
    assert accept[4] and not accept[5]                                                        # exactly 1 / its upper neighbour
    assert ratio[4] == 0.9 and ratio[5] == 0.9
    assert not accept[6] and calls[6][2][N.CTL_STEP_SIZE] == calls[6][5][N.CTL_STEP_SIZE] * 0.2   # 1e6: clamped at 0.2
    assert (not accept[7]) and (not accept[8]) and accept[9]                                  # reject, reject, accept
    assert ratio[7] == ratio[8] == 0.9 and ratio[9] == 0.9 / 0.7                              # survives rejections, then replaced
    kinds = [c[0] for c in calls]
    assert kinds.count("pow") >= 15 and kinds.count("clamped") >= 5
    assert any(c[0] == "pow" and e > 1 for c, e in zip(calls, errs)) and any(c[0] == "pow" and e <= 1 for c, e in zip(calls, errs))
    last = calls[-1][2]
    assert last[N.CTL_ATTEMPTS] == len(errs) and last[N.CTL_ACCEPTED] == sum(accept) and last[N.CTL_DT_MIN_HITS] == 0
    assert last[N.CTL_NAN_SEEN] == 0 and last[N.CTL_ACTIVE] == 1


@pytest.mark.parametrize("fracs", STAGE_FRACS[:2] + STAGE_FRACS[-1:], ids=lambda f: "fracs" + "-".join(str(x) for x in f))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_controller_dt_min(dtype, fracs):
    _, trace = run_sequence(dtype, fracs, "dt_min")
    calls = trace[1:]
    hits = [c[2][N.CTL_DT_MIN_HITS] for c in calls]
    # 50.0: proposal 0.2 * step < dt_min -> step = dt_min, hit, ratio none, accepted although the error exceeds 1
    assert hits[0] == 0 and hits[1] == 1 and calls[1][2][N.CTL_STEP_SIZE] == 0.05
    assert calls[1][2][N.CTL_PREV_ERROR_RATIO] != calls[1][2][N.CTL_PREV_ERROR_RATIO] and calls[1][3][N.SCAL_ACCEPT] == 1
    # ... and the next call treats the ratio as none: its factor is that of a first call, (0.9 / 0.4) ** (1 / 4.5) alone
    assert calls[2][2][N.CTL_PREV_ERROR_RATIO] == 0.9 / 0.4
    first_call_factor = (0.9 / 0.4) ** (1 / 4.5)
    assert abs(_factor(calls[2]) / first_call_factor - 1) < 1e-14
    assert hits[3] == 2 and hits[6] == 3 and hits[-1] == 3
    # the equal case: 0.25 * 0.2 == dt_min is NOT below it
    _, trace = run_sequence(dtype, fracs, "dt_min_equal")
    calls = trace[1:]
    assert calls[0][2][N.CTL_STEP_SIZE] == 0.25 and calls[0][2][N.CTL_PREV_ERROR_RATIO] == 0.9
    assert calls[1][2][N.CTL_STEP_SIZE] == 0.05 and calls[1][2][N.CTL_DT_MIN_HITS] == 0
    assert calls[1][2][N.CTL_PREV_ERROR_RATIO] == 0.9 and calls[1][3][N.SCAL_ACCEPT] == 1
    assert all(c[2][N.CTL_DT_MIN_HITS] == 0 for c in calls)


@pytest.mark.parametrize("fracs", STAGE_FRACS[:2] + STAGE_FRACS[-1:], ids=lambda f: "fracs" + "-".join(str(x) for x in f))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_controller_clamps_to_t_end_and_goes_inert(dtype, fracs):
    T = NP[dtype]
    drv, trace = run_sequence(dtype, fracs, "t_end")
    t_end = float(T(0.3))
    n = len(fracs)
    after_first = trace[1]
    assert after_first[3][N.SCAL_ACCEPT] == 1 and after_first[2][N.CTL_CURR_T] == float(T(0.0) + T(0.2))
    # the second attempt would pass t_end: next_t == t_end bit for bit, and the second half's end equals t_end
    scal = after_first[3]
    assert _bits(scal[N.SUB_TIMES + n]) == _bits(T(t_end)) and _bits(scal[2 * N.SUB_STRIDE + N.SUB_TIMES + n]) == _bits(T(t_end))
    assert after_first[2][N.CTL_BOUNDS_B + 1] == t_end
    assert scal[N.SUB_DT] == T(t_end) - T(after_first[2][N.CTL_CURR_T])
    # rejected once (the clamp holds with the smaller step or not -- the model decides), then accepted to t_end
    done = [k for k, c in enumerate(trace[1:]) if c[2][N.CTL_ACTIVE] == 0]
    assert done and done[0] <= 3
    k = done[0] + 1
    final = trace[k]
    assert final[2][N.CTL_CURR_T] == t_end and final[2][N.CTL_OUT_IDX] == final[2][N.CTL_N_OUT] == 1
    assert final[2][N.CTL_EMIT_COUNT] == 1 and final[3][N.SCAL_ACCEPT] == 1
    assert final[3][N.SCAL_W0] == 0 and final[3][N.SCAL_W1] == 1          # the state sits on the output time
    # further calls: inert -- bit-identical tables but ACCEPT == 0 and EMIT_COUNT == 0, attempts not counted
    assert len(trace) - 1 - k >= 3
    for later in trace[k + 1:]:
        assert later[0] == "inert"
        ctl, scal = later[2].copy(), later[3].copy()
        assert ctl[N.CTL_EMIT_COUNT] == 0 and scal[N.SCAL_ACCEPT] == 0
        ctl[N.CTL_EMIT_COUNT], scal[N.SCAL_ACCEPT] = final[2][N.CTL_EMIT_COUNT], final[3][N.SCAL_ACCEPT]
        assert _bits(ctl).tolist() == _bits(final[2]).tolist() and _bits(scal).tolist() == _bits(final[3]).tolist()
        assert _bits(later[4]).tolist() == _bits(final[4]).tolist()


@pytest.mark.parametrize("fracs", STAGE_FRACS[:1] + STAGE_FRACS[-1:], ids=lambda f: "fracs" + "-".join(str(x) for x in f))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_controller_times_straddling_zero(dtype, fracs):
    T = NP[dtype]
    _, trace = run_sequence(dtype, fracs, "straddling_zero")
    ctl = trace[0][2]
    curr, mid, nxt = T(-0.1), T(0.5) * (T(-0.1) + (T(-0.1) + T(0.3))), T(-0.1) + T(0.3)
    assert ctl[N.CTL_BOUNDS_A:N.CTL_BOUNDS_A + 2].tolist() == [float(curr), float(mid)]
    assert ctl[N.CTL_WIDTHS:N.CTL_WIDTHS + 2].tolist() == [float(mid) - float(curr), float(nxt) - float(mid)]
    if dtype == torch.float32:      # (what makes the case worth having)
        assert float(nxt) - float(mid) != float(T(nxt - mid))
    assert trace[-1][2][N.CTL_ACTIVE] == 0 and trace[-1][2][N.CTL_OUT_IDX] == 2


@pytest.mark.parametrize("name", ["outputs", "outputs_offset"])
@pytest.mark.parametrize("fracs", STAGE_FRACS[:1] + STAGE_FRACS[-1:], ids=lambda f: "fracs" + "-".join(str(x) for x in f))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_controller_walks_the_output_times_and_emit_writes_their_rows(dtype, fracs, name):
    """The output list on the device, and after every call the emit kernel on a 5-element state: the rows the model says,
    every other row untouched."""
    T = NP[dtype]
    drv = Driver(dtype, fracs, SEQUENCES[name])
    rng = np.random.default_rng(3)
    prev_np, curr_np = rng.standard_normal(5).astype(T), rng.standard_normal(5).astype(T)
    prev_y, curr_y = torch.from_numpy(prev_np).to(DEV), torch.from_numpy(curr_np).to(DEV)
    want_ys = np.full((len(drv.outs), 5), -777.0, dtype=T)
    counts, emitted_at = [], {}

    def emit_and_compare(ctl, where):
        drv.ctrl.emit(prev_y, curr_y)
        rows = drv.model.emit_rows(prev_np, curr_np)
        assert sorted(rows) == list(range(int(ctl[N.CTL_EMIT_FIRST]), int(ctl[N.CTL_EMIT_FIRST] + ctl[N.CTL_EMIT_COUNT])))
        for j, row in rows.items():
            want_ys[j] = row
            emitted_at[j] = (ctl[N.CTL_PREV_T], ctl[N.CTL_CURR_T])
        torch.cuda.synchronize()
        assert _bits(drv.ys.cpu().numpy()).tolist() == _bits(want_ys).tolist(), where
        counts.append(int(ctl[N.CTL_EMIT_COUNT]))

    ctl, _, _ = drv.begin()
    emit_and_compare(ctl, "begin")
    for k, err in enumerate(drv.errors):
        _, ctl, _, _, _ = drv.control(err, f"{name}[{k}] err={err!r}")
        emit_and_compare(ctl, f"{name}[{k}]")
    assert ctl[N.CTL_OUT_IDX] == ctl[N.CTL_N_OUT] == len(drv.outs) and ctl[N.CTL_ACTIVE] == 0
    assert sum(counts) == len(drv.outs) and counts[-1] == 0 and not (want_ys == -777.0).any()
    if name == "outputs":
        assert counts[0] == 1                                   # the output time equal to t0: marked by begin ...
        assert _bits(want_ys[0]).tolist() == _bits(curr_np).tolist()      # ... weights 0 and 1
        assert counts[1] == 1 and emitted_at[1][1] == float(T(0.1))        # landed on exactly
        assert emitted_at[2][0] < drv.outs[2] < emitted_at[2][1]           # passed
        assert 3 in counts and emitted_at[3] == emitted_at[4] == emitted_at[5]      # three inside one step
        assert emitted_at[6] == emitted_at[7]                              # two equal output times
    else:
        assert counts[0] == 0 and emitted_at[1] == emitted_at[2]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_accept_log_shorter_than_the_accepted_steps(dtype):
    """`tsde_adaptive_control_outputs` with log_capacity = 3 on a 16-double buffer: six doubles written, ten keep the sentinel,
    ACCEPTED goes on counting."""
    drv, trace = run_sequence(dtype, (0, 0.5), "outputs", log_capacity=3)
    final_ctl, log = trace[-1][2], trace[-1][4]
    assert final_ctl[N.CTL_ACCEPTED] >= 9
    assert len(log) == 16 and (log[6:] == -5.0).all() and not (log[:6] == -5.0).any()
    accepted = [c for c in trace[1:] if c[3][N.SCAL_ACCEPT] == 1][:3]
    assert log[:6].tolist() == [x for c in accepted for x in (c[2][N.CTL_PREV_T], c[2][N.CTL_CURR_T])]
    assert float(drv.ctrl.accept_log.abs().max()) == 0.0        # (the controller's own log was not the one handed over)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_nan_error_is_latched_and_counted(dtype):
    _, trace = run_sequence(dtype, (0,), "nan")
    calls = trace[1:]
    assert calls[0][2][N.CTL_NAN_SEEN] == 0 and calls[0][2][N.CTL_ATTEMPTS] == 1
    assert calls[1][0] == "nan" and calls[1][2][N.CTL_NAN_SEEN] == 1 and calls[1][2][N.CTL_ATTEMPTS] == 2
    for later in calls[2:]:
        assert later[2][N.CTL_NAN_SEEN] == 1            # (nothing is asserted about the numeric state after a NaN)
    assert calls[-1][2][N.CTL_ATTEMPTS] == len(calls)


class _Overflowing(torch.nn.Module):
    noise_type = "diagonal"
    sde_type = "ito"

    def f(self, t, y):
        return y * y

    def g(self, t, y):
        return y * y * y


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("device_adaptive", [True, False])
def test_overflowing_solve_raises_the_references_assertion(device_adaptive):
    """adaptive_stepping.py:66-68 through both control modes: on the device the NaN is latched in ctl[NAN_SEEN] and raised at
    the host's next read (adaptive.py), on the host by `solvers._error_estimate`."""
    import torchsde_amd
    y0 = torch.full((8, 3), 1e15, dtype=torch.float32, device=DEV)
    ts = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float32, device=DEV)
    bm = torchsde_amd.BrownianInterval(0.0, 1.0, size=(8, 3), dtype=torch.float32, device=DEV, entropy=7)
    with torch.no_grad(), pytest.raises(AssertionError, match="Found nans in the error estimate"):
        torchsde_amd.sdeint(_Overflowing(), y0, ts, bm=bm, method="euler", dt=0.1, adaptive=True,
                            options={"device_adaptive": device_adaptive})


def measure_pow_ulps():
    """Every unclamped proposal of every sequence: (records, worst distance device - CPython, worst device - mpmath, worst
    CPython - mpmath), the last two None without mpmath. The records do not depend on the dtype or the stage fractions."""
    del pow_records[:]
    for name in SEQUENCES:
        run_sequence(torch.float64, (0,), name)
    records = list(pow_records)
    worst = max(ulps_apart(d, m) for _, _, _, d, m in records)
    try:
        import mpmath
    except ImportError:
        return records, worst, None, None
    worst_dev = worst_py = 0.0
    with mpmath.workprec(200):          # (more than 50 digits)
        for err, step, ratio, d, m in records:
            er = mpmath.mpf(0.9 / err)
            pf, ifac = (0, 1 / 1.5) if err > 1 else (0.13, 1 / 4.5)
            prev = er if ratio is None else mpmath.mpf(ratio)
            exact = mpmath.mpf(step) * mpmath.power(er, mpmath.mpf(ifac)) * mpmath.power(er / prev, mpmath.mpf(pf))
            ulp = mpmath.mpf(float(np.spacing(float(exact))))
            worst_dev = max(worst_dev, float(abs(mpmath.mpf(d) - exact) / ulp))
            worst_py = max(worst_py, float(abs(mpmath.mpf(m) - exact) / ulp))
    return records, worst, worst_dev, worst_py


def test_pow_distance_is_what_the_bound_was_derived_from():
    """The bound asserted per call is max(4, 2 x measured): the measurement itself, repeated (it printed
    profiles/adaptive_controller_pow_ulps.txt), must not exceed what it was when the bound was set."""
    records, worst, worst_dev, worst_py = measure_pow_ulps()
    print(f"unclamped proposals {len(records)}: device vs CPython {worst} ulps, device vs mpmath {worst_dev}, "
          f"CPython vs mpmath {worst_py}")
    assert len(records) >= 40
    assert worst <= POW_ULPS_BOUND
    if worst_dev is not None:
        assert worst_dev <= POW_ULPS_BOUND


# ------------------------------------------------------------------------------------------------------------------------------
# 3. The elementwise kernels of an attempt
# ------------------------------------------------------------------------------------------------------------------------------
GUARD = 64                      # elements on each side (a multiple of 4: the aligned view starts on a 16-byte boundary)
GUARD_VALUE = -1234.5
# n: 1, 3, 4, 1023, 4100 (scalar tails, one and several blocks; 4100: consecutive tiles on 5 blocks), then the smallest n of
# each further branch of launch_elementwise (tsde_common.h): 7172 = the XCD-matched tiling (8 blocks of 16-byte groups),
# 4194304 = two groups per thread (nq >= 2 * 256 * 2048). The streaming branch starts at 96 MiB per buffer: left out.
SIZES = [1, 3, 4, 1023, 4100, 7172, 4 * 2 * 256 * 2048]
SHIFTS = [0, 1]                 # the view shifted by one element is not 16-byte aligned: the scalar path
_inputs = {}


def _special_values(T):
    tiny = np.finfo(T).tiny
    return np.array([-0.0, tiny / 4, -tiny / 2, np.inf, -np.inf, np.nan, np.finfo(T).max, -np.finfo(T).max, np.finfo(T).eps,
                     1.0], dtype=T)


def _input(n, T, which, specials):
    """A fixed-seed array (cached, never modified). `specials`: -0.0, subnormals, +-inf, NaN, the largest finite values sown in."""
    key = (n, T, which, specials)
    if key not in _inputs:
        rng = np.random.default_rng([n % 65521, which, 11])
        x = rng.standard_normal(n).astype(T)
        if specials:
            sv = np.roll(_special_values(T), which)
            if n >= 2 * len(sv):
                x[np.arange(len(sv)) * (n // len(sv)) + which % 3] = sv
            else:
                x[:] = np.resize(sv, n)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


class Guarded:
    """A buffer of n elements inside a larger allocation with sentinel guards on both sides."""

    def __init__(self, values, dtype, shift, n=None):
        n = len(values) if values is not None else n
        self.whole = torch.full((GUARD + shift + n + GUARD,), GUARD_VALUE, dtype=dtype, device=DEV)
        self.lo = GUARD + shift
        self.view = self.whole[self.lo:self.lo + n]
        if values is not None:
            self.view.copy_(torch.from_numpy(np.array(values)).to(DEV))
        assert (self.view.data_ptr() % 16 == 0) == (shift == 0)

    def guards_intact(self):
        n = self.view.numel()
        return bool((self.whole[:self.lo] == GUARD_VALUE).all() and (self.whole[self.lo + n:] == GUARD_VALUE).all())


def same_bits(got, want_np, nan_as_class=False):
    """Equal as integer bit patterns (on the device: the large sizes stay there). `nan_as_class`: where the expected value is
    the RESULT of arithmetic and a NaN, any NaN will do (its sign and payload are the processor's choice)."""
    want = torch.from_numpy(np.array(want_np)).to(got.device)
    gi, wi = got.contiguous().view(INT[got.dtype]), want.view(INT[want.dtype])
    if not nan_as_class:
        return torch.equal(gi, wi)
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(gi[~nan], wi[~nan])


CASES_NS = [(n, s) for n in SIZES for s in SHIFTS]


@pytest.mark.parametrize("accept", [0, 1])
@pytest.mark.parametrize("n,shift", CASES_NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_commit(dtype, n, shift, accept):
    T = NP[dtype]
    prev_np, curr_np, next_np = _input(n, T, 0, False), _input(n, T, 1, True), _input(n, T, 2, True)
    prev_y, curr_y, y_next = (Guarded(x, dtype, shift) for x in (prev_np, curr_np, next_np))
    scal = torch.zeros(N.SCAL_SIZE, dtype=dtype, device=DEV)
    scal[N.SCAL_ACCEPT] = accept
    model = M.ControllerModel(T, (0,))
    model.scal[N.SCAL_ACCEPT] = accept
    want_prev, want_curr = prev_np.copy(), curr_np.copy()
    model.commit(want_prev, want_curr, next_np)
    code = N.load().tsde_adaptive_commit(prev_y.view.data_ptr(), curr_y.view.data_ptr(), y_next.view.data_ptr(), n,
                                         scal.data_ptr(), N.dtype_code(dtype), N.stream_ptr())
    N.check(code, "tsde_adaptive_commit")
    torch.cuda.synchronize()
    if accept:
        assert _bits(want_prev).tolist() == _bits(curr_np).tolist() and _bits(want_curr).tolist() == _bits(next_np).tolist()
    else:
        assert _bits(want_prev).tolist() == _bits(prev_np).tolist() and _bits(want_curr).tolist() == _bits(curr_np).tolist()
    assert same_bits(prev_y.view, want_prev) and same_bits(curr_y.view, want_curr) and same_bits(y_next.view, next_np)
    assert prev_y.guards_intact() and curr_y.guards_intact() and y_next.guards_intact()


ROWS = 5
EMIT_TIMES = [0.1, 0.25, 0.26, 0.3, 0.7]        # the output times of the rows
# (prev_t, curr_t, first, count, special values in the data)
EMIT_CASES = {
    "three_rows_after_the_first": (0.2, 0.3125, 1, 3, True),
    "one_row": (0.0, 0.1, 0, 1, True),
    "last_row_inside": (0.55, 0.9, 4, 1, True),
    "nothing": (0.2, 0.3125, 1, 0, True),
    "state_has_not_moved": (0.25, 0.25, 1, 1, False),
}


# (the largest size runs the three-row and the empty case only)
EMIT_PARAMS = [(n, s, c) for n, s in CASES_NS for c in EMIT_CASES
               if n < 100000 or c in ("three_rows_after_the_first", "nothing")]


@pytest.mark.parametrize("n,shift,case", EMIT_PARAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_emit(dtype, n, shift, case):
    T = NP[dtype]
    prev_t, curr_t, first, count, specials = EMIT_CASES[case]
    prev_np, curr_np = _input(n, T, 3, False), _input(n, T, 4, specials)
    prev_y, curr_y = Guarded(prev_np, dtype, shift), Guarded(curr_np, dtype, shift)
    # ys: ROWS rows of n elements in the MIDDLE of a larger tensor (one row of sentinel before, one after)
    big = torch.full(((ROWS + 2) * n,), -777.0, dtype=dtype, device=DEV)
    ys = big[n:(ROWS + 1) * n]
    slot = torch.tensor([ys.data_ptr()], dtype=torch.int64, device=DEV)
    out_times = torch.tensor([float(T(t)) for t in EMIT_TIMES], dtype=torch.float64, device=DEV)
    model = M.ControllerModel(T, (0,))
    model.out_times = out_times.cpu().numpy()
    model.ctl[N.CTL_PREV_T], model.ctl[N.CTL_CURR_T] = float(T(prev_t)), float(T(curr_t))
    model.ctl[N.CTL_EMIT_FIRST], model.ctl[N.CTL_EMIT_COUNT] = first, count
    ctl = torch.from_numpy(model.ctl.copy()).to(DEV)
    code = N.load().tsde_adaptive_emit(slot.data_ptr(), prev_y.view.data_ptr(), curr_y.view.data_ptr(), n, ctl.data_ptr(),
                                       out_times.data_ptr(), N.dtype_code(dtype), N.stream_ptr())
    N.check(code, "tsde_adaptive_emit")
    torch.cuda.synchronize()
    rows = model.emit_rows(prev_np, curr_np)
    assert sorted(rows) == list(range(first, first + count))
    for j in range(ROWS):
        row = ys[j * n:(j + 1) * n]
        if j in rows:
            assert same_bits(row, rows[j], nan_as_class=True), (case, j)
        else:
            assert bool((row == -777.0).all()), (case, j)
    if case == "state_has_not_moved":
        assert _bits(rows[first]).tolist() == _bits(curr_np).tolist()          # curr_y itself
    assert bool((big[:n] == -777.0).all() and (big[(ROWS + 1) * n:] == -777.0).all())
    assert same_bits(prev_y.view, prev_np) and same_bits(curr_y.view, curr_np)
    assert prev_y.guards_intact() and curr_y.guards_intact()


@pytest.mark.parametrize("with_U", [True, False], ids=["U", "noU"])
@pytest.mark.parametrize("n,shift", CASES_NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_merge_halves(dtype, n, shift, with_U):
    T = NP[dtype]
    ha, hb = float(T(0.1375)) - float(T(0.1)), float(T(0.2)) - float(T(0.1375))       # widths as the controller forms them
    Wa_np, Ha_np, Wb_np, Hb_np = (_input(n, T, 5 + k, k == 0) for k in range(4))
    ins = [Guarded(x, dtype, shift) for x in (Wa_np, Ha_np, Wb_np, Hb_np)]
    ctl = torch.zeros(N.CTL_SIZE, dtype=torch.float64, device=DEV)
    ctl[N.CTL_WIDTHS], ctl[N.CTL_WIDTHS + 1] = ha, hb
    want_W, want_U = M.merge_halves(Wa_np, Ha_np, Wb_np, Hb_np, ha, hb, want_U=with_U)
    results = []
    for source in ("device", "host"):
        W, U = Guarded(None, dtype, shift, n), Guarded(None, dtype, shift, n)
        code = N.load().tsde_merge_halves(
            W.view.data_ptr(), U.view.data_ptr() if with_U else None, ins[0].view.data_ptr(),
            ins[1].view.data_ptr() if with_U else None, ins[2].view.data_ptr(), ins[3].view.data_ptr() if with_U else None, n,
            ctl.data_ptr() if source == "device" else None, 0.0 if source == "device" else ha,
            0.0 if source == "device" else hb, N.dtype_code(dtype), N.stream_ptr())
        N.check(code, "tsde_merge_halves")
        torch.cuda.synchronize()
        assert same_bits(W.view, want_W, nan_as_class=True), source
        if with_U:
            assert same_bits(U.view, want_U, nan_as_class=True), source
        else:
            assert bool((U.view == GUARD_VALUE).all())
        assert W.guards_intact() and U.guards_intact()
        results.append((W.view.clone(), U.view.clone()))
    for a, b in zip(*results):          # the two width sources: the same bits
        assert torch.equal(a.view(INT[dtype]), b.view(INT[dtype]))
    for g, x in zip(ins, (Wa_np, Ha_np, Wb_np, Hb_np)):
        assert same_bits(g.view, x) and g.guards_intact()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. tsde_brownian_query_dev
# ------------------------------------------------------------------------------------------------------------------------------
UNEVEN = np.array([0.0, 0.11, 0.35, 0.36, 0.8, 1.0])


def _query_cases(e):
    w = np.diff(e)
    nonempty = {
        "inside_one_cell": (e[1] + 0.2 * w[1], e[1] + 0.7 * w[1]),
        "one_whole_cell": (e[1], e[2]),
        "three_whole_cells": (e[1], e[4]),
        "four_cells_interior_ends": (e[0] + 0.3 * w[0], e[3] + 0.6 * w[3]),
        "clamped_both_sides": (e[0] - 0.5, e[-1] + 0.5),
        "b_on_first_interior_edge": (e[0] + 0.4 * w[0], e[1]),
        "a_on_last_interior_edge": (e[-2], e[-2] + 0.5 * w[-1]),
    }
    empty = {"a_equals_b": (0.3, 0.3), "a_above_b": (0.6, 0.2), "both_beyond_the_end": (e[-1] + 0.2, e[-1] + 0.7)}
    return nonempty, empty


@pytest.mark.parametrize("row_offset", [0, 3])
@pytest.mark.parametrize("n", [1, 5, 4096])
@pytest.mark.parametrize("grid", ["dt_hint", "uneven"])
@pytest.mark.parametrize("levy", ["none", "space-time"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_query_dev(dtype, levy, grid, n, row_offset):
    import torchsde_amd
    from torchsde_amd import adaptive
    have_h = levy != "none"
    entropy = 4242
    bm = torchsde_amd.BrownianInterval(0.0, 1.0, size=(n,), dtype=dtype, device=DEV, entropy=entropy,
                                       dt=0.125 if grid == "dt_hint" else None, levy_area_approximation=levy,
                                       row_offset=row_offset)
    if grid == "uneven":
        assert bm.adopt_grid(UNEVEN)
    edges = bm._edges.copy()
    assert len(edges) >= 6 and bm._elem0 == row_offset and (grid == "dt_hint" or len(set(np.round(np.diff(edges), 9))) > 2)
    tol = 3e-5 if dtype == torch.float32 else 1e-11       # tests/test_gpu_parity.py: test_query_matches_oracle
    ab = torch.zeros(2, dtype=torch.float64, device=DEV)
    nonempty, empty = _query_cases(edges)

    def query(a, b):
        ab.copy_(torch.tensor([a, b], dtype=torch.float64))
        outs = [torch.full((n,), -9.0, dtype=dtype, device=DEV) for _ in range(3)]
        adaptive.query_dev(bm, ab.data_ptr(), outs[0], outs[1] if have_h else None, outs[2] if have_h else None)
        torch.cuda.synchronize()
        return outs

    for name, (a, b) in nonempty.items():
        W, U, H = query(float(a), float(b))
        a_c, b_c = min(max(float(a), edges[0]), edges[-1]), min(max(float(b), edges[0]), edges[-1])
        H_host = torch.full((n,), -9.0, dtype=dtype, device=DEV)
        W_host, U_host = bm.increment(a_c, b_c, want_U=have_h, out_H=H_host if have_h else None)
        assert torch.equal(W, W_host), name
        Wr, Ur, Hr = counter.query(n, entropy, edges, a_c, b_c, dtype=NP[dtype], elem0=row_offset, have_h=have_h)
        assert np.abs(W.cpu().numpy() - Wr).max() <= tol, name
        if have_h:
            assert torch.equal(U, U_host) and torch.equal(H, H_host), name
            assert np.abs(U.cpu().numpy() - Ur).max() <= tol and np.abs(H.cpu().numpy() - Hr).max() <= tol, name
        else:
            assert bool((U == -9.0).all() and (H == -9.0).all())
    for name, (a, b) in empty.items():
        W, U, H = query(float(a), float(b))
        for out in (W, U, H) if have_h else (W,):
            assert not bool(out.view(INT[dtype]).any()), name          # exactly +0 in every element


# ------------------------------------------------------------------------------------------------------------------------------
# 5. tsde_error_norm
# ------------------------------------------------------------------------------------------------------------------------------
N_ALL_PARTIALS = 4 * 256 * 1024 * 2 + 4         # the vector path with all 1024 partials and a grid-stride tail
EPS = 1e-7
_norm_refs = {}


def _norm_inputs(kind, n, T):
    rng = np.random.default_rng([n % 65521, 17])
    a = rng.standard_normal(n).astype(T)
    b = (a + T(1e-3) * rng.standard_normal(n).astype(T)).astype(T)
    rtol, atol = 1e-3, 1e-4
    if kind == "zero_tolerances_unequal":
        rtol = atol = 0.0
    elif kind == "zero_tolerances_equal":
        rtol = atol = 0.0
        b = a.copy()
    elif kind == "opposite_signs":
        b = (-T(1.5) * a).astype(T)                  # |a| < |b|, signs opposite
    elif kind == "magnitudes":
        scale = (10.0 ** rng.uniform(-30, 30, n)).astype(T)
        a, b = (a * scale).astype(T), (b * scale).astype(T)
    elif kind == "inf_against_finite":
        a[n // 2] = np.inf
    elif kind == "inf_against_inf":
        a[n // 3] = b[n // 3] = np.inf
    elif kind == "nan_in_the_last_element":
        b[n - 1] = np.nan
    else:
        assert kind == "plain"
    return a, b, rtol, atol


def _norm_reference(kind, n, T):
    key = (kind, n, T)
    if key not in _norm_refs:
        a, b, rtol, atol = _norm_inputs(kind, n, T)
        _norm_refs[key] = (a, b, rtol, atol, M.error_norm(a, b, rtol, atol, EPS))
    return _norm_refs[key]


NORM_CASES = ([(k, 5, 0) for k in ("plain", "zero_tolerances_unequal", "zero_tolerances_equal", "opposite_signs", "magnitudes",
                                   "inf_against_finite", "inf_against_inf", "nan_in_the_last_element")] +
              [(k, 4100, s) for k in ("zero_tolerances_unequal", "zero_tolerances_equal", "opposite_signs", "magnitudes",
                                      "inf_against_finite", "inf_against_inf", "nan_in_the_last_element") for s in (0, 1)] +
              [(k, N_ALL_PARTIALS, s) for k in ("plain", "magnitudes", "nan_in_the_last_element") for s in (0, 1)])


@pytest.mark.parametrize("kind,n,shift", NORM_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_error_norm(dtype, kind, n, shift):
    """Terms in T in the kernel's operation order, summed exactly: what is left to the kernel is the order of a double sum of n
    non-negative terms, each addition within 2^-53 of its result: |got - ref| <= n 2^-52 ref (the division by n and the square
    root add two more roundings, covered by the factor 2)."""
    from torchsde_amd import kernels as K
    T = NP[dtype]
    a, b, rtol, atol, ref = _norm_reference(kind, n, T)
    ga, gb = Guarded(a, dtype, shift), Guarded(b, dtype, shift)
    got = K.error_norm(ga.view, gb.view, rtol, atol, EPS).item()
    print(f"{kind} n={n} shift={shift}: got {got!r} ref {ref!r}")
    if kind in ("inf_against_finite", "inf_against_inf", "nan_in_the_last_element"):
        assert math.isnan(ref) and math.isnan(got)
    elif kind == "zero_tolerances_equal":
        assert ref == float(T(EPS)) and got == ref
    else:
        assert math.isfinite(ref) and ref > float(T(EPS))
        assert abs(got - ref) <= n * 2.0 ** -52 * ref, (got, ref, abs(got - ref) / ref)
    assert ga.guards_intact() and gb.guards_intact() and same_bits(ga.view, a) and same_bits(gb.view, b)
