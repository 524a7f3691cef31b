"""What tests/test_prog_machine_reference.py and tests/test_gpu_prog_machine.py share (a helper: nothing here is collected).

The expression-program kernels of csrc/trajectory.hip state the meaning of an instruction word five times (two interpreters,
two generators, the row model). This module states it once more, independently and in high precision, and drives the C ABI so
that one launch reads a program's value -- or a tangent the kernel formed -- back EXACTLY:

  words       `word(op, src, k)` and the opcode / source names of include/torchsde_amd.h
  reference   `run_reference` (torch float64, differentiable: `reference_slopes`) and `run_mp` (mpmath at 40 digits with
              analytic slopes; numpy.longdouble where mpmath is missing) -- the stack discipline of
              tests/test_recognise._run_program: four slots asserted, DUP included; cube is (v*v)*v, softplus is v above 20 and
              log1p(exp(v)) otherwise, sigmoid is 1/(1+exp(-v))
  harness     `solve` (any launch of the three entry points, or of a generated unit) and `read_out` (one step from y0 = 0 with
              the step row [dt, dt/2, 1/dt, sqrt_dt, sw, sh, th, t0] = [1, .5, 1, 1, 0, 0, 0, t0]: W = z*0 = 0 and U = 0)
  ulp         `compare`: |got - ref| / spacing_T(ref), and the class checks where that has no meaning

Reading a slot (every scaling is a power of two, so nothing is rounded; +0 and -0 compare equal):
  f    Euler, g = LOAD const(0):                                     y1 = (0 + f*1) + 1*(g*0) = f
  g    Milstein Ito (v2 = (0 - 1)/2 = -1/2), f = LOAD const(0), g' = LOAD const(-2):   y1 = (g*(-1/2))*(-2) = g
  g'   the same with g = LOAD const(-2):                            y1 = g'
A value that is not finite can only be read through f: g*0 would turn it into NaN. The sensitivity entry point is read the same
way: a constant row with param_slot = s has tangent 1 in plane s, and plane s of the output is the slope the kernel formed."""
import ctypes
import math
import types

import numpy as np
import torch

try:
    import mpmath
except ImportError:                     # the yardstick of the float64 kernels is then numpy.longdouble (64-bit mantissa)
    mpmath = None

DEV = "cuda"

# ---- words (include/torchsde_amd.h: tsde_trajectory_prog_diag) ---------------------------------------------------------------
LOAD, ADD, SUB, RSUB, MUL, DIV, RDIV = range(7)
NEG, EXP, LOG, SIN, COS, TANH, SIGMOID, SOFTPLUS, SQRT, ABS, RELU, RECIP, SQUARE, CUBE, DUP = range(16, 31)
STACK, CONST, STATE, TIME = range(4)
EULER, MILSTEIN_ITO, MILSTEIN_STRAT, MIDPOINT, SRK, HEUN, EULER_HEUN = range(7)
BINARY = (ADD, SUB, RSUB, MUL, DIV, RDIV)
UNARY = (NEG, EXP, LOG, SIN, COS, TANH, SIGMOID, SOFTPLUS, SQRT, ABS, RELU, RECIP, SQUARE, CUBE)
NAMES = {LOAD: "LOAD", ADD: "ADD", SUB: "SUB", RSUB: "RSUB", MUL: "MUL", DIV: "DIV", RDIV: "RDIV", NEG: "NEG", EXP: "EXP",
         LOG: "LOG", SIN: "SIN", COS: "COS", TANH: "TANH", SIGMOID: "SIGMOID", SOFTPLUS: "SOFTPLUS", SQRT: "SQRT", ABS: "ABS",
         RELU: "RELU", RECIP: "RECIP", SQUARE: "SQUARE", CUBE: "CUBE", DUP: "DUP"}
MAX_WORDS, MAX_CONST, REG_ROWS, SENS = 96, 64, 8, 5


def word(op, src=0, k=0):
    return op | (src << 8) | (k << 16)


def fields(w):
    return w & 0xFF, (w >> 8) & 0xFF, w >> 16


# ---- the reference machine ---------------------------------------------------------------------------------------------------
def _softplus(v):
    inside = v <= 20
    return torch.where(inside, torch.log1p(torch.exp(torch.where(inside, v, torch.zeros_like(v)))), v)


class _Sqrt(torch.autograd.Function):
    """The correctly rounded square root (numpy's: the hardware instruction). torch's vectorised CPU sqrt is off by one ulp at
    about one float64 in 200, which a bit-for-bit expectation cannot afford."""

    @staticmethod
    def forward(ctx, v):
        with np.errstate(all="ignore"):
            r = torch.from_numpy(np.sqrt(v.detach().cpu().numpy())).to(v.device)
        ctx.save_for_backward(r)
        return r

    @staticmethod
    def backward(ctx, grad):
        r, = ctx.saved_tensors
        return grad * (0.5 / r)


_TORCH_UNARY = {NEG: torch.neg, EXP: torch.exp, LOG: torch.log, SIN: torch.sin, COS: torch.cos, TANH: torch.tanh,
                SIGMOID: lambda v: 1.0 / (1.0 + torch.exp(-v)), SOFTPLUS: _softplus, SQRT: _Sqrt.apply, ABS: torch.abs,
                RELU: torch.relu, RECIP: lambda v: 1.0 / v, SQUARE: lambda v: v * v, CUBE: lambda v: (v * v) * v}


def run_reference(words, consts, y, t, after=None):
    """The program's value on torch tensors (float64 for a reference; autograd follows). `consts`: a (n_const, d) tensor or a
    list of rows; `after`: applied to the result of every instruction (rounding to float32, say)."""
    after = after or (lambda v: v)
    stack = []
    for w in words:
        op, src, k = fields(w)
        if op < 16:
            if src == STACK:
                assert op != LOAD
                b, a = stack.pop(), stack.pop()
            else:
                time = torch.as_tensor(t, dtype=y.dtype)
                b = consts[k].expand_as(y) if src == CONST else (y if src == STATE else time.expand_as(y))
                a = stack.pop() if op != LOAD else None
            if op == LOAD:
                stack.append(b)
            else:
                stack.append(after({ADD: lambda: a + b, SUB: lambda: a - b, RSUB: lambda: b - a, MUL: lambda: a * b,
                                    DIV: lambda: a / b, RDIV: lambda: b / a}[op]()))
        elif op == DUP:
            stack.append(stack[-1])
        elif op == CUBE:                                  # two products, two roundings
            v = stack.pop()
            stack.append(after(after(v * v) * v))
        else:
            stack.append(after(_TORCH_UNARY[op](stack.pop())))
        assert len(stack) <= 4, "the machine has four stack slots"
    assert len(stack) == 1
    return stack[0]


def round_to_float32(v):
    return v.to(torch.float32).to(torch.float64)


def reference_slopes(words, consts, y, t, rows=()):
    """(value, d/dy, [d/d consts[k] for k in rows]) in float64 through autograd; everything is elementwise."""
    consts = torch.as_tensor(consts, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64)
    leaves = [consts[k].clone().requires_grad_(k in rows) for k in range(consts.shape[0])]
    yy = y.clone().requires_grad_(True)
    value = run_reference(words, leaves, yy, t)
    wanted = [yy] + [leaves[k] for k in rows]
    if value.requires_grad:
        grads = torch.autograd.grad(value.sum(), wanted, allow_unused=True)
    else:
        grads = [None] * len(wanted)
    grads = [torch.zeros_like(y) if g is None else g for g in grads]
    return value.detach(), grads[0], list(grads[1:])


class _HighPrecision:
    """mpmath at 40 digits, or numpy.longdouble: the few functions the machine needs."""

    def __init__(self):
        self.name = "mpmath" if mpmath is not None else "numpy.longdouble"
        if mpmath is not None:
            self.ctx = mpmath.mp.clone()
            self.ctx.dps = 40
            self.num = self.ctx.mpf
            for fn in ("exp", "log", "sin", "cos", "tanh", "log1p", "sqrt"):
                setattr(self, fn, getattr(self.ctx, fn))
        else:
            self.num = np.longdouble
            for fn in ("exp", "log", "sin", "cos", "tanh", "log1p", "sqrt"):
                setattr(self, fn, getattr(np, fn))


HP = _HighPrecision()


def run_mp(words, consts, y, t, seeds=()):
    """One element in high precision: (value, [tangent per seed]); a seed is "y" or a constant row. The slopes are the analytic
    ones (abs'(0) = relu'(0) = 0). `consts`: this element's entry of every row."""
    H, n = HP, len(seeds)
    zero, one = H.num(0), H.num(1)

    def leaf(value, name):
        return H.num(float(value)), [one if s == name else zero for s in seeds]

    def chain(x, value, slope):
        return value, [slope * d for d in x[1]]

    def unary(op, x):
        v = x[0]
        if op == NEG:
            return chain(x, -v, -one)
        if op == EXP:
            e = H.exp(v)
            return chain(x, e, e)
        if op == LOG:
            return chain(x, H.log(v), one / v)
        if op == SIN:
            return chain(x, H.sin(v), H.cos(v))
        if op == COS:
            return chain(x, H.cos(v), -H.sin(v))
        if op == TANH:
            th = H.tanh(v)
            return chain(x, th, one - th * th)
        if op == SIGMOID:
            s = one / (one + H.exp(-v))
            return chain(x, s, s * (one - s))
        if op == SOFTPLUS:
            return chain(x, v, one) if v > 20 else chain(x, H.log1p(H.exp(v)), one / (one + H.exp(-v)))
        if op == SQRT:
            r = H.sqrt(v)
            return chain(x, r, one / (2 * r))
        if op == ABS:
            return chain(x, abs(v), one if v > 0 else (-one if v < 0 else zero))
        if op == RELU:
            return chain(x, v if v > 0 else zero, one if v > 0 else zero)
        if op == RECIP:
            r = one / v
            return chain(x, r, -(r * r))
        if op == SQUARE:
            return chain(x, v * v, 2 * v)
        assert op == CUBE
        return chain(x, (v * v) * v, 3 * (v * v))

    def binary(op, a, b):
        if op in (RSUB, RDIV):
            a, b = b, a
            op = SUB if op == RSUB else DIV
        if op == ADD:
            return a[0] + b[0], [p + q for p, q in zip(a[1], b[1])]
        if op == SUB:
            return a[0] - b[0], [p - q for p, q in zip(a[1], b[1])]
        if op == MUL:
            return a[0] * b[0], [p * b[0] + a[0] * q for p, q in zip(a[1], b[1])]
        quotient = a[0] / b[0]
        return quotient, [(p - quotient * q) / b[0] for p, q in zip(a[1], b[1])]

    stack = []
    for w in words:
        op, src, k = fields(w)
        if op < 16:
            if src == STACK:
                b, a = stack.pop(), stack.pop()
            else:
                b = leaf(consts[k], k) if src == CONST else (leaf(y, "y") if src == STATE else leaf(t, None))
                a = stack.pop() if op != LOAD else None
            stack.append(b if op == LOAD else binary(op, a, b))
        elif op == DUP:
            stack.append(stack[-1])
        else:
            stack.append(unary(op, stack.pop()))
        assert len(stack) <= 4
    assert len(stack) == 1 and len(stack[0][1]) == n
    return stack[0]


# ---- ulp distance ------------------------------------------------------------------------------------------------------------
def np_dtype(dtype):
    return np.float32 if dtype in (torch.float32, np.float32) else np.float64


def compare(got, ref, dtype):
    """(ulps, right_class) per element. `got`: what a kernel (or torch) returned, in `dtype`; `ref`: the reference, float64
    numbers for float32 results and high-precision numbers (`HP.num`) for float64 ones.
    ulps = |got - ref| / spacing_T(ref), NaN where the element is judged by class alone: a reference that rounds to 0, +-inf or
    NaN in T has to be met exactly (class and sign), and where |ref| >= max_T / 2 or |ref| < 2 tiny_T only NaN-ness and sign are
    compared."""
    T = np_dtype(dtype)
    info = np.finfo(T)
    got = np.asarray(got, dtype=T).reshape(-1)
    n = got.size
    ulps, right = np.full(n, np.nan), np.zeros(n, dtype=bool)
    wide = T is np.float64
    ref = list(ref) if wide else np.asarray(ref, dtype=np.float64).reshape(-1)
    assert len(ref) == n
    with np.errstate(all="ignore"):
        for i in range(n):
            r = ref[i]
            rf = float(r)                               # (float64: correctly rounded from the high-precision number)
            if math.isnan(rf):
                right[i] = np.isnan(got[i])
                continue
            rt = T(rf)
            if np.isinf(rt) or rt == 0:
                right[i] = got[i] == rt
                continue
            if abs(rf) >= float(info.max) / 2 or abs(rf) < 2 * float(info.tiny):
                right[i] = (not np.isnan(got[i])) and (np.signbit(got[i]) == np.signbit(rt) or got[i] == 0)
                continue
            right[i] = bool(np.isfinite(got[i]))
            if not right[i]:
                continue
            spacing = float(np.spacing(np.abs(rt)))
            if wide:
                ulps[i] = float(abs(HP.num(float(got[i])) - r) / HP.num(spacing))
            else:
                ulps[i] = abs(float(got[i]) - rf) / spacing
    return ulps, right


def same_bits(a, b):
    """Equal element by element; NaN counts as equal to NaN (and +0 to -0)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


# ---- the harness -------------------------------------------------------------------------------------------------------------
ONE = (3, 67)            # one element per lane, a ragged last wave
VEC = (128, 4096)        # n / 4 = kTrajVecMinGroups with elem0 = 0: the smallest problem that takes four elements per lane


def read_row(t0=0.0):
    return [1.0, 0.5, 1.0, 1.0, 0.0, 0.0, 0.0, t0]


def noise_rows(n, dt, t_start=0.0):
    """Step rows of n equal steps with the real noise scales, one Brownian cell per step."""
    return [[dt, dt / 2, 1 / dt, math.sqrt(dt), math.sqrt(dt), math.sqrt(dt / 12), dt, t_start + k * dt] for k in range(n)]


def _schedule(step_rows, out_step, out_w, dtype):
    from torchsde_amd import kernels as K
    return K.TrajectorySchedule(step_rows, list(range(len(step_rows))), list(out_step), list(out_w), torch.device(DEV), dtype)


def unit_for(kind, dtype, f, g, dg, n_const, method):
    """The generated unit of these programs (specialise.lookup, compiled in the calling thread), or an assertion."""
    from torchsde_amd import specialise
    key, library = specialise.lookup(tuple(f), tuple(g), tuple(dg), n_const, dtype, method, torch.device(DEV), wait=True, kind=kind)
    assert library is not None, specialise.status().get(key)
    return library


def solve(kind, dtype, shape, f, g, dg, consts, *, method=EULER, step_rows=None, out_step=None, out_w=None, y0=None,
          scalar_noise=0, param_slot=None, entropy=2024, elem0=0, unit=None, check=True, fill=float("nan"), m=1, g_table=None):
    """One launch. kind: "values" (tsde_trajectory_prog_diag), "sens" (.._sens) or "additive" (tsde_trajectory_prog_additive:
    f only, `m` channels, a zero (m, d) table unless `g_table`); `unit`: a generated library (`unit_for`) in place of the
    interpreter. `consts`: (n_const, d), anything torch.as_tensor takes. Returns (ys (n_out, rows, d), sens or None, return code);
    a non-zero code raises unless `check` is False."""
    from torchsde_amd import _native, specialise
    lib = _native.load()
    rows, d = shape
    step_rows = [read_row()] if step_rows is None else step_rows
    out_step = [len(step_rows)] if out_step is None else out_step
    out_w = [(0.0, 1.0)] * len(out_step) if out_w is None else out_w
    schedule = _schedule(step_rows, out_step, out_w, dtype)
    consts = torch.as_tensor(consts, dtype=torch.float64).to(dtype).to(DEV).contiguous()
    n_const = consts.shape[0]
    assert consts.shape == (n_const, d) and 1 <= n_const <= MAX_CONST
    for w in tuple(f) + tuple(g) + tuple(dg):            # no word reads a row that is not there
        assert fields(w)[1] != CONST or fields(w)[2] < n_const
    if y0 is None:
        y0 = torch.zeros(rows, d, dtype=dtype, device=DEV)
    y0 = torch.as_tensor(y0, dtype=torch.float64).to(dtype).to(DEV).expand(rows, d).contiguous()
    n_out = len(out_step)
    ys = torch.full((n_out, rows, d), fill, dtype=dtype, device=DEV)
    sens = torch.full((n_out, SENS, rows, d), fill, dtype=dtype, device=DEV) if kind == "sens" else None
    stream = torch.cuda.current_stream().cuda_stream
    tail = (schedule.struct(), entropy, elem0, None, _native.dtype_code(dtype), stream)
    words = tuple(f) + tuple(g) + tuple(dg)
    code = (ctypes.c_uint32 * max(len(words), 1))(*words)
    slots = (ctypes.c_int8 * MAX_CONST)(*([-1] * MAX_CONST))
    for k, s in (param_slot or {}).items():
        slots[k] = s
    if kind == "additive" and g_table is None:
        g_table = torch.zeros(m, d, dtype=dtype, device=DEV)
    if unit is not None:
        bm = types.SimpleNamespace(_key=entropy, _elem0=elem0, _entropy_dev=None)
        sp = _native.stream_ptr()
        if kind == "values":
            args = (ys.data_ptr(), y0.data_ptr(), rows, d, consts.data_ptr(), n_const, int(scalar_noise))
        elif kind == "sens":
            args = (ys.data_ptr(), sens.data_ptr(), ctypes.cast(slots, ctypes.c_void_p), y0.data_ptr(), rows, d, consts.data_ptr(),
                    n_const, int(scalar_noise))
        else:
            args = (ys.data_ptr(), y0.data_ptr(), rows, d, m, consts.data_ptr(), n_const, g_table.data_ptr(), int(g_table.dim() == 4))
        specialise.launch(unit, schedule, bm, sp, *args)
        rc = 0
    elif kind == "values":
        rc = lib.tsde_trajectory_prog_diag(ys.data_ptr(), y0.data_ptr(), rows, d, code, len(f), len(g), len(dg), consts.data_ptr(),
                                           n_const, int(scalar_noise), method, *tail)
    elif kind == "sens":
        rc = lib.tsde_trajectory_prog_diag_sens(ys.data_ptr(), sens.data_ptr(), y0.data_ptr(), rows, d, code, len(f), len(g), len(dg),
                                                consts.data_ptr(), n_const, slots, int(scalar_noise), method, *tail)
    else:
        assert kind == "additive" and not g and not dg
        rc = lib.tsde_trajectory_prog_additive(ys.data_ptr(), y0.data_ptr(), rows, d, m, code, len(f), consts.data_ptr(), n_const,
                                               g_table.data_ptr(), int(g_table.dim() == 4), method, *tail)
    if check:
        _native.check(rc, f"{kind} launch")
    torch.cuda.synchronize()
    return ys, sens, rc


def slot_programs(prog, slot, zero_row, minus_two_row):
    """(f, g, dg, method) that read `prog` back through `slot` ("f", "g" or "dg") of a one-step solve from y0 = 0."""
    zero, m2 = [word(LOAD, CONST, zero_row)], [word(LOAD, CONST, minus_two_row)]
    if slot == "f":
        return list(prog), zero, zero, EULER
    if slot == "g":
        return zero, list(prog), m2, MILSTEIN_ITO
    assert slot == "dg"
    return zero, m2, list(prog), MILSTEIN_ITO


def read_out(kind, dtype, shape, prog, points, *, slot="f", t0=0.0, param_slot=None, aux=None, scalar_noise=0, compiled=False,
             state=None):
    """The value of `prog` at every point, read exactly through `slot`. `points`: (n_rows, P) -- constant rows, one point per
    CHANNEL; two rows (0 and -2) are appended for the other programs unless `aux` = (zero row, -2 row) names rows the caller
    already has. ONE: the channels go through in launches of 67; VEC: in launches of 4096 (padded by repeating the last point).
    Every batch row sees the same inputs and must return the same value. Returns a (P,) array -- with "sens" also the (5, P)
    tangent planes. `compiled`: through the generated unit of the same programs. kind "additive": f only. `state`: (P,) initial
    values in place of 0 -- every slot then returns state + value, exact as long as that sum is."""
    T = np_dtype(dtype)
    points = np.atleast_2d(np.asarray(points, dtype=np.float64))
    n_rows, P = points.shape
    if aux is None:
        points = np.concatenate([points, np.zeros((1, P)), np.full((1, P), -2.0)])
        aux = (n_rows, n_rows + 1)
    f, g, dg, method = slot_programs(prog, slot, *aux)
    if kind == "additive":
        assert slot == "f"
        g, dg = [], []
    unit = unit_for(kind if kind != "additive" else "additive4", dtype, f, g, dg, points.shape[0], method) if compiled else None
    rows, d = shape
    values, planes = np.empty(P, dtype=T), np.empty((SENS, P), dtype=T)
    for lo in range(0, P, d):
        chunk = points[:, lo:lo + d]
        width = chunk.shape[1]
        if width < d:
            chunk = np.concatenate([chunk, np.repeat(chunk[:, -1:], d - width, axis=1)], axis=1)
        y0 = None
        if state is not None:
            y0 = np.asarray(state, dtype=np.float64)[lo:lo + d]
            y0 = np.concatenate([y0, np.repeat(y0[-1:], d - width)])
        ys, sens, _ = solve(kind, dtype, shape, f, g, dg, chunk, method=method, step_rows=[read_row(t0)], param_slot=param_slot,
                            scalar_noise=scalar_noise, unit=unit, y0=y0)
        assert same_bits(ys[0], ys[0, :1].expand(rows, d)), "batch rows with the same inputs differ"
        values[lo:lo + width] = ys[0, 0, :width].cpu().numpy()
        if sens is not None:
            assert same_bits(sens[0], sens[0, :, :1].expand(SENS, rows, d))
            planes[:, lo:lo + width] = sens[0, :, 0, :width].cpu().numpy()
    return (values, planes) if kind == "sens" else values


# ---- test points -------------------------------------------------------------------------------------------------------------
def _rounded(values, dtype):
    """The values as numbers of `dtype`, held in float64."""
    return np.asarray(values, dtype=np.float64).astype(np_dtype(dtype)).astype(np.float64)


def arithmetic_points(dtype):
    """(a, b) for the arithmetic opcodes: 4096 random pairs with exponents in [-40, 40] and either sign, then the edges: +-1,
    perfect squares, 1 +- 2^-23, divisor 0, sqrt of a negative, reciprocal of 2^-100, the square of 2^64 and the cube of 2^43 (inf in
    float32) -- and for float64 the same at its own limits. No operand, intermediate or result is subnormal."""
    rng = np.random.default_rng(20240607)
    n = 4096

    def random():
        return np.ldexp((1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n), rng.integers(-40, 41, n))
    a, b = random(), random()
    e = 2.0 ** -23
    edge_a = [1, -1, 1, -1, 4, 9, 16, 0.25, 2.25, 1 + e, 1 - e, 1, -1, -4, 2.0 ** -100, 2.0 ** 64, 2.0 ** 43, 0, 1 + e, 1 - e]
    edge_b = [1, 1, -1, -1, 9, 4, 0.25, 16, 2.25, 1 - e, 1 + e, 0, 0, 2, 2.0 ** -100, 2.0 ** 64, 2.0 ** 43, 3, 1 + e, 1 - e]
    if np_dtype(dtype) is np.float64:
        e = 2.0 ** -52
        edge_a += [1 + e, 1 - e, 2.0 ** -1000, 2.0 ** 512, 2.0 ** 342, 1 + e]
        edge_b += [1 - e, 1 + e, 2.0 ** -1000, 2.0 ** 512, 2.0 ** 342, 1 + e]
    return _rounded(np.concatenate([a, edge_a]), dtype), _rounded(np.concatenate([b, edge_b]), dtype)


ARITHMETIC = (ADD, SUB, RSUB, MUL, DIV, RDIV, NEG, ABS, RELU, RECIP, SQUARE, CUBE, SQRT)
FUNCTIONS = (EXP, LOG, SIN, COS, TANH, SIGMOID, SOFTPLUS)
PER_GROUP = 32


def _binades(rng, exponents, dtype, negative_cap=None, positive_cap=None):
    """PER_GROUP points in every binade [2^e, 2^(e+1)) of `exponents`, cut at the caps, for each sign that has a cap."""
    out = []
    for sign, cap in ((-1.0, negative_cap), (1.0, positive_cap)):
        if cap is None:
            continue
        for e in exponents:
            lo, hi = 2.0 ** e, min(2.0 ** (e + 1), cap)
            if lo >= hi:
                continue
            pts = _rounded(lo + (hi - lo) * rng.random(PER_GROUP), dtype)
            out.append(sign * np.clip(pts, lo, np.nextafter(np_dtype(dtype)(hi), np_dtype(dtype)(0))))
    return np.concatenate(out)


def function_points(op, dtype):
    """(points, class points) of a function opcode: the ranges of the accuracy rule -- the float64 kernels' ranges reach to their
    own overflow points -- at least PER_GROUP points in every group (sign, binade), and the inputs that are judged by class
    alone, {input: what is expected}."""
    wide = np_dtype(dtype) is np.float64
    T = np_dtype(dtype)
    rng = np.random.default_rng(1000 + op)
    big = 9 if wide else 6                           # 2^big: the binade of the largest argument exp takes
    inf = float("inf")
    if op == EXP:
        pts = _binades(rng, range(-10, big + 1), dtype, 708.0 if wide else 87.0, 709.0 if wide else 88.0)
        return pts, {1000.0 if wide else 100.0: inf}
    if op == LOG:
        span, bits = ((range(-1000, 1000, 40), 52) if wide else (range(-100, 100, 4), 23))
        near_one = [1 + s * 2.0 ** -k for k in range(1, bits + 1) for s in (1, -1)]
        pts = np.concatenate([_binades(rng, sorted(set(span) | {-1, 0}), dtype, None, inf), _rounded(near_one, dtype)])
        return pts, {0.0: -inf, -1.0: float("nan")}
    if op in (SIN, COS):
        return _binades(rng, range(-10, 3), dtype, 8.0, 8.0), {1e3: "unit", 1e5: "unit"}
    if op == TANH:
        return _binades(rng, range(-30, 5), dtype, 20.0, 20.0), {}
    if op == SIGMOID:
        return _binades(rng, range(-10, big + 1), dtype, 700.0 if wide else 80.0, 700.0 if wide else 80.0), {}
    assert op == SOFTPLUS
    twenty = T(20)
    special = [20.0, float(np.nextafter(twenty, T(0))), float(np.nextafter(twenty, T(100))), 20.5, 100.0]
    above = [20.5 + 11.0 * rng.random(PER_GROUP), 32 + 32 * rng.random(PER_GROUP), 64 + 64 * rng.random(PER_GROUP)]
    pts = np.concatenate([_binades(rng, range(-10, big + 1), dtype, 700.0 if wide else 80.0, 19.999),
                          _rounded(np.concatenate(above), dtype), _rounded(special, dtype)])
    return pts, {}


def groups(points):
    """{(sign, binade of |v|): indices}"""
    out = {}
    for i, v in enumerate(points):
        out.setdefault((-1 if v < 0 else 1, int(math.floor(math.log2(abs(v))))), []).append(i)
    return out


def mp_values(prog, points, seeds=()):
    """`run_mp` over the channels of `points` (n_rows, P): ([value], [[tangent per seed]])."""
    points = np.atleast_2d(points)
    values, tangents = [], []
    for c in range(points.shape[1]):
        v, d = run_mp(prog, points[:, c], 0.0, 0.0, seeds)
        values.append(v)
        tangents.append(d)
    return values, tangents
