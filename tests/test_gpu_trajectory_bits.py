"""The whole-trajectory kernels of csrc/trajectory.hip, pinned bit for bit (``-m gpu``): every family, every method the
family accepts, float32 and float64, one launch per case through the C ABI, and the SHA-256 of the output bytes compared with
``tests/golden/trajectory_kernel_bits.json`` -- recorded from the build BEFORE the kernels' shared step header, noise draw,
output emitter and dispatch were factored out (tests/golden/make_trajectory_kernel_bits.py). The other GPU tests hold these
kernels to the stepwise route; this one holds a refactor of them to what they computed before it.

Shapes: (5, 6) -- one element per lane, an odd first element of the noise field; (8192, 64) -- n / 4 = 131072 groups, the
smallest problem that takes the four-elements-per-lane form. Twelve steps of unequal size and five outputs: two inside one
step, one on a step boundary, one inside a later step, and the last step (the interpolating branch, the exact branch and the
loop of the emitter). Every input is an exact binary fraction computed with integer arithmetic, so the inputs are the same
bits wherever the test runs."""
import ctypes
import hashlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_kernel_bits.json")

N_STEPS = 12
OUT_STEP = [3, 3, 7, 9, 12]
OUT_W = [(0.75, 0.25), (0.25, 0.75), (0.0, 1.0), (0.5, 0.5), (0.0, 1.0)]
SHAPES = {"small": (5, 6, 7), "vector": (8192, 64, 8)}        # rows, d, first element of the noise field
METHOD_NAMES = ["euler", "milstein_ito", "milstein_strat", "midpoint", "srk", "heun", "euler_heun"]   # TSDE_TRAJ_* codes 0..6
STAGE_SLOTS = [1, 1, 1, 2, 4, 2, 2]                           # csrc/trajectory.hip stage_slots
ADDITIVE_METHODS = (0, 3, 4)
FAMILIES = ["affine", "affine_linear", "affine_timed", "affine_sens", "expr", "expr_timed", "prog_diagonal", "prog_scalar",
            "prog_sens", "additive_m3", "additive_m8"]
ENTROPY = 2024
SAMPLES = 8


def _cases():
    for family in FAMILIES:
        for method in (ADDITIVE_METHODS if family.startswith("additive") else range(7)):
            for dtype in ("float32", "float64"):
                for shape in SHAPES:
                    yield f"{family}-{METHOD_NAMES[method]}-{dtype}-{shape}"


CASES = list(_cases())


def _fractions(numerators, denominator, dtype):
    """numerators / denominator (a power of two) as a device tensor: exact in either dtype."""
    return (numerators.to(torch.float64) / denominator).to(dtype).to(DEV)


def _channel(d, mul, mod, denominator, offset, dtype):
    return _fractions((torch.arange(d) * mul) % mod, denominator, dtype) + offset


def _table(n_rows, d, mul, mod, denominator, offset, dtype):
    r, c = torch.arange(n_rows).reshape(-1, 1), torch.arange(d).reshape(1, -1)
    return (_fractions((r * mul + c * 3) % mod, denominator, dtype) + offset).contiguous()


def _schedule(dtype):
    from torchsde_amd import kernels as K
    rows, t = [], 0.0
    for k in range(N_STEPS):
        dt = (4 + (k * 3) % 5) / 256.0                        # unequal steps, one Brownian cell each
        rows.append([dt, dt / 2, 1 / dt, math.sqrt(dt), math.sqrt(dt), math.sqrt(dt / 12), dt, t])
        t += dt
    return K.TrajectorySchedule(rows, list(range(N_STEPS)), OUT_STEP, OUT_W, torch.device(DEV), dtype)


def _word(op, src=0, k=0):
    return op | (src << 8) | (k << 16)


# csrc/trajectory.hip: sources 1 = constant row k, 2 = the state, 3 = the stage time; opcodes
_LOAD, _ADD, _RSUB, _MUL, _SIN, _TANH, _SQUARE = 0, 1, 3, 4, 19, 21, 28
F_CODE = [_word(_LOAD, 2), _word(_SIN), _word(_MUL, 1, 0), _word(_ADD, 3)]                                # c0 sin(y) + t
G_CODE = [_word(_LOAD, 2), _word(_TANH), _word(_MUL, 1, 1), _word(_ADD, 1, 2)]                            # c1 tanh(y) + c2
DG_CODE = [_word(_LOAD, 2), _word(_TANH), _word(_SQUARE), _word(_RSUB, 1, 3), _word(_MUL, 1, 1)]          # c1 (1 - tanh(y)^2)


def run_case(case):
    """One launch; the tensors it wrote (values, and the sensitivities of the families that have them)."""
    from torchsde_amd import _native
    lib = _native.load()
    family, method_name, dtype_name, shape = case.split("-")
    method, dtype = METHOD_NAMES.index(method_name), getattr(torch, dtype_name)
    rows, d, elem0 = SHAPES[shape]
    n, n_out = rows * d, len(OUT_STEP)
    schedule = _schedule(dtype)
    tail = (schedule.struct(), ENTROPY, elem0, None, _native.dtype_code(dtype), torch.cuda.current_stream().cuda_stream)
    y0 = (_fractions((torch.arange(n) * 7919) % 1024, 1024, dtype) + 0.5).reshape(rows, d)
    ys = torch.full((n_out, rows, d), float("nan"), dtype=dtype, device=DEV)
    sens = torch.full((n_out, _native.TRAJ_SENS, rows, d), float("nan"), dtype=dtype, device=DEV)
    out = [ys]
    if family.startswith("affine"):
        timed_rows = N_STEPS * STAGE_SLOTS[method]
        if family == "affine_timed":
            a, b, c, e = (_table(timed_rows, d, 7, 16, 256, offset, dtype) for offset in (-0.25, -0.03125, 0.125, 0.0))
        else:
            a, b = _channel(d, 13, 32, 64, -0.5, dtype), _channel(d, 5, 16, 64, -0.125, dtype)
            c, e = _channel(d, 11, 32, 128, 0.125, dtype), _channel(d, 3, 8, 64, 0.0, dtype)
        if family == "affine":
            code = lib.tsde_trajectory_affine_diag(ys.data_ptr(), y0.data_ptr(), rows, d, a.data_ptr(), b.data_ptr(), c.data_ptr(),
                                                   e.data_ptr(), method, *tail)
        elif family == "affine_linear":
            code = lib.tsde_trajectory_affine_diag(ys.data_ptr(), y0.data_ptr(), rows, d, a.data_ptr(), None, c.data_ptr(), None,
                                                   method, *tail)
        elif family == "affine_timed":
            code = lib.tsde_trajectory_affine_diag_timed(ys.data_ptr(), y0.data_ptr(), rows, d, a.data_ptr(), b.data_ptr(),
                                                         c.data_ptr(), e.data_ptr(), d, method, *tail)
        else:
            code = lib.tsde_trajectory_affine_diag_sens(ys.data_ptr(), sens.data_ptr(), y0.data_ptr(), rows, d, a.data_ptr(),
                                                        b.data_ptr(), c.data_ptr(), e.data_ptr(), method, *tail)
            out.append(sens)
    elif family.startswith("expr"):
        timed = family == "expr_timed"
        offsets = (0.5, 0.75, -0.25, 0.0625, 0.25, 0.5, 0.125, 0.03125)       # drift scale, rate, shift, offset; diffusion likewise
        if timed:
            coefs = [_table(N_STEPS * STAGE_SLOTS[method], d, 5 + i, 16, 256, offset, dtype) for i, offset in enumerate(offsets)]
        else:
            coefs = [_channel(d, 3 + 2 * i, 16, 128, offset, dtype) for i, offset in enumerate(offsets)]
        arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in coefs])
        code = lib.tsde_trajectory_expr_diag_timed(ys.data_ptr(), y0.data_ptr(), rows, d, arr, d if timed else 0,
                                                   _native.FN_CODES["tanh"], _native.FN_CODES["sigmoid"], method, *tail)
    else:
        consts = torch.stack([_channel(d, 7, 16, 64, -0.5, dtype), _channel(d, 5, 16, 128, 0.125, dtype),
                              _channel(d, 3, 8, 128, 0.0625, dtype), torch.ones(d, dtype=dtype, device=DEV)]).contiguous()
        if family.startswith("prog"):
            words = F_CODE + G_CODE + DG_CODE
            prog = ((ctypes.c_uint32 * len(words))(*words), len(F_CODE), len(G_CODE), len(DG_CODE), consts.data_ptr(), 4)
            if family == "prog_sens":
                slots = (ctypes.c_int8 * 4)(1, 2, 3, -1)
                code = lib.tsde_trajectory_prog_diag_sens(ys.data_ptr(), sens.data_ptr(), y0.data_ptr(), rows, d, *prog, slots, 0,
                                                          method, *tail)
                out.append(sens)
            else:
                code = lib.tsde_trajectory_prog_diag(ys.data_ptr(), y0.data_ptr(), rows, d, *prog,
                                                     int(family == "prog_scalar"), method, *tail)
        else:
            m = int(family[len("additive_m"):])
            slots = 1 if method == 0 else 2
            r, c = torch.arange(N_STEPS * slots * m).reshape(-1, 1), torch.arange(d).reshape(1, -1)
            gtab = _fractions((r * 5 + c) % 32, 256, dtype).reshape(N_STEPS, slots, m, d).contiguous()
            code = lib.tsde_trajectory_prog_additive(ys.data_ptr(), y0.data_ptr(), rows, d, m,
                                                     (ctypes.c_uint32 * len(F_CODE))(*F_CODE), len(F_CODE), consts.data_ptr(), 4,
                                                     gtab.data_ptr(), 1, method, *tail)
    _native.check(code, case)
    torch.cuda.synchronize()
    return out


def digest(tensors):
    """SHA-256 of the tensors' bytes, and SAMPLES values spread over them (as hexadecimal floats: exact)."""
    h, samples = hashlib.sha256(), []
    for t in tensors:
        flat = t.reshape(-1).cpu()
        h.update(flat.numpy().tobytes())
        samples += [float(flat[(k * (flat.numel() - 1)) // (SAMPLES // len(tensors) - 1)]).hex()
                    for k in range(SAMPLES // len(tensors))]
    return {"sha256": h.hexdigest(), "samples": samples}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_kernel_reproduces_the_recorded_bits(case, golden):
    got, want = digest(run_case(case)), golden["cases"][case]
    assert got["sha256"] == want["sha256"], f"{case}: sampled values {got['samples']} against the recorded {want['samples']}"
