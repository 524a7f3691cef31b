"""The 16-byte path and the scalar path of every flat elementwise step kernel compute the same bits (run with ``-m gpu``).

A launcher takes the 16-byte path when ``n % 4 == 0``, every operand is 16-byte aligned and the noise allows it
(csrc/tsde_launch.h: `vec_ok`, `noise_vec_ok`). A wrong answer there does not crash: it drops up to three tail elements, reads
the wrong row of a row-broadcast increment, or takes the slow path. So each entry point of `kernels.py` runs the SAME operand
values in layouts that sit on either side of that decision -- aligned (one tile; a grid of 8 blocks), views one element into
larger buffers, the first 1023 elements, a row-broadcast increment with 4 and with 3 channels a row -- into outputs pre-filled
with NaN, and the layouts must agree bit for bit on the elements they share, leave no NaN, write nothing behind their last
element, and (float64) agree with the torch statement of the wrapper's formula. External noise throughout, so the arithmetic
does not depend on which normal routine a path draws with (the generated-noise predicates: test_gpu_parity.py,
test_gpu_box_muller_shared.py)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_BIG, N = 8192, 1024
DT, CG = 0.07, 0.9
SQRT_DT, RDT = math.sqrt(DT), 1.0 / DT
HA, HB = 0.03, 0.04

_rng = np.random.default_rng(20261020)
_BASE = {name: _rng.standard_normal(N_BIG) for name in "abcde"}           # the operands, in the order an op takes them
_BASE["W"] = _rng.standard_normal(N_BIG) * SQRT_DT
_BASE["U"] = _rng.standard_normal(N_BIG) * DT * SQRT_DT


def _kernels():
    from torchsde_amd import kernels
    return kernels


# ---- the entry points: (inputs, noise, run, float64 statement) -----------------------------------------------------------
# run(k, ins, noise, outs) -> tuple of outputs; `outs`: NaN-filled buffers for the wrappers that take them (None entries: the
# wrapper allocates). statement(ins, W, U) -> tuple of tensors, the formula of the wrapper's docstring.
class Op:
    def __init__(self, n_in, noise, run, statement, n_out=1, takes_out=True):
        self.n_in, self.noise, self.run, self.statement = n_in, noise, run, statement
        self.n_out, self.takes_out = n_out, takes_out


def _gf_diag(ito):
    def statement(i, W, U):
        v = W * W - DT if ito else W * W
        return (((i[0] + i[1] * DT) + i[2] * W) + ((i[3] - i[2]) * v) / (2 * SQRT_DT),)
    return Op(4, "W", lambda k, i, nz, o: (k.milstein_gf_diag(i[0], i[1], i[2], i[3], DT, SQRT_DT, ito, nz, out=o[0]),),
              statement)


def _gf_prime(ito):
    return Op(3, None, lambda k, i, nz, o: (k.milstein_gf_prime(i[0], i[1], i[2], DT, SQRT_DT, ito, out=o[0]),),
              lambda i, W, U: (((i[0] + DT * i[1]) + i[2] * SQRT_DT) if ito else (i[0] + i[2] * SQRT_DT),))


def _weight(ito):
    return Op(1, "W", lambda k, i, nz, o: (k.milstein_weight(i[0], nz, DT, ito, 0.5),),
              lambda i, W, U: (i[0] * (0.5 * ((W * W - DT) if ito else W * W)),), takes_out=False)


def _srk(stage):
    n_in, n_out = (0, 3, 5, 4, 2)[stage], (0, 3, 3, 2, 1)[stage]

    def run(k, i, nz, o):
        return k.srk_diag_stage(stage, list(i), DT, RDT, SQRT_DT, nz, out_last=o[0] if stage == 4 else None)

    def statement(i, W, U):
        k = _kernels()
        return k._srk_diag_stage_autograd(stage, list(i), DT, RDT, SQRT_DT, k.NoiseSpec.external(W, U))

    # (stage 3 advances its second input in place: every run works on its own copy of the operands)
    return Op(n_in, "WU", run, statement, n_out=n_out, takes_out=stage == 4)


def _heun(mode, prod):
    def run(k, i, nz, o):
        return (k.heun_final(i[0], i[1], i[2] if mode == 0 else None, i[3], i[4], DT, mode, nz, prod=prod, out=o[0]),)

    def statement(i, W, U):
        p0, p1 = (i[3], i[4]) if prod else (i[3] * W, i[4] * W)
        if mode == 0:
            return (i[0] + (((DT * (i[1] + i[2])) + p0) + p1) * 0.5,)
        return ((i[0] + DT * i[1]) + ((p0 + p1) * 0.5),)
    return Op(5, None if prod else "W", run, statement)


def _adj_b_statement(i, W, U):
    z = i[1] + i[2]
    return i[0] + 2 * z, -z, i[0] * (0.5 * DT) + z * DT, i[0] * (0.5 * W) + z * W


def _merge(with_u):
    def run(k, i, nz, o):
        return tuple(t for t in k.merge_halves(o[0], o[1] if with_u else None, i[0], i[1] if with_u else None, i[2],
                                               i[3] if with_u else None, ha=HA, hb=HB) if t is not None)

    def statement(i, W, U):
        w = i[0] + i[2]
        if not with_u:
            return (w,)
        h = (HB * (i[3] + 0.5 * i[0]) + HA * (i[1] - 0.5 * i[2])) / (HA + HB)
        return w, (HA + HB) * (0.5 * w + h)
    return Op(4, None, run, statement, n_out=2 if with_u else 1)


OPS = {
    "step_diag": Op(3, "W", lambda k, i, nz, o: (k.step_diag(i[0], i[1], i[2], DT, CG, nz, out=o[0]),),
                    lambda i, W, U: ((i[0] + DT * i[1]) + CG * (i[2] * W),)),
    "step_prod": Op(3, None, lambda k, i, nz, o: (k.step_prod(i[0], i[1], i[2], DT, CG, out=o[0]),),
                    lambda i, W, U: ((i[0] + DT * i[1]) + CG * i[2],)),
    "milstein_diag": Op(4, "W", lambda k, i, nz, o: (k.milstein_diag(i[0], i[1], i[2], i[3], DT, nz, out=o[0]),),
                        lambda i, W, U: (((i[0] + i[1] * DT) + i[2] * W) + i[3],)),
    "milstein_gf_prime-ito": _gf_prime(True), "milstein_gf_prime-strat": _gf_prime(False),
    "milstein_gf_diag-ito": _gf_diag(True), "milstein_gf_diag-strat": _gf_diag(False),
    "milstein_weight-ito": _weight(True), "milstein_weight-strat": _weight(False),
    "srk_diag_stage-1": _srk(1), "srk_diag_stage-2": _srk(2), "srk_diag_stage-3": _srk(3), "srk_diag_stage-4": _srk(4),
    "heun_final-heun": _heun(0, False), "heun_final-euler_heun": _heun(1, False),
    "heun_final-heun-prod": _heun(0, True), "heun_final-euler_heun-prod": _heun(1, True),
    "rheun_z": Op(4, "W", lambda k, i, nz, o: (k.rheun_z(i[0], i[1], i[2], i[3], DT, -1.0, nz, out=o[0]),),
                  lambda i, W, U: (((2 * i[0] - i[1]) + -1.0 * (i[2] * DT)) + -1.0 * (i[3] * W),)),
    "rheun_y": Op(5, "W", lambda k, i, nz, o: (k.rheun_y(i[0], i[1], i[2], i[3], i[4], 0.5 * DT, 1.0, nz, out=o[0]),),
                  lambda i, W, U: ((i[0] + (i[1] + i[2]) * (0.5 * DT)) + (i[3] + i[4]) * (0.5 * W),)),
    "lincomb2": Op(2, None, lambda k, i, nz, o: (k.lincomb2(i[0], i[1], 0.3, -1.7, out=o[0]),),
                   lambda i, W, U: (0.3 * i[0] + -1.7 * i[1],)),
    "rheun_adj_a": Op(3, "W", lambda k, i, nz, o: tuple(k.rheun_adj_a(i[0], i[1], i[2], 0.5 * DT, nz)),
                      lambda i, W, U: (i[1] + i[0] * (0.5 * DT), i[2] + i[0] * (0.5 * W)), n_out=2, takes_out=False),
    "rheun_adj_b": Op(3, "W", lambda k, i, nz, o: tuple(k.rheun_adj_b(i[0], i[1], i[2], DT, 0.5 * DT, nz)),
                      _adj_b_statement, n_out=4, takes_out=False),
    "linear_interp": Op(2, None, lambda k, i, nz, o: (k.linear_interp(i[0], i[1], 0.25, 0.75, out=o[0]),),
                        lambda i, W, U: (0.25 * i[0] + 0.75 * i[1],)),
    "merge_halves": _merge(False), "merge_halves-U": _merge(True),
}


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def _place(values, layout):
    """A tensor of these values (on the device): aligned, or (`offset`) a view one element into a larger buffer."""
    if layout != "offset":
        return values.clone()
    buf = torch.empty(values.numel() + 1, dtype=values.dtype, device=DEV)
    buf[1:] = values
    return buf[1:]


def _nan_out(n, dtype, layout):
    """(the view a kernel writes to, the elements around it): one spare element behind the view, and with `offset` one in
    front of it, which must stay NaN."""
    lead = 1 if layout == "offset" else 0
    buf = torch.full((lead + n + 1,), float("nan"), dtype=dtype, device=DEV)
    return buf[lead:lead + n], (buf, lead)


def _poison(n, dtype, count):
    """NaN into the blocks the caching allocator hands out next for `count` tensors of n elements (the wrappers that allocate
    their own outputs): a path that leaves a tail unwritten then shows it, not the bits of an earlier run."""
    junk = [torch.full((n,), float("nan"), dtype=dtype, device=DEV) for _ in range(count)]
    del junk


def _run(op, dtype, base, n, layout, bcast_d=0, expand=0):
    """Outputs of `op` on the first n elements of the operands. `bcast_d`: the increment has one value per row of bcast_d
    elements; `expand`: the same increment, written out per element."""
    k = _kernels()
    ins = [_place(base[name][:n], layout) for name in "abcde"[:op.n_in]]
    noise = None
    if op.noise:
        if bcast_d:
            W, U = base["W"][:n // bcast_d], base["U"][:n // bcast_d]
        elif expand:
            W, U = (base[name][:n // expand].repeat_interleave(expand) for name in "WU")
        else:
            W, U = base["W"][:n], base["U"][:n]
        noise = k.NoiseSpec.external(_place(W, layout), _place(U, layout) if op.noise == "WU" else None, bcast_d=bcast_d)
    outs, buffers = [None] * op.n_out, []
    if op.takes_out:
        for j in range(op.n_out):
            outs[j], around = _nan_out(n, dtype, layout)
            buffers.append(around)
    else:
        _poison(n, dtype, op.n_out)
    result = op.run(k, ins, noise, outs)
    torch.cuda.synchronize()
    assert len(result) == op.n_out
    for j, r in enumerate(result):
        assert r.numel() == n and not torch.isnan(r).any(), f"output {j}: NaN left in {layout} n={n} bcast_d={bcast_d}"
    for buf, lead in buffers:
        assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + n:]).all(), f"wrote outside its {n} elements ({layout})"
    return [r.reshape(-1) for r in result]


@pytest.fixture(scope="module", params=[torch.float32, torch.float64], ids=["f32", "f64"])
def operands(request):
    """The operand values in this dtype, on the device; nothing changes them (every layout works on copies)."""
    return request.param, {name: torch.from_numpy(v).to(request.param).to(DEV) for name, v in _BASE.items()}


@pytest.mark.parametrize("name", list(OPS))
def test_paths_agree_bitwise(name, operands):
    dtype, base = operands
    op = OPS[name]
    one_tile, eight_blocks = _run(op, dtype, base, N, "aligned"), _run(op, dtype, base, N_BIG, "aligned")
    for label, got, shared in (("8 blocks", eight_blocks, N),
                               ("offset views", _run(op, dtype, base, N, "offset"), N),
                               ("first 1023", _run(op, dtype, base, N - 1, "aligned"), N - 1)):
        for j, (a, b) in enumerate(zip(one_tile, got)):
            assert torch.equal(a[:shared], b[:shared]), f"{name} output {j}: {label} differs from the aligned 1024"
    if op.noise:
        for d, n in ((4, N), (3, 1020)):          # 1020: whole groups of 4 and whole rows of 3 -- only the rows say "scalar"
            flat = _run(op, dtype, base, n, "aligned", expand=d)
            rows = _run(op, dtype, base, n, "aligned", bcast_d=d)
            for j, (a, b) in enumerate(zip(flat, rows)):
                assert torch.equal(a, b), f"{name} output {j}: bcast_d={d} differs from the increment written out"
    if dtype == torch.float64:
        ins = [base[c] for c in "abcde"[:op.n_in]]
        want = op.statement(ins, base["W"], base["U"])
        for j, (a, b) in enumerate(zip(eight_blocks, want)):
            torch.testing.assert_close(a, b.reshape(-1), rtol=1e-9, atol=1e-11, msg=lambda m: f"{name} output {j}: {m}")
