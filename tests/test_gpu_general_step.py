"""``tsde_step_general`` / ``tsde_step_general_w``: the per-row contraction y1 = (y0 + (ca*f)*cf) + cg*(g . w) against a
float64 statement of it, on every kernel, instantiation and rows-per-wave that `launch_step_general` can pick (csrc/steps.hip;
the cases and what each reaches: tests/helpers_general_step.py, held to the launcher on the CPU by
tests/test_general_step_cases.py). Run with ``-m gpu``.

The bound. Per element |got - want| <= (m + 16) * u * S with S = |y0| + |ca*f*cf| + |cg| * sum_j |g_ij| |w_j| and u the unit
roundoff of the launch dtype (doubled in float64, where the reference is float64 arithmetic itself). m + 16 counts the
roundings on the longest path from the stored operands to the stored result: the weight (cu*U, *rdt, cw*W, their sum) <= 4,
the product 1, the sum over the channels <= max(m, 9) (the generic kernel adds m terms in sequence; the vector kernels add
4 and then log2(m / 4) <= 6 shuffle steps), the epilogue 5, the casts of ca, cf, cg, cw, cu to the launch dtype <= 4.
It is a count, not a measurement.

Generated against external increments. `normal4_pairs` returns the bits of `normal4`, and `lane_weights` / `stage_noise`
form W = n * sw and U = th * (0.5 * W + n * sh) with the expressions of `cell_noise`, which `NoiseSpec.materialise` runs
(the library is built with -ffp-contract=off). So a launch that generates its increments and the launch that is handed
them as tensors must agree bit for bit, in all three weight modes."""
import pytest
import torch

from tests import helpers_general_step as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
CF, CG = 2.0 ** -7, 0.5
RDT = 1.0 / CF
# (mode, (ca, cw, cu)): the triples of tests/test_gpu_shared_diffusion.py, and mode 2 once more with a cw that is not 1
MODES = ((0, (1.0, 0.0, 0.0)), (1, (0.75, 0.0, 1.5)), (2, (1 / 3, 1.0, -1.0)), (2, (0.6, -0.5, 0.25)))
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
KID_STEP_GENERAL = 2
WORST = {}           # kernel class -> largest error / bound seen (printed; the summary of the suite quotes it)


def _K():
    from torchsde_amd import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: per kernel class, the largest error / bound of the run -- the room the counted constant leaves."""
    yield
    for label in sorted(WORST):
        print(f"WORST {label}: error / bound = {WORST[label]:.4f}")
    torch.cuda.empty_cache()      # the large cases' blocks go back to the device, not to the rest of the suite's process


def _spec(B, m, dtype, cell=3, h=2.0 ** -7, elem0=0):
    return _K().NoiseSpec((B, m), dtype, torch.device(DEV), entropy=0x1234567, elem0=elem0, cell=cell, h=h)


def _offset_view(t):
    """The same values as a view one element into a larger buffer (off the 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def _nan_out(B, d, dtype, layout):
    """tests/test_gpu_step_paths.py `_nan_out`: the view a kernel writes to and the NaN guard elements around it."""
    lead, n = (1 if layout == "offset" else 0), B * d
    buf = torch.full((lead + n + 1,), float("nan"), dtype=dtype, device=DEV)
    return buf[lead:lead + n].view(B, d), buf, lead


def _launch(y0, f, g, mode, coefs, noise, layout="aligned", cf=CF, rdt=RDT):
    """One call through the public wrapper into a NaN-filled output: exactly one launch, nothing left unwritten, nothing
    written outside."""
    K = _K()
    ca, cw, cu = coefs
    B, d = y0.shape
    out, buf, lead = _nan_out(B, d, y0.dtype, layout)
    K.prof_begin(KID_STEP_GENERAL, 4)
    with torch.no_grad():
        if mode == 0 and ca == 1.0:
            got = K.step_general(y0, f, g, cf, CG, noise, out=out)
        else:
            got = K.step_general_weighted(y0, f, g, ca, cf, CG, mode, cw, cu, rdt, noise, out=out)
    torch.cuda.synchronize()
    assert K.prof_end()[1] == 1
    assert got.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any(), f"NaN left in the output ({layout})"
    assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + B * d:]).all(), f"wrote outside its output ({layout})"
    return out


def _weight(mode, coefs, W, U):
    _, cw, cu = coefs
    W, U = W.double(), U.double()
    return W if mode == 0 else ((cu * U) * RDT if mode == 1 else (cw * W) + (cu * U) * RDT)


def _check_bound(got, y0, f, g, mode, coefs, W, U, label, what):
    """|got - want| <= (m + 16) u S per element, in float64 from the operands as stored."""
    ca = coefs[0]
    m, dtype = g.shape[-1], y0.dtype
    w = _weight(mode, coefs, W, U)
    g64 = g.double()
    drift = (ca * f.double()) * CF
    want = (y0.double() + drift) + CG * (g64 * w.unsqueeze(1)).sum(-1)
    S = y0.double().abs() + drift.abs() + abs(CG) * (g64.abs() * w.abs().unsqueeze(1)).sum(-1)
    bound = (m + 16) * UNIT[dtype] * S * (2.0 if dtype == torch.float64 else 1.0)
    err = (got.double() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    WORST[label] = max(WORST.get(label, 0.0), ratio)
    print(f"RATIO {label} {what} mode {mode}: error / bound = {ratio:.4f}")
    bad = err > bound
    assert not bad.any(), (f"{what} mode {mode}: {int(bad.sum())} elements outside the bound, worst error / bound "
                           f"{ratio:.3f} at flat index {int((err / bound.clamp_min(1e-300)).argmax())}")


def _operands(B, d, m, dtype, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    y0 = torch.randn(B, d, generator=gen, device=DEV, dtype=dtype)
    f = torch.randn(B, d, generator=gen, device=DEV, dtype=dtype)
    g = torch.randn(B, d, m, generator=gen, device=DEV, dtype=dtype)
    return y0, f, g


def _case_id(c):
    return f"{c.expect[0]}{'-nc%d' % c.expect[1] if c.expect[0] == 'rows' else ''}-B{c.B}-d{c.d}-m{c.m}" + \
        (f"-{c.view}_view" if c.view else "")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", H.CASES, ids=_case_id)
def test_small_batches_against_float64(case, dtype):
    """Every shape of the table at B = 1 and B = 37 (one row per wave), each weight mode, generated and external increments
    (bit-equal), aligned and offset outputs (bit-equal)."""
    K = _K()
    B, d, m = case.B, case.d, case.m
    y0, f, g = _operands(B, d, m, dtype, 1000 * B + 10 * d + m)
    if case.view == "g":
        g = _offset_view(g)
        assert g.data_ptr() % 16 != 0
    label = case.expect[0] + ("-f64" if dtype == torch.float64 else "-f32")
    for mode, coefs in MODES:
        spec = _spec(B, m, dtype, elem0=2 if case.view == "dW" else 0)
        W, U = spec.materialise(need_U=True)
        got = _launch(y0, f, g, mode, coefs, spec)
        _check_bound(got, y0, f, g, mode, coefs, W, U, label, _case_id(case))
        ext = K.NoiseSpec.external(*((_offset_view(W), _offset_view(U)) if case.view == "dW" else (W, U)))
        assert torch.equal(_launch(y0, f, g, mode, coefs, ext), got), f"mode {mode}: external increments differ"
        assert torch.equal(_launch(y0, f, g, mode, coefs, spec, layout="offset"), got), f"mode {mode}: offset output"
        assert torch.equal(_launch(y0, f, g, mode, coefs, ext, layout="offset"), got), f"mode {mode}: offset, external"


# ---- the ladder of rows per wave ---------------------------------------------------------------------------------------
_LADDER_PARAMS = [(lad, dt) for lad in H.LADDER for dt in lad.dtypes]


@pytest.fixture(scope="module", params=_LADDER_PARAMS,
                ids=[f"nc{lad.nc}-rw{lad.rw}-B{lad.B}-d{lad.d}-m{lad.m}-{dt}" for lad, dt in _LADDER_PARAMS])
def ladder(request):
    """A ladder case: its operands and the big launch on generated increments in each weight mode; nothing changes them."""
    lad, dtype = request.param[0], getattr(torch, request.param[1])
    y0, f, g = _operands(lad.B, lad.d, lad.m, dtype, lad.B + lad.d)
    full = [_launch(y0, f, g, mode, coefs, _spec(lad.B, lad.m, dtype)) for mode, coefs in MODES]
    yield lad, dtype, (y0, f, g), full
    del y0, f, g, full
    torch.cuda.empty_cache()


def test_rows_per_wave_against_float64(ladder):
    """RW = 2 ... 64 with a ragged last group: every row of the big launch within the bound; external increments and an
    offset output give the same bits."""
    K = _K()
    lad, dtype, (y0, f, g), full = ladder
    label = f"rows-rw>1-{'f64' if dtype == torch.float64 else 'f32'}"
    W, U = _spec(lad.B, lad.m, dtype).materialise(need_U=True)
    for (mode, coefs), big in zip(MODES, full):
        _check_bound(big, y0, f, g, mode, coefs, W, U, label, f"nc{lad.nc} rw{lad.rw}")
        ext = K.NoiseSpec.external(W, U)
        assert torch.equal(_launch(y0, f, g, mode, coefs, ext, layout="offset"), big), f"mode {mode} {coefs}: external"


def test_shards_are_the_rows_of_the_big_launch(ladder):
    """37 rows launched alone (elem0 = lo * m: one row per wave) are, bit for bit, those rows of the launch that shares a
    Philox call among RW rows: a row that picked up a neighbour's increments, or a ragged group whose last row got none,
    cannot pass."""
    lad, dtype, (y0, f, g), full = ladder
    n = H.SHARD_ROWS
    for lo in H.shard_ranges(lad):
        for (mode, coefs), big in zip(MODES, full):
            part = _launch(y0[lo:lo + n], f[lo:lo + n], g[lo:lo + n], mode, coefs,
                           _spec(n, lad.m, dtype, elem0=lo * lad.m))
            same = (part == big[lo:lo + n]).all(dim=1)
            assert same.all(), (f"rows [{lo}, {lo + n}) mode {mode}: rows {(lo + torch.nonzero(~same).flatten()).tolist()} "
                                f"differ from the launch of {lad.B} rows (RW = {lad.rw})")


# ---- edges ---------------------------------------------------------------------------------------------------------------
def test_more_channels_than_the_launcher_stages_is_an_error():
    from torchsde_amd import _native
    c = H.ERROR_CASE
    y0, f, g = _operands(c.B, c.d, c.m, torch.float32, 5)
    with pytest.raises(_native.NativeLibraryError):
        with torch.no_grad():
            _K().step_general(y0, f, g, CF, CG, _spec(c.B, c.m, torch.float32))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_empty_batch_launches_nothing(dtype):
    K = _K()
    y0, f, g = _operands(0, 32, 16, dtype, 6)
    with torch.no_grad():
        a = K.step_general(y0, f, g, CF, CG, _spec(0, 16, dtype))
        b = K.step_general_weighted(y0, f, g, 1 / 3, CF, CG, 2, 1.0, -1.0, RDT, _spec(0, 16, dtype))
    torch.cuda.synchronize()
    assert a.shape == b.shape == (0, 32)


def test_device_resident_coefficients_give_the_bits_of_numbers():
    """cf and 1 / dt read from device memory (adaptive stepping), rows kernel NC = 2, float32, all weight modes."""
    from torchsde_amd import _native
    B, d, m = 37, 32, 16
    cf = 0.07
    y0, f, g = _operands(B, d, m, torch.float32, 7)
    table = torch.tensor([cf, 1.0 / cf], dtype=torch.float32, device=DEV)
    for mode, coefs in MODES:
        want = _launch(y0, f, g, mode, coefs, _spec(B, m, torch.float32), cf=cf, rdt=1.0 / cf)
        got = _launch(y0, f, g, mode, coefs, _spec(B, m, torch.float32), cf=_native.dev_scalar(table, 0),
                      rdt=_native.dev_scalar(table, 1))
        assert torch.equal(got, want), f"mode {mode}"
