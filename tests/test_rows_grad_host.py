"""Row-coupled systems under autograd, the host side (no GPU): the differentiable column interpretation
(recognise_rows.recognise_rows(..., differentiable=True)), the generated tangent units (specialise.source_rows_sens: compiled
for gfx950, one entry point, no scratch), the backward contraction of kernels._RowsTrajectoryFn, and -- for
test_gpu_rows_grad.py -- that the float64-oracle criterion bites on the chosen inputs."""
import re
import subprocess

import pytest
import torch
from torch import nn

from tests import helpers
from tests import helpers_rows_grad as H
from torchsde_amd import _native, kernels, recognise, recognise_rows, specialise
from torchsde_amd.sde import ForwardSDE


def _recognise(sde, d, **kw):
    return recognise_rows.recognise_rows(ForwardSDE(sde), torch.tensor(0.3), torch.randn(7, d), **kw)


# ---- 1. recognition -------------------------------------------------------------------------------------------------------------
def test_trainable_scalars_lead_back_to_the_users_tensors():
    sde = H.ForcedVanDerPol()
    found = _recognise(sde, 2, differentiable=True)
    assert len(found.sources) == 3 and all(a is b for a, b in zip(found.sources, (sde.mu, sde.amp, sde.sigma)))
    assert found.trainable == [(0, 0), (1, 0), (2, 0), (2, 1)]
    assert found.slots() == (0, 1, 2, 3) and found.untrainable is None
    assert found.reaches(list(sde.parameters()))
    assert torch.equal(found.const_table(), torch.tensor([1.5, 0.4, 0.2, 0.3]))
    assert found.structure() == _recognise(sde, 2).structure()

    sde = H.Lorenz()
    found = _recognise(sde, 3, differentiable=True)
    # `a1, a2, a3 = self.a`: three 0-d tensors autograd saw the code derive from the parameter; `y * self.b`: the parameter
    assert found.trainable == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2)]
    assert found.sources[3] is sde.b
    for k in range(3):
        assert found.sources[k].dim() == 0 and found.sources[k].grad_fn is not None
        onehot, = torch.autograd.grad(found.sources[k], sde.a, retain_graph=True)
        assert torch.equal(onehot, torch.eye(3)[k])
    assert found.reaches(list(sde.parameters()))
    assert torch.equal(found.const_table(), torch.cat([sde.a.detach(), sde.b.detach()]))
    assert found.structure() == _recognise(sde, 3).structure()
    # a constant used twice is one trainable scalar, one tangent slot

    class Twice(H.Lorenz):
        def g(self, t, y):
            return y * self.b + self.b
    found = _recognise(Twice(), 3, differentiable=True)
    assert len(found.consts) == 9 and len(found.trainable) == 6 and sorted(found.slots()) == [0, 1, 2, 3, 3, 4, 4, 5, 5]


def test_the_plain_interpretation_is_what_it_was():
    """`structure()` keys the compiled units in users' caches: the Lorenz system's, spelled out."""
    found = _recognise(H.Lorenz(), 3)
    assert found.sources == [] and found.trainable == [] and found.slots() == (-1,) * 6
    assert found.structure() == (
        ("rows", 3, (("sub", ("x.v[1]", "x.v[0]")), ("mul", ("c[0]", "n0")), ("mul", ("c[1]", "x.v[0]")), ("sub", ("n2", "x.v[1]")),
                     ("mul", ("x.v[0]", "x.v[2]")), ("sub", ("n3", "n4")), ("mul", ("x.v[0]", "x.v[1]")), ("mul", ("c[2]", "x.v[2]")),
                     ("sub", ("n6", "n7")), ("mul", ("x.v[0]", "c[3]")), ("mul", ("x.v[1]", "c[4]")), ("mul", ("x.v[2]", "c[5]"))),
         ("n1", "n5", "n8", "n9", "n10", "n11")), ("consts", 6))


def test_stop_gradients_and_clamp_are_refused_with_the_reason():
    class Detached(H.Lorenz):
        def f(self, t, y):
            return super().f(t, y.detach())

    class Clamped(H.Lorenz):
        def g(self, t, y):
            return torch.clamp(y, min=0) * self.b
    with pytest.raises(recognise.NotElementwise, match="stop-gradient"):
        _recognise(Detached(), 3, differentiable=True)
    _recognise(Detached(), 3)                                # (no gradient asked for: the detach is a view)
    with pytest.raises(recognise.NotElementwise, match="clamp with autograd recording"):
        _recognise(Clamped(), 3, differentiable=True)


def test_a_parameter_no_constant_reaches_keeps_the_solve_off_the_route():
    class Hidden(H.Lorenz):
        def __init__(self):
            super().__init__()
            self.shift = nn.Parameter(torch.tensor(0.5))

        def g(self, t, y):
            return y * self.b + float(self.shift.detach())         # (read on the host: a number, no way back to the parameter)
    sde = Hidden()
    found = _recognise(sde, 3, differentiable=True)
    assert not found.reaches(list(sde.parameters()))
    sde.shift.requires_grad_(False)
    assert found.reaches(list(sde.parameters()))


def test_the_size_rule():
    f32, f64 = torch.float32, torch.float64
    assert specialise.rows_sens_refusal(3, 9, _native.TRAJ_EULER, f32) is None          # Lorenz, six parameters and y0
    assert specialise.rows_sens_refusal(3, 9, _native.TRAJ_EULER, f64) is None
    assert "more than the 14" in specialise.rows_sens_refusal(3, 9, _native.TRAJ_SRK, f32)
    assert specialise.rows_sens_refusal(2, 6, _native.TRAJ_SRK, f32) is None            # Van der Pol, four parameters and y0
    assert specialise.rows_sens_refusal(8, 9, _native.TRAJ_EULER, f32) is None
    assert "more than the 84" in specialise.rows_sens_refusal(8, 10, _native.TRAJ_EULER, f32)
    assert "more than 16" in specialise.rows_sens_refusal(2, 17, _native.TRAJ_EULER, f32)
    assert specialise.rows_sens_refusal(3, 9, _native.TRAJ_MILSTEIN_ITO, f32) is not None


def test_every_admitted_unit_of_the_recorded_listing_fits():
    """profiles/rows_sens_resource_usage.txt holds the dense worst-case unit of every (scheme, dtype, d, NT) the caps admit,
    d = 2 .. 8, and none of them has scratch or spilled vector registers."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rows_sens_resource_usage.txt")
    rows = {}
    for line in open(path):
        m = re.match(r"(\w+) (\d+) (\d+) \d+ (float\d+) : .*ScratchSize \[bytes/lane\] (\d+), .*VGPRs Spill (\d+),", line)
        if m:
            rows[(m.group(1), int(m.group(2)), int(m.group(3)), m.group(4))] = int(m.group(5)) + int(m.group(6))
    for name, method in SCHEMES.items():
        for column, dtype in enumerate(("float32", "float64")):
            cap = specialise.ROWS_SENS_CAP[method][column]
            for d in range(2, 9):
                for nt in range(1, min(specialise.ROWS_SENS_MAX_TANGENTS, cap // d - 1) + 1):
                    assert rows[(name, d, nt, dtype)] == 0, (name, d, nt, dtype)


# ---- 2. the generated units -----------------------------------------------------------------------------------------------------
def _exports(path):
    listed = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in listed.splitlines() if "tsde_specialised" in line)


SCHEMES = {"euler": _native.TRAJ_EULER, "midpoint": _native.TRAJ_MIDPOINT, "heun": _native.TRAJ_HEUN,
           "euler_heun": _native.TRAJ_EULER_HEUN, "srk": _native.TRAJ_SRK}


def _compiles_clean(text, tmp_path):
    src, out = tmp_path / "unit.hip", tmp_path / "unit.so"
    src.write_text(text)
    done = subprocess.run(specialise._compile_command("gfx950", str(out), str(src)) + ["-Rpass-analysis=kernel-resource-usage"],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert _exports(str(out)) == ["tsde_specialised_rows_sens_launch"]
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", done.stderr) == ["0"], done.stderr[-1500:]
    assert re.findall(r"VGPRs Spill: (\d+)", done.stderr) == ["0"], done.stderr[-1500:]


def test_the_lorenz_tangent_unit_compiles_exports_one_entry_point_and_has_no_scratch(tmp_path):
    found = _recognise(H.Lorenz(), 3, differentiable=True)
    text = specialise.source_rows_sens(found.structure(), 6, torch.float32, _native.TRAJ_EULER, found.slots(), True)
    assert "RowTan<T, 3, 9>" in text and "tan_seed<8, T, 9>(c[5])" in text
    _compiles_clean(text, tmp_path)


# the dense worst case at the largest NT each cap admits: the widest row, and the narrower rows that set float32 caps
@pytest.mark.parametrize("d", [8, 7, 5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_the_dense_unit_at_the_cap_compiles_exports_one_entry_point_and_has_no_scratch(scheme, dtype, d, tmp_path):
    method = SCHEMES[scheme]
    cap = specialise.ROWS_SENS_CAP[method][0 if dtype == torch.float32 else 1]
    nt = min(specialise.ROWS_SENS_MAX_TANGENTS, cap // d - 1)
    if nt < 1:              # (SRK in float32, cap 14: no system of 7 or 8 channels is admitted at all)
        assert specialise.rows_sens_refusal(d, 1, method, dtype) is not None
        return
    assert specialise.rows_sens_refusal(d, nt, method, dtype) is None and specialise.rows_sens_refusal(d, nt + 1, method, dtype)
    structure, n_const, slots, y0_grad = H.dense_system(d, nt)
    _compiles_clean(specialise.source_rows_sens(structure, n_const, dtype, method, slots, y0_grad), tmp_path)


def test_the_value_statements_are_those_of_the_plain_unit():
    """Statement by statement the tangent unit is `source_rows`'s unit: a binary operation the same expression on `Tan` operands
    (whose value part is that expression: csrc/trajectory.hip), a function its `d_` helper from the one table of slope rules,
    and a statement neither the state nor a trainable constant reaches the plain statement itself. Hence the same `ys`."""
    found = _recognise(H.ForcedVanDerPol(), 2, differentiable=True)
    plain = specialise.source_rows(found.structure(), 4, torch.float32, _native.TRAJ_EULER)
    dual = specialise.source_rows_sens(found.structure(), 4, torch.float32, _native.TRAJ_EULER, found.slots(), True)

    def spell(o):
        return f"x{o[4]}" if o.startswith("x.v[") else f"k{o[2]}" if o.startswith("c[") else o
    assert len(found.statements) >= 10
    for name, op, operands in found.statements:
        expression = specialise._ROW_OPS[op].format(*operands)
        assert f"const T {name} = {expression};" in plain
        if len(operands) == 2:
            assert (f"const N {name} = {specialise._ROW_OPS[op].format(*[spell(o) for o in operands])};" in dual
                    or f"const T {name} = {expression};" in dual), name
        else:
            assert f"const N {name} = d_{op}({spell(operands[0])});" in dual or f"const T {name} = {expression};" in dual, name
    assert "const T n" in dual and "d_sigmoid" in dual and "d_tanh" in dual and "d_square" in dual     # (sin(t) stays plain)
    for rule in re.findall(r"Dual<T> (d_\w+)", specialise._DUAL_HELPERS):
        assert f"Tan<T, NT> {rule}(const Tan<T, NT>& s)" in dual


# ---- 3. the backward contraction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y0_grad", [True, False])
def test_the_backward_contraction_is_the_transpose_of_the_linear_map(y0_grad):
    gen = torch.Generator().manual_seed(5)
    n_out, rows, d = 3, 5, 2
    shapes = [(), (1,), (2, 2)]                       # a 0-d source, a one-element one, one with several trainable elements
    trainable = [(0, 0), (2, 3), (1, 0), (2, 0)]      # (source, flat element) in slot order; elements 1, 2 of the last: untouched
    d0 = d if y0_grad else 0
    sens = torch.randn(n_out, d0 + len(trainable), rows, d, generator=gen, dtype=torch.float64)
    gys = torch.randn(n_out + 1, rows, d, generator=gen, dtype=torch.float64)
    y0 = torch.randn(rows, d, generator=gen, dtype=torch.float64, requires_grad=True)
    sources = [torch.randn(shape, generator=gen, dtype=torch.float64, requires_grad=True) for shape in shapes]

    # ys as the linear function of (y0, sources) whose Jacobian `sens` is
    scalars = torch.stack([sources[s].reshape(-1)[j] for s, j in trainable])
    later = torch.einsum("jkrc,k->jrc", sens[:, d0:], scalars)
    if y0_grad:
        later = later + torch.einsum("jkrc,rk->jrc", sens[:, :d0], y0)
    ys = torch.cat([(y0 if y0_grad else y0.detach()).unsqueeze(0), later])
    want = torch.autograd.grad((ys * gys).sum(), ([y0] if y0_grad else []) + sources)
    grad_y0, grads = kernels.rows_sens_contract(gys, sens, d0, trainable, shapes)
    if y0_grad:
        torch.testing.assert_close(grad_y0, want[0], rtol=1e-12, atol=1e-12)
    else:
        assert grad_y0 is None
    for got, expected, shape in zip(grads, want[-3:], shapes):
        assert tuple(got.shape) == shape
        torch.testing.assert_close(got, expected, rtol=1e-12, atol=1e-12)
    assert grads[2].reshape(-1)[1] == 0 and grads[2].reshape(-1)[2] == 0


# ---- the criterion of test_gpu_rows_grad.py bites ---------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(H.CASES)), ids=[c.id for c in H.CASES])
def test_the_oracle_criterion_bites_on_these_inputs(index):
    case = H.CASES[index]
    out = H.oracle(index)
    ys32, grads32 = out[torch.float32]
    ys64, grads64 = out[torch.float64]
    for label, _ in case.cotangents():
        for (name, a32), (_, a64) in zip(H.quantities(case, ys32, grads32[label]), H.quantities(case, ys64, grads64[label])):
            # the float32 oracle's own error is there to compare against ...
            assert (a32.double() - a64).abs().max() > 0, (label, name)
            if name == "ys":
                continue
            # ... a gradient off by one part in a thousand is rejected at the factor ...
            with pytest.raises(AssertionError):
                helpers.assert_within_reference_rounding(a32 * 1.001, a32, a64, factor=H.ROWS_GRAD_FACTOR, floor=H.ROWS_GRAD_FLOOR)
            # ... and so are two scalars' gradients exchanged
            if a32.numel() in (2, 3, 4):
                swapped = a32.reshape(-1)[[1, 0] + list(range(2, a32.numel()))].reshape(a32.shape)
                with pytest.raises(AssertionError):
                    helpers.assert_within_reference_rounding(swapped, a32, a64, factor=H.ROWS_GRAD_FACTOR, floor=H.ROWS_GRAD_FLOOR)
