"""The column interpreter on diffusion MATRICES (torchsde_amd/recognise_rows.py `recognise_rows(..., m=m)`: general, scalar and
additive noise) and the unit specialise.source_rows_general generates from it (CPU: no kernel is launched)."""
import concurrent.futures
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from tests import helpers_rows_general as H
from tests.test_recognise_rows import _evaluate as _evaluate_columns
from torchsde_amd import _native, recognise_rows, specialise
from torchsde_amd.recognise import NotElementwise
from torchsde_amd.sde import ForwardSDE
from workloads.problems import StochasticLorenz as _Lorenz

SCHEMES = {"euler": _native.TRAJ_EULER, "midpoint": _native.TRAJ_MIDPOINT, "heun": _native.TRAJ_HEUN,
           "euler_heun": _native.TRAJ_EULER_HEUN}
LISTING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "rows_general_resource_usage.txt")


def _evaluate(found, y, t):
    """The linearised statements evaluated in torch (tests/test_recognise_rows._evaluate): the drift (rows, d) and the d * m
    diffusion outputs, row-major, as the matrix (rows, d, m)."""
    f, entries = _evaluate_columns(found, y, t)
    return f, entries.reshape(y.shape[0], found.d, found.m)


def _probe(sde, rows=7, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(rows, sde.d, dtype=torch.float64, generator=gen) + 0.3     # (positive: Heston takes a square root)


_ROUNDED_ONCE = {"add", "sub", "mul", "neg", "square", "cube"}      # (integer powers are expanded into products)


def _only_sums_and_products(found):
    """Per output, whether its expression holds only + - x: those must reproduce the module's own bits."""
    made = {name: (op, operands) for name, op, operands in found.statements}
    memo = {}

    def exact(o):
        if o not in made:
            return True
        if o not in memo:
            op, operands = made[o]
            memo[o] = op in _ROUNDED_ONCE and all(exact(x) for x in operands)
        return memo[o]
    return [exact(o) for o in found.outputs]


def _assert_reproduces(found, sde, y, t):
    """`torch.equal` for every output that holds only + - x, rtol 1e-12 where a function occurs; returns the exact flags of
    the drift and of the matrix."""
    f, g = _evaluate(found, y, t)
    with torch.no_grad():
        want_f, want_g = sde.f(t, y), sde.g(t, y).reshape(y.shape[0], -1)
    got = torch.cat([f, g.reshape(y.shape[0], -1)], dim=1)
    want = torch.cat([want_f, want_g], dim=1)
    flags = _only_sums_and_products(found)
    assert got.shape == want.shape and len(flags) == got.shape[1]
    for c, exact in enumerate(flags):
        if exact:
            assert torch.equal(got[:, c], want[:, c]), (c, found.outputs[c])
        else:
            torch.testing.assert_close(got[:, c], want[:, c], rtol=1e-12, atol=0)
    return flags[:found.d], flags[found.d:]


# what must come out bit for bit: the outputs of these modules hold only + - x
_EXACT = {"heston": ("f",), "langevin": ("f",), "langevin_untimed": ("f", "g")}


@pytest.mark.parametrize("name", sorted(H.modules()))
def test_the_matrix_is_followed_entry_by_entry(name):
    sde = H.modules()[name]("ito").double()
    y, t = _probe(sde), torch.tensor(0.3, dtype=torch.float64)
    found = recognise_rows.recognise_rows(ForwardSDE(sde), t, y, m=sde.m)
    assert (found.d, found.m) == (sde.d, sde.m) and len(found.outputs) == sde.d + sde.d * sde.m
    assert found.structure()[0][:3] == ("rows_general", sde.d, sde.m)
    assert found.spec()[0] == "program_rows_general" and found.spec()[3:] == (sde.d, sde.m)
    exact_f, exact_g = _assert_reproduces(found, sde, y, t)
    assert all(exact_f) or "f" not in _EXACT.get(name, ())
    assert all(exact_g) or "g" not in _EXACT.get(name, ())
    again = recognise_rows.recognise_rows(ForwardSDE(sde), t, y, rows=5, m=sde.m)
    assert again.structure() == found.structure()
    # the constants are this solve's live values: another interpretation after an optimiser step reproduces the changed module
    before = found.const_table().clone()
    with torch.no_grad():
        for p in sde.parameters():
            p.mul_(1.25)
    changed = recognise_rows.recognise_rows(ForwardSDE(sde), t, y, m=sde.m)
    assert changed.structure() == found.structure() and not torch.equal(changed.const_table(), before)
    assert _assert_reproduces(changed, sde, y, t) == (exact_f, exact_g)


class _Ops(nn.Module):
    """d = 2; `g` is the expression under test, over y, t, B and an asymmetric (2, 2) parameter A."""
    noise_type, sde_type, d = "general", "ito", 2

    def __init__(self, code):
        super().__init__()
        self.code = code
        self.A = nn.Parameter(torch.tensor([[0.3, -0.2], [0.7, 1.1]], dtype=torch.float64))

    def f(self, t, y):
        return -y

    def g(self, t, y):
        B = y.shape[0]
        return eval(self.code)


@pytest.mark.parametrize("code,m", [
    ("torch.stack([y * 2, y.tanh(), -y], dim=2)", 3),                                           # stack along dim 2
    ("torch.stack([y * 2, y * y], dim=-1)", 2),
    ("torch.cat([torch.stack([y, y * y], dim=2), (y * 3).unsqueeze(-1)], dim=2)", 3),            # cat along dim 2
    ("torch.cat([(y * 3).unsqueeze(2), torch.stack([y, y * y], dim=2)], dim=-1)", 3),
    ("torch.diag_embed(y * self.A[0])", 2),                                                      # diag_embed
    ("self.A.repeat(B, 1, 1) * y.unsqueeze(-1)", 2),                                             # repeat
    ("torch.cat([y, y.sin()], dim=1).unflatten(1, (2, 2))", 2),                                  # unflatten
    ("torch.cat([y, y * y, y - 1], dim=1).view(-1, 2, 3)", 3),                                   # view
    ("torch.cat([y.new_zeros(B, 2, 1), torch.full_like(y, 0.5).unsqueeze(-1), y.new_ones(B, 2, 1) * y.unsqueeze(2)], dim=2)", 3),
    ("y[:, :, None] * self.A[None]", 2),                                                         # indexing with None
    ("y[:, None, :] + torch.diag_embed(y)", 2),
    ("y.unsqueeze(-1) * self.A[1].reshape(1, 1, 2)", 2),                                         # (rows, d, 1) x (1, 1, m)
    ("y.unsqueeze(2) * y.cos().unsqueeze(1)", 2),                                                # (rows, d, 1) x (rows, 1, m)
    ("(self.A * torch.exp(-t)).expand(B, 2, 2) + torch.diag_embed(y)", 2),                       # a (d, m) function of t
    ("(self.A * t).unsqueeze(0).expand(B, -1, -1) * y.unsqueeze(-1)", 2),
    ("torch.zeros_like(torch.diag_embed(y)) + y.unsqueeze(-1) - 2.0", 2),
])
def test_every_followed_operator_reproduces_the_modules_own_matrix(code, m):
    sde = _Ops(code)
    y, t = _probe(sde), torch.tensor(0.3, dtype=torch.float64)
    found = recognise_rows.recognise_rows(ForwardSDE(sde), t, y, m=m)
    assert found.m == m
    _assert_reproduces(found, sde, y, t)
    assert recognise_rows.recognise_rows(ForwardSDE(sde), t, y, rows=5, m=m).structure() == found.structure()


def test_hestons_zero_is_structural_and_its_parameters_are_live():
    sde = H.Heston()
    found = recognise_rows.recognise_rows(ForwardSDE(sde), torch.tensor(0.0), _probe(sde).float(), m=2)
    assert found.zero_mask == (False, True, False, False)
    text = specialise.source_rows_general(found.structure(), len(found.consts), torch.float32, SCHEMES["euler"])
    assert "launch_rows_general<T, METHOD, 2, 2, RowGeneralModel<T>>" in text
    # three products per stage: no term for the zero, and no matrix anywhere
    assert len(re.findall(r"\* w\[\d\]", text)) == 3 and "(T)0.0 * w" not in text
    assert re.search(r"r\.v\[0\] = n\d+ \* w\[0\];", text) and re.search(r"r\.v\[1\] = \(n\d+ \* w\[0\]\) \+ n\d+ \* w\[1\];", text)
    # a parameter the code hands over as it is stays a view: the table follows an in-place change
    before = found.const_table().clone()
    with torch.no_grad():
        sde.mu.fill_(0.25)
    after = found.const_table()
    assert not torch.equal(before, after) and 0.25 in after.tolist()


def test_langevins_upper_half_costs_nothing():
    sde = H.Langevin()
    found = recognise_rows.recognise_rows(ForwardSDE(sde), torch.tensor(0.2), _probe(sde).float(), m=2)
    assert found.zero_mask == (True,) * 4 + (False,) * 4
    text = specialise.source_rows_general(found.structure(), len(found.consts), torch.float32, SCHEMES["euler"])
    assert len(re.findall(r"\* w\[\d\]", text)) == 4 and "r.v[0] = (T)0;" in text and "r.v[1] = (T)0;" in text


def test_without_m_nothing_changes():
    y = torch.randn(7, 3)
    found = recognise_rows.recognise_rows(ForwardSDE(_Lorenz()), torch.tensor(0.3), y)
    assert found.structure()[0][0] == "rows" and len(found.structure()[0]) == 4 and found.spec()[0] == "program_rows"
    assert found.m is None and found.zero_mask is None and len(found.outputs) == 6
    assert "launch_prog_w<T, METHOD, 3, RowModel<T>>" in specialise.source_rows(found.structure(), 0, torch.float32, 0)


@pytest.mark.parametrize("code,reason", [
    ("torch.full_like(y, 0.5) * y", "full_like"),
    ("y.new_zeros(y.shape[0], 3) + y", "new_zeros"),
    ("y.unsqueeze(-1).squeeze(-1)", "unsqueeze"),
    ("torch.stack([y, y], dim=2)[:, :, 0]", "stack"),
])
def test_without_m_the_matrix_operators_are_refused_as_before(code, reason):
    class M(nn.Module):
        noise_type, sde_type = "diagonal", "ito"

        def f(self, t, y):
            return eval(code)

        def g(self, t, y):
            return 0.1 * y
    with pytest.raises(NotElementwise, match=reason):
        recognise_rows.recognise_rows(ForwardSDE(M()), torch.tensor(0.0), torch.randn(6, 3))


class _Case(nn.Module):
    noise_type, sde_type = "general", "ito"

    def __init__(self, code):
        super().__init__()
        self.code = code
        self.A = nn.Parameter(torch.eye(2))

    def f(self, t, y):
        return -y

    def g(self, t, y):
        B, s, v = y.shape[0], y[:, 0], y[:, 1]
        return eval(self.code)


def _in_place(y):
    g = torch.zeros(y.shape[0], 2, 2)
    g[:, 0, 0] = y[:, 0]
    return g


@pytest.mark.parametrize("code,m,reason", [
    ("_in_place(y)", 2, "in-place"),
    ("(y @ self.A).unsqueeze(-1).expand(B, 2, 2)", 2, "mm"),
    ("torch.stack([y, y, y], dim=2)", 2, r"\(rows, d, m\)"),
    ("torch.stack([y] * 9, dim=2)", 9, "more than 8"),
    ("torch.stack([y, y[:1].expand(B, 2)], dim=2)", 2, "picked out"),
    ("torch.stack([y, y * float(t)], dim=2)", 2, "reads t on the host"),
    ("torch.stack([y, y * torch.randn(2)], dim=2)", 2, "random"),
    ("torch.stack([y, y * torch.arange(B, dtype=y.dtype).reshape(B, 1)], dim=2)", 2, "beside columns"),
    ("torch.einsum('bi,ij->bj', y, self.A).unsqueeze(-1).expand(B, 2, 2)", 2, "permute|bmm|einsum"),
])
def test_what_is_not_matrix_assembly_is_refused(code, m, reason):
    with pytest.raises(NotElementwise, match=reason):
        recognise_rows.recognise_rows(ForwardSDE(_Case(code)), torch.tensor(0.5), torch.rand(6, 2) + 0.3, m=m)


def test_a_per_row_constant_block_is_refused():
    class PerRow(_Case):
        def g(self, t, y):
            B = y.shape[0]
            return torch.cat([torch.stack([y, y], dim=1), torch.arange(B * 2.0).reshape(B, 1, 2)], dim=1)
    with pytest.raises(NotElementwise, match="per-row constant"):
        recognise_rows.recognise_rows(ForwardSDE(PerRow("")), torch.tensor(0.5), torch.rand(6, 2), m=2)


def test_sizes_over_the_cap_and_other_schemes_are_refused(monkeypatch):
    for method in SCHEMES.values():
        for dtype in (torch.float32, torch.float64):
            cap = specialise.ROWS_GENERAL_CAP[method][0 if dtype == torch.float32 else 1]
            assert specialise.rows_general_refusal(1, 1, method, dtype) is None
            d, m = next(((d, m) for d in range(1, 9) for m in range(1, 9) if d * m > cap), (None, None))
            if d is not None:
                assert "more than the" in specialise.rows_general_refusal(d, m, method, dtype)
    monkeypatch.setitem(specialise.ROWS_GENERAL_CAP, SCHEMES["heun"], (20, 12))
    assert specialise.rows_general_refusal(4, 5, SCHEMES["heun"], torch.float32) is None
    assert "more than the 20" in specialise.rows_general_refusal(3, 7, SCHEMES["heun"], torch.float32)
    assert "more than the 12" in specialise.rows_general_refusal(4, 5, SCHEMES["heun"], torch.float64)
    assert "scheme" in specialise.rows_general_refusal(2, 2, _native.TRAJ_SRK, torch.float32)
    assert "scheme" in specialise.rows_general_refusal(2, 2, _native.TRAJ_MILSTEIN_ITO, torch.float32)


def _listing():
    """{(scheme, d, m, dtype): (scratch bytes, spilled vector registers)} and {(scheme, dtype): cap} of the committed listing."""
    rows, caps = {}, {}
    for line in open(LISTING):
        head = re.match(r"## (\w+): cap d\*m = (\d+) \(float32\), (\d+) \(float64\)", line)
        if head:
            caps[(head.group(1), "float32")], caps[(head.group(1), "float64")] = int(head.group(2)), int(head.group(3))
        row = re.match(r"(\w+) (\d+) (\d+) \d+ (float\d+) : .*ScratchSize \[bytes/lane\] (\d+),.*VGPRs Spill (\d+),", line)
        if row:
            rows[(row.group(1), int(row.group(2)), int(row.group(3)), row.group(4))] = (int(row.group(5)), int(row.group(6)))
    return rows, caps


def test_the_caps_are_the_measured_ones_and_every_admitted_pair_fits():
    rows, caps = _listing()
    assert len(rows) == len(SCHEMES) * 2 * 64
    for name, method in SCHEMES.items():
        assert specialise.ROWS_GENERAL_CAP[method] == (caps[(name, "float32")], caps[(name, "float64")])
        for dname in ("float32", "float64"):
            for d in range(1, 9):
                for m in range(1, 9):
                    if d * m <= caps[(name, dname)]:
                        assert rows[(name, d, m, dname)] == (0, 0), (name, d, m, dname)


def _largest_admitted(method, dtype):
    cap = specialise.ROWS_GENERAL_CAP[method][0 if dtype == torch.float32 else 1]
    return max(((d, m) for d in range(1, 9) for m in range(1, 9) if d * m <= cap), key=lambda p: (p[0] * p[1], p[0]))


@pytest.mark.skipif(specialise.compiler() is None, reason="no hipcc: generated units cannot be compiled here")
def test_the_generated_units_compile_for_every_scheme_and_dtype(tmp_path):
    """Dense(8, 8) -- or the largest pair a scheme's cap admits -- and Dense(3, 5): each compiles for gfx950 with the flags
    `specialise._compile` uses and exports the family's one entry point."""
    units = {}
    for name, method in SCHEMES.items():
        for dtype in (torch.float32, torch.float64):
            for d, m in {_largest_admitted(method, dtype), (3, 5)}:
                sde = H.Dense(d, m, "stratonovich")
                found = recognise_rows.recognise_rows(ForwardSDE(sde), torch.tensor(0.3), torch.rand(7, d), m=m)
                text = specialise.source_rows_general(found.structure(), len(found.consts), dtype, method)
                units[f"{name}_{d}x{m}_{str(dtype)[6:]}"] = text

    def build(item):
        name, text = item
        src, out = tmp_path / f"{name}.hip", tmp_path / f"{name}.so"
        src.write_text(text)
        done = subprocess.run(specialise._compile_command("gfx950", str(out), str(src)), capture_output=True, text=True)
        if done.returncode != 0:
            return name, done.stderr[-2000:]
        listed = subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True, check=True).stdout
        return name, sorted(line.split()[-1] for line in listed.splitlines() if "tsde_specialised" in line)
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        for name, exports in pool.map(build, units.items()):
            assert exports == [specialise._ENTRY["rows_general"][0]], (name, exports)
