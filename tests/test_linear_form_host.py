"""Host side of the affine trajectory kernel's linear form (f = rate * y: both shifts zero) and of the step loop's
scalar Philox head; no GPU. The launch plan decides once whether both shifts are all zero and hands the C entry null
shift pointers; the headed Philox entry of csrc/tsde_rng.h returns the words of the standard one."""
import ctypes
import os
import subprocess

import pytest
import torch

from tests.test_oracle_brownian import PHILOX_KAT
from torchsde_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def reads(monkeypatch):
    """Counts the device-to-host reads of `kernels.affine_plan` (each is one call of `kernels._all_zero`)."""
    seen = []
    true_read = K._all_zero

    def counting(tensor):
        seen.append(tensor)
        return true_read(tensor)

    monkeypatch.setattr(K, "_all_zero", counting)
    return seen


def _coefs(d, drift_shift, diff_shift):
    return (torch.full((d,), 0.3), drift_shift.reshape(-1).expand(d).contiguous(), torch.full((d,), 0.4),
            diff_shift.reshape(-1).expand(d).contiguous())


def test_zero_shift_tensors_are_read_once_per_plan(reads):
    d, memo = 8, {}
    b, e = torch.zeros(d), torch.zeros(())
    for _ in range(5):                                   # five solves of one plan
        plan = K.affine_plan(_coefs(d, b, e), (b, e), memo)
        assert plan.linear is True and len(plan) == 4
    assert len(reads) == 2                               # one look at each shift, at the first solve only


def test_any_non_zero_shift_element_keeps_the_general_form(reads):
    d = 8
    for where in ("drift", "diffusion"):
        b, e, memo = torch.zeros(d), torch.zeros(d), {}
        (b if where == "drift" else e)[d - 1] = 1e-30
        for _ in range(3):
            assert K.affine_plan(_coefs(d, b, e), (b, e), memo).linear is False
    assert len(reads) <= 4                               # (at most one look per tensor and plan)
    nan = torch.full((d,), float("nan"))
    assert K.affine_plan(_coefs(d, nan, nan), (nan, nan), {}).linear is False
    negative_zero = torch.full((d,), -0.0)
    assert K.affine_plan(_coefs(d, negative_zero, negative_zero), (negative_zero, negative_zero), {}).linear is True


def test_an_in_place_update_of_a_shift_is_seen_and_costs_one_more_look(reads):
    d, memo = 4, {}
    b, e = torch.zeros(d), torch.zeros(d)
    assert K.affine_plan(_coefs(d, b, e), (b, e), memo).linear is True
    b.add_(0.5)                                          # an optimiser step: the version counter moves
    assert K.affine_plan(_coefs(d, b, e), (b, e), memo).linear is False
    assert K.affine_plan(_coefs(d, b, e), (b, e), memo).linear is False
    b.zero_()
    assert K.affine_plan(_coefs(d, b, e), (b, e), memo).linear is True
    assert len(reads) <= 6 and len(reads) >= 3


def test_shifts_absent_from_the_code_need_no_look_and_numbers_decide_themselves(reads):
    d = 4
    z = torch.zeros(d)
    assert K.affine_plan(_coefs(d, z, z), (None, None), {}).linear is True
    assert K.affine_plan(_coefs(d, z, z), (0.0, 0), {}).linear is True
    assert K.affine_plan(_coefs(d, z + 0.1, z), (0.1, None), {}).linear is False
    # a value the interpretation assembled itself (a new tensor at every solve) cannot be remembered: general form
    assert K.affine_plan(_coefs(d, z, z), (NotImplemented, None), {}).linear is False
    # coefficient tables (functions of t) stay on the general, timed kernels
    tables = tuple(torch.zeros(6, d) for _ in range(4))
    assert K.affine_plan(tables, (None, None), {}).linear is False
    assert reads == []


class _Recorder:
    """Stands in for the library: keeps the arguments of the affine entry."""

    def __init__(self):
        self.calls = []

    def tsde_trajectory_affine_diag(self, *args):
        self.calls.append(args)
        return 0


class _Schedule:
    n_steps, n_out, dtype = 3, 1, torch.float32

    @staticmethod
    def struct():
        return None


class _Bm:
    _entropy_dev, _key, _elem0 = None, 5, 0


def _launch(monkeypatch, coefs, linear):
    lib = _Recorder()
    monkeypatch.setattr(K._native, "require_device", lambda *tensors: None)
    monkeypatch.setattr(K, "_launch_env", lambda y0: (lib, 0, None))
    y0 = torch.ones(2, coefs[0].numel())
    ys = torch.empty(1, *y0.shape)
    K.trajectory_affine_diag(ys, y0, *coefs, 0, _Schedule, _Bm, linear=linear)
    (args,) = lib.calls
    return args, coefs


def test_the_linear_plan_passes_null_shift_pointers_and_the_general_plan_both_arrays(monkeypatch):
    d = 4
    z = torch.zeros(d)
    plan = K.affine_plan(_coefs(d, z, z), (z, z), {})
    args, coefs = _launch(monkeypatch, plan, plan.linear)
    # (ys, y0, rows, d, drift_rate, drift_shift, diff_rate, diff_shift, ...)
    assert args[4] == coefs[0].data_ptr() and args[6] == coefs[2].data_ptr()
    assert args[5] is None and args[7] is None
    shifted = torch.tensor([0.0, 0.0, 0.25, 0.0])
    plan = K.affine_plan(_coefs(d, z, shifted), (z, shifted), {})
    args, coefs = _launch(monkeypatch, plan, plan.linear)
    assert plan.linear is False
    assert args[5] == coefs[1].data_ptr() and args[7] == coefs[3].data_ptr()


@pytest.mark.parametrize("ctr,key,expected", PHILOX_KAT)
def test_library_philox_known_answers_are_unchanged(ctr, key, expected):
    from torchsde_amd import _native
    lib = _native.load()
    out = (ctypes.c_uint32 * 4)()
    lib.tsde_philox4x32_10((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out)
    assert tuple(out) == expected


_HEADED_TWIN = r"""
#include <stdio.h>
#include "tsde_rng.h"
static int same(tsde::u32x4 a, tsde::u32x4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }
int main() {
  const uint32_t kat[3][10] = {%s};
  for (int i = 0; i < 3; ++i) {
    const tsde::u32x4 c = {kat[i][0], kat[i][1], kat[i][2], kat[i][3]}, want = {kat[i][6], kat[i][7], kat[i][8], kat[i][9]};
    if (!same(tsde::philox4x32_10_headed(c, kat[i][4], kat[i][5], tsde::philox_head(c.y, c.z, kat[i][4])), want)) return 2;
  }
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); };
  for (int i = 0; i < 100000; ++i) {
    tsde::u32x4 c = {next(), next(), next(), next()};
    if (i %% 3 == 0) c.z = 0;                      /* node 0: what the step loops draw */
    const uint32_t k0 = next(), k1 = next();
    if (!same(tsde::philox4x32_10(c, k0, k1), tsde::philox4x32_10_headed(c, k0, k1, tsde::philox_head(c.y, c.z, k0))))
      return 3;
  }
  return 0;
}
"""


def test_headed_philox_returns_the_words_of_the_standard_one_for_any_input(tmp_path):
    """csrc/tsde_rng.h compiled for the host: `philox4x32_10_headed` (the step loops' entry, rounds 0 and 1 split so the
    part that is the same for every lane is scalar work) against the Random123 vectors and against `philox4x32_10` on
    100000 random (counter, key) pairs, node 0 and not."""
    rows = ", ".join("{" + ", ".join(f"0x{w:08x}u" for w in ctr + key + expected) + "}" for ctr, key, expected in PHILOX_KAT)
    src = tmp_path / "headed.cpp"
    src.write_text(_HEADED_TWIN % rows)
    exe = tmp_path / "headed"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "torchsde_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
