"""Training through ``sdeint`` on the perceptron kernels on ANY output grid (run with ``-m gpu``): outputs inside steps, several in
one step, one inside the first step, a ragged last step -- `kernels._MlpTrajectoryFn` behind ``sdeint`` on
`MLPDriftDiagonalSDE`, `kernels._MlpLogqpTrajectoryFn` behind ``sdeint(..., logqp=True)`` on an unchanged user module
(tsde_trajectory_mlp_diag_backward_weighted, tsde_trajectory_mlp_diag_logqp_backward_weighted).

A. the route is taken and the values are those of the no-grad one-launch solve, bit for bit;
B. values and gradients against the float64 oracle (autograd through the oracle's stepwise solver, which interpolates as
   interp.py:15-18 does) through `helpers.assert_within_reference_rounding` with the measured factor of
   tests/helpers_interp_backprop.py; tests/test_interp_backprop_host.py shows on the CPU what that criterion rejects;
C. chunks and re-run chunks are invisible, with outputs around every chunk edge;
D. solves whose outputs all sit on boundaries give what the build before this route gave, bit for bit (tests/golden/);
E. two row shards equal the rows of the whole.

(Under plain ``sdeint`` an unchanged user module has no perceptron route with autograd recording, on any grid: the user-module
case is the ``logqp=True`` one.)"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import helpers_interp_backprop as I
from tests import helpers_logqp as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLAIN, LOGQP = I.plain_cases(), I.kl_cases()
CASES = PLAIN + LOGQP
MID = (37, 20, 36)


@functools.lru_cache(maxsize=None)
def _oracle(index):
    """Computed once per case, shared, never written to."""
    return I.oracle(CASES[index])


def _find(route, grid, shape=MID, method="euler", diffusion="sigmoid"):
    return next(c for c in CASES if (c.route, c.grid, (c.B, c.d, c.hidden), c.method, c.diffusion) ==
                (route, grid, shape, method, diffusion) and getattr(c, "sde_type", "ito") == "ito")


def _close(got, want, what, tol):
    err = (got.double().cpu() - want.double().cpu()).abs().max().item()
    scale = want.abs().max().item()
    print(f"{what}: max error {err:.3e} at scale {scale:.3e}")
    assert err <= tol * scale + 1e-7, f"{what}: max error {err:.3e} vs scale {scale:.3e}"


# ---- A. route and values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", I.INSIDE_GRIDS)
def test_the_published_module_trains_on_the_kernels_on_grids_that_interpolate(grid):
    case = _find("plain", grid)
    sde = case.module().to(DEV)
    ys, _ = I.plain_call(case, sde, DEV)
    assert type(ys.grad_fn).__name__.startswith(I.PLAIN_FN), type(ys.grad_fn).__name__
    with torch.no_grad():
        sampled, _ = I.plain_call(case, sde, DEV, y0=case.y0().to(DEV))
    assert sampled.grad_fn is None and torch.equal(ys.detach(), sampled)          # the one-launch solve's own interpolation
    assert not torch.equal(ys[1], ys[0]) and torch.isfinite(ys).all()


@pytest.mark.parametrize("grid", I.INSIDE_GRIDS)
def test_a_user_module_with_logqp_trains_on_the_kernels_after_earning_trust_for_interpolation(grid):
    from torchsde_amd import trust
    case = _find("logqp", grid)
    sde = case.module().to(DEV)
    aligned = I.grid_ts("aligned")
    for i in range(2):                                   # trust on an aligned grid: verified, then taken
        ys, log_ratio, _ = I.kl_call(case, sde, DEV, ts=aligned)
        assert L.graph_has(ys, I.KL_FN) == (i == 1)
    marked = lambda: [k for k in trust.book_of(sde)["trusted"] if "interpolated outputs" in k]        # noqa: E731
    assert marked() == []
    first = I.kl_call(case, sde, DEV)                      # ... does not cover the new sweep: both routes, the stepwise result
    assert not L.graph_has(first[0], I.KL_FN) and not L.graph_has(first[1], I.KL_FN)
    assert len(marked()) == 1 and trust.book_of(sde)["trusted"][marked()[0]] is True, trust.book_of(sde)["trusted"]
    ys, log_ratio, _ = I.kl_call(case, sde, DEV)
    assert L.graph_has(ys, I.KL_FN) and L.graph_has(log_ratio, I.KL_FN)
    _close(ys, first[0], "against the stepwise route, ys", 5e-4)
    _close(log_ratio, first[1], "against the stepwise route, log_ratio", 5e-4)
    for _ in range(2):                                   # the no-grad solve: verified, then one launch
        with torch.no_grad():
            sampled = I.kl_call(case, sde, DEV, y0=case.y0().to(DEV))
    assert torch.equal(ys.detach(), sampled[0]) and torch.equal(log_ratio.detach(), sampled[1])
    assert any("tsde_trajectory_mlp_diag_logqp_backward_weighted" in line for line in trust.describe(sde)), trust.describe(sde)


# ---- B. values and gradients against the float64 oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.id for c in CASES])
def test_values_and_gradients_are_the_float64_oracles_to_float32_rounding(index):
    case = CASES[index]
    ref = _oracle(index)
    if case.route == "logqp":
        assert ref["min_g"] >= L.MIN_DIFFUSION, f"the reference run meets |g| = {ref['min_g']:.3e}: an ill-conditioned case"
    got = I.solve(case, DEV)
    assert set(got) == {entry[0] for entry in case.cotangents()}
    records, failures = I.compare(got, ref)
    for what, err_new, err_ref, ratio in records:
        print(f"{case.id} {what}: err {err_new:.3e} ref {err_ref:.3e} ratio {ratio:.2f}")
    assert len(records) == len(got) * len(got["all"])
    assert not failures, "\n".join(failures)


# ---- C. chunking is invisible -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [MID, (129, 4, 16)], ids=["37x20x36", "129x4x16"])
@pytest.mark.parametrize("route", ["plain", "logqp"])
def test_chunks_and_rerun_chunks_are_invisible_with_outputs_around_every_chunk_edge(route, shape, monkeypatch):
    from torchsde_amd import kernels
    case = _find(route, "chunk_edges", shape)
    fn = kernels._MlpTrajectoryFn if route == "plain" else kernels._MlpLogqpTrajectoryFn
    whole = I.solve(case, DEV)
    results = {}
    for variant in ("chunked", "re-run"):
        with monkeypatch.context() as m:
            m.setattr(fn, "STASH_BYTES", 5 * case.B * (case.d + 2 * case.hidden) * 4)       # chunk tops 16, 11, 6, 1
            if variant == "re-run":
                m.setattr(fn, "STATE_BYTES", 1)
            assert fn._chunk(I.STEPS, case.B, case.d, case.hidden) == 5
            results[variant] = I.solve(case, DEV)
    for variant, got in results.items():
        for label in whole:
            for name in ("ys", "log_ratio", "y0"):
                if name in whole[label]:
                    assert torch.equal(got[label][name], whole[label][name]), (variant, label, name)
            for name, want in whole[label].items():
                _close(got[label][name], want, f"{variant} {label} {name}", 1e-4)


# ---- D. unchanged behaviour -------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interp_backprop_parent.npz")


@pytest.mark.parametrize("grid", ["aligned", "every_step"])
@pytest.mark.parametrize("scheme", ["euler-sigmoid", "milstein-affine"])
@pytest.mark.parametrize("route", ["plain", "logqp"])
def test_boundary_only_solves_are_bit_for_bit_those_of_the_build_before_this_route(route, scheme, grid):
    """tests/golden/make_interp_backprop_parent.py recorded these on the parent build, same seeds."""
    from tests.golden import make_interp_backprop_parent as G
    recorded = np.load(GOLDEN)
    got = G.solve(route, scheme, grid, DEV)
    keys = [k for k in recorded.files if k.startswith(f"{route}/{scheme}/{grid}/")]
    assert sorted(keys) == sorted(f"{route}/{scheme}/{grid}/{name}" for name in got) and len(keys) >= 8
    for name, value in got.items():
        want = torch.from_numpy(recorded[f"{route}/{scheme}/{grid}/{name}"])
        assert torch.equal(value.cpu(), want), (route, scheme, grid, name, (value.cpu() - want).abs().max().item())


# ---- E. sharding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["plain", "logqp"])
def test_shards_equal_the_rows_of_the_whole(route):
    case = _find(route, "inside")
    sde = case.module().to(DEV)
    y0_all = case.y0().to(DEV)
    cot = case.cotangents()[0][1:]

    def run(rows, offset):
        for _ in range(2):       # (KL, per batch size: the verifying solve, then the trusted one)
            y0 = y0_all[offset:offset + rows].clone().requires_grad_(True)
            if route == "plain":
                outs = [I.plain_call(case, sde, DEV, y0=y0, rows=rows, row_offset=offset)[0]]
            else:
                outs = list(I.kl_call(case, sde, DEV, y0=y0, rows=rows, row_offset=offset)[:2])
        assert L.graph_has(outs[0], I.PLAIN_FN if route == "plain" else I.KL_FN)
        grad, = torch.autograd.grad(outs, [y0], grad_outputs=[w[:, offset:offset + rows].to(DEV) for w in cot])
        return [o.detach() for o in outs] + [grad]

    whole = run(case.B, 0)
    for rows, offset in ((20, 0), (17, 20)):
        part = run(rows, offset)
        for a, b in zip(part[:-1], whole[:-1]):
            assert torch.equal(a, b[:, offset:offset + rows]), (rows, offset)
        assert torch.equal(part[-1], whole[-1][offset:offset + rows]), (rows, offset)
