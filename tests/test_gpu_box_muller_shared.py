"""The float32 two-pair Box-Muller (torchsde_amd/csrc/tsde_rng.h: `box_muller2`) evaluates the small-radius series once per
Philox call -- on whichever pair is hot, and on the second pair of a both-hot lane in a block the wave enters by a ballot --
and must return the floats the per-pair `box_muller` returns, bit for bit.

The kernels hold two independent evaluations of the same normals: a launch with 16-byte-aligned operands and n % 4 == 0
draws through `normal4` (the shared series), the same elements through operands offset by one element draw through
`normal1` (per-pair, both series evaluated). Tests A compare the two bytewise on a sample that the oracle shows to hold
every class of quad; test B compares whole solves of the two routes; test C checks the select logic itself on the CPU."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.test_box_muller_series import _f32, _fma, _series_two_folded

DEV = "cuda"
N, ENTROPY, CELL = 16384, 7, 3
HOT_FROM = 0xF0000000
HOT_R2 = -2.0 * math.log(15.0 / 16.0)      # a pair is hot when its squared radius -2 ln u1 is below this: u1 > 15/16


# ---- A: the vector path against the scalar path ---------------------------------------------------------------------
def _quad_classes(stream):
    """Quads of the sample by which of their pairs are hot, counted from the oracle's float64 normals."""
    from oracle import counter
    z = counter.normals(N, ENTROPY, elem0=0, cell=CELL, node=0, stream=stream).reshape(-1, 4)
    h0 = z[:, 0] ** 2 + z[:, 1] ** 2 < HOT_R2
    h1 = z[:, 2] ** 2 + z[:, 3] ** 2 < HOT_R2
    return {"both": int((h0 & h1).sum()), "first only": int((h0 & ~h1).sum()), "second only": int((~h0 & h1).sum()),
            "none": int((~h0 & ~h1).sum())}


def _require_every_class(stream):
    classes = _quad_classes(stream)
    print(f"stream {stream}: {classes}")
    assert sum(classes.values()) == N // 4
    assert all(count >= 8 for count in classes.values()), classes
    return classes


def _spec():
    from torchsde_amd import kernels as K
    return K.NoiseSpec((N,), torch.float32, torch.device(DEV), entropy=ENTROPY, elem0=0, cell=CELL, h=1.0)


def _buffers(k, offset):
    """k float32 vectors of N elements: 16-byte aligned (offset 0) or one element past an aligned address (offset 1)."""
    outs = []
    for _ in range(k):
        base = torch.zeros(N + 4, dtype=torch.float32, device=DEV)
        assert base.data_ptr() % 16 == 0
        outs.append(base[offset:offset + N])
        assert (outs[-1].data_ptr() % 16 == 0) == (offset == 0)
    return outs


def _increments(offset):
    """(W, U) of the sample's cell with h = 1 from the increment kernel: W is stream W's normal itself, U mixes in stream H."""
    from torchsde_amd import _native
    W, U = _buffers(2, offset)
    code = _native.load().tsde_cell_increment(W.data_ptr(), U.data_ptr(), N, _spec().struct(), _native.F32,
                                              _native.stream_ptr(torch.device(DEV)))
    _native.check(code, "tsde_cell_increment")
    torch.cuda.synchronize()
    return W, U


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.mark.gpu
def test_sample_holds_every_class_of_quad():
    assert _require_every_class(0) == {"both": 15, "first only": 220, "second only": 248, "none": 3613}


@pytest.mark.gpu
def test_step_kernel_draws_the_same_normals_on_vector_and_scalar_path():
    from torchsde_amd import kernels as K
    _require_every_class(0)
    drawn = []
    for offset in (0, 1):
        y0, f, g, out = _buffers(4, offset)
        g.fill_(1.0)
        K._raw_step_diag(y0, f, g, 0.0, 1.0, _spec(), out)      # (0 + 0 * 0) + 1 * (1 * dW): the normal itself at h = 1
        torch.cuda.synchronize()
        drawn.append(out)
    assert torch.isfinite(drawn[0]).all() and 0.9 < float(drawn[0].std()) < 1.1
    assert _bytes(drawn[0]) == _bytes(drawn[1])


@pytest.mark.gpu
def test_increment_kernel_draws_the_same_normals_on_vector_and_scalar_path_both_streams():
    from oracle import counter
    _require_every_class(0)
    _require_every_class(1)
    Wv, Uv = _increments(0)
    Ws, Us = _increments(1)
    assert _bytes(Wv) == _bytes(Ws)
    assert _bytes(Uv) == _bytes(Us)         # U = th * (W / 2 + sh * (stream H's normal)): stream H through both paths
    # and they are the oracle's normals (to the fp32 transcendental tolerance of tests/test_gpu_parity.py), so that the two
    # paths cannot agree on something else
    ref = counter.normals(N, ENTROPY, elem0=0, cell=CELL, node=0, stream=0)
    assert np.abs(Wv.cpu().numpy().astype(np.float64) - ref).max() <= 2e-5


# ---- B: through a solve -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method,sde_type", [("euler", "ito"), ("milstein", "ito"), ("midpoint", "stratonovich"),
                                             ("srk", "ito")])
def test_default_route_solve_is_bytewise_the_stepwise_solve(method, sde_type):
    import torchsde_amd
    from workloads import problems
    B, d, steps, dt = 64, 64, 3, 2.0 ** -6
    sde = problems.GBMDiag(d, sde_type).to(DEV)
    y0 = torch.full((B, d), 0.1, device=DEV)
    ts = torch.tensor([0.0, steps * dt], device=DEV)
    levy = "space-time" if method == "srk" else "none"
    solves = []
    for options in (None, {"trajectory_kernel": False}):
        bm = torchsde_amd.BrownianInterval(t0=0.0, t1=steps * dt, size=(B, d), dtype=torch.float32, device=DEV, entropy=2024,
                                           dt=dt, levy_area_approximation=levy)
        with torch.no_grad():
            solves.append(torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=dt, options=options))
    torch.cuda.synchronize()
    assert solves[0].shape == (2, B, d) and torch.isfinite(solves[0]).all()
    assert not torch.equal(solves[0][1], solves[0][0])
    assert _bytes(solves[0]) == _bytes(solves[1])


# ---- C: the select logic, on the CPU ----------------------------------------------------------------------------------
def _series(a):
    """The series value of first word `a` in exact rational arithmetic (tests/test_box_muller_series.py)."""
    w = _fma(_f32(np.float32(np.uint32(~a & 0xFFFFFFFF))), Fraction(1, 1 << 32), Fraction(1, 1 << 33))
    return ("series", _series_two_folded(w)[0])


def _log(a):
    return ("log", a)       # the log path is one opaque value per word: the selects only move it around


def _per_pair(a):
    return _series(a) if a >= HOT_FROM else _log(a)


def _two_pair_wave(lanes):
    """Mirror of `box_muller2`'s selects for the lanes (r.x, r.z) of one wave; the cold block runs only on a ballot."""
    state = []
    for a0, a1 in lanes:
        s0, s1 = _log(a0), _log(a1)
        h0, h1 = a0 >= HOT_FROM, a1 >= HOT_FROM
        ser = _series(a0 if h0 else a1)
        s0 = ser if h0 else s0
        s1 = ser if (h1 and not h0) else s1
        state.append([a1, h0 and h1, s0, s1])
    entered = any(both for _, both, _, _ in state)
    if entered:
        for lane in state:
            lane[3] = _series(lane[0]) if lane[1] else lane[3]
    return [(s0, s1) for _, _, s0, s1 in state], entered


def test_selects_return_each_pairs_own_series_or_log_value():
    edge = (0xEFFFFFFF, 0xF0000000, 0xFFFFFFFF)
    words = edge + (0, 1, 0x80000000, 0xF0000001, 0xFFFFFFFE)
    cold, hot = [a for a in words if a < HOT_FROM], [a for a in words if a >= HOT_FROM]
    assert set(edge) & set(cold) == {0xEFFFFFFF} and set(edge) & set(hot) == {0xF0000000, 0xFFFFFFFF}
    assert _series(0xF0000000) != _series(0xFFFFFFFF)         # the mirror can tell whose series a lane was given
    every = [(a0, a1) for a0 in words for a1 in words]
    no_both = [(a0, a1) for a0, a1 in every if not (a0 >= HOT_FROM and a1 >= HOT_FROM)]
    for lanes, enters in ((every, True), (no_both, False), ([(h, h2) for h in hot for h2 in hot], True)):
        got, entered = _two_pair_wave(lanes)
        assert entered == enters
        for (a0, a1), (s0, s1) in zip(lanes, got):
            assert s0 == _per_pair(a0) and s1 == _per_pair(a1), (hex(a0), hex(a1))
    kinds = {(a0 >= HOT_FROM, a1 >= HOT_FROM) for a0, a1 in every}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
