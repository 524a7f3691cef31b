"""The float32 two-pair Box-Muller (torchsde_amd/csrc/tsde_rng.h: `box_muller2`) writes the small-radius series under narrowed
execution masks and puts the mask at entry back afterwards. The mask at entry is not always full: the last wave of a launch is
ragged. tests/test_gpu_box_muller_shared.py samples whole waves only; these run the draw in a ragged wave whose few active lanes
hold a both-hot quad, a first-only quad and a second-only quad (shown from the oracle before anything is compared), and compare
it bytewise with the per-pair form, which the same kernels take for operands offset by one element.

The (entropy, cell) pairs were found by a search over cells 0, 1, 2, ... at entropy 7 with `oracle.counter.normals`; a wave of 3
active lanes that holds all three classes exists (the first is cell 2151), so no larger lane count had to stand in for it.

The solves: the affine Euler kernel at B = 69, d = 4 is below `kTrajVecMinGroups` (csrc/trajectory.hip) and takes one element
per lane on both routes, so a second shape, B = kTrajVecMinGroups + 5, is the one whose 16-byte-group form ends in a 5-lane
wave; each is compared with the same solve from a state offset by one element, which the launcher sends to the
one-element-per-lane form."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENTROPY = 7
HOT_R2 = -2.0 * math.log(15.0 / 16.0)      # a pair is hot when its squared radius -2 ln u1 is below this: u1 > 15/16
WAVE = 64
TRAJ_VEC_MIN_GROUPS = 256 * 8 * 64         # csrc/trajectory.hip kTrajVecMinGroups

# (elements, cell, classes of the quads of the ragged wave in lane order)
RAGGED = [
    (4 * (WAVE + 5), 2094, ["second only", "none", "both", "first only", "none"]),   # a full wave, then a wave of 5 lanes
    (4 * 3, 2151, ["both", "second only", "first only"]),                            # a wave of 3 lanes alone
]


def _classes(n, cell, stream=0):
    from oracle import counter
    z = counter.normals(n, ENTROPY, elem0=0, cell=cell, node=0, stream=stream).reshape(-1, 4)
    h0 = z[:, 0] ** 2 + z[:, 1] ** 2 < HOT_R2
    h1 = z[:, 2] ** 2 + z[:, 3] ** 2 < HOT_R2
    names = {(True, True): "both", (True, False): "first only", (False, True): "second only", (False, False): "none"}
    return [names[(bool(a), bool(b))] for a, b in zip(h0, h1)]


def _increments(n, cell, offset):
    """(W, U) of `cell` with h = 1 from the increment kernel, the outputs 16-byte aligned (offset 0: `normal4`) or one element
    past an aligned address (offset 1: `normal1`)."""
    from torchsde_amd import _native
    from torchsde_amd import kernels as K
    outs = []
    for _ in range(2):
        base = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
        assert base.data_ptr() % 16 == 0
        outs.append(base[offset:offset + n])
    spec = K.NoiseSpec((n,), torch.float32, torch.device(DEV), entropy=ENTROPY, elem0=0, cell=cell, h=1.0)
    code = _native.load().tsde_cell_increment(outs[0].data_ptr(), outs[1].data_ptr(), n, spec.struct(), _native.F32,
                                              _native.stream_ptr(torch.device(DEV)))
    _native.check(code, "tsde_cell_increment")
    torch.cuda.synchronize()
    return outs


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.mark.parametrize("n,cell,classes", RAGGED, ids=["wave_plus_5_lanes", "3_lanes"])
def test_ragged_wave_draws_the_normals_of_the_per_pair_form(n, cell, classes):
    from oracle import counter
    ragged = _classes(n, cell)[(n // 4) // WAVE * WAVE:]
    print(f"n = {n}, cell {cell}: ragged wave {ragged}")
    assert ragged == classes
    assert {"both", "first only", "second only"} <= set(ragged)
    Wv, Uv = _increments(n, cell, 0)
    Ws, Us = _increments(n, cell, 1)
    assert torch.isfinite(Wv).all() and torch.isfinite(Uv).all()        # every element written: no lane left masked off
    assert _bytes(Wv) == _bytes(Ws)
    assert _bytes(Uv) == _bytes(Us)
    ref = counter.normals(n, ENTROPY, elem0=0, cell=cell, node=0, stream=0)
    assert np.abs(Wv.cpu().numpy().astype(np.float64) - ref).max() <= 2e-5


@pytest.mark.parametrize("B", [69, TRAJ_VEC_MIN_GROUPS + 5], ids=["b69", "min_groups_plus_5"])
def test_affine_euler_solve_with_a_ragged_wave_is_bytewise_the_one_element_per_lane_solve(B):
    import torchsde_amd
    from torchsde_amd import kernels as K
    d, steps, dt = 4, 64, 2.0 ** -6
    gen = torch.Generator().manual_seed(7)
    rate = torch.rand(d, generator=gen, dtype=torch.float64) * 0.6 - 0.3
    vol = torch.rand(d, generator=gen, dtype=torch.float64) * 0.5 + 0.1
    sde = torchsde_amd.AffineDiagonalSDE(rate, torch.zeros(d, dtype=torch.float64), vol, 0.0, sde_type="ito",
                                         dtype=torch.float32, device=DEV)
    ts = torch.tensor([0.0, steps * dt], dtype=torch.float32, device=DEV)
    base = torch.linspace(0.5, 1.5, B * d + 4, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    values = base[:B * d].clone()
    true_launch = K.trajectory_affine_diag
    solves, seen = [], []

    def recording(ys, y0_, *args, **kwargs):
        seen.append(y0_.data_ptr() % 16)
        return true_launch(ys, y0_, *args, **kwargs)

    K.trajectory_affine_diag = recording
    try:
        for offset in (0, 1):
            holder = torch.empty(B * d + 4, dtype=torch.float32, device=DEV)
            y0 = holder[offset:offset + B * d]
            y0.copy_(values)
            y0 = y0.view(B, d)
            bm = torchsde_amd.BrownianInterval(0.0, steps * dt, size=(B, d), dtype=torch.float32, device=DEV, entropy=23)
            with torch.no_grad():
                solves.append(torchsde_amd.sdeint(sde, y0, ts, bm=bm, method="euler", dt=dt,
                                                  options={"trajectory_kernel": True}))
    finally:
        K.trajectory_affine_diag = true_launch
    torch.cuda.synchronize()
    assert seen == [0, 4]              # the second state reached the launcher off the 16-byte grid: one element per lane
    vec, scalar = solves
    assert vec.shape == (2, B, d) and torch.isfinite(vec).all()
    assert (vec[1] != vec[0]).all(dim=1).all()        # every row moved: no lane stopped stepping after the masked writes
    assert _bytes(vec) == _bytes(scalar)
