"""``tsde_aug_update`` (csrc/steps.hip `aug_multi_kernel`): the solver step on every segment of the stochastic adjoint's
augmented state (y, a_y, one a_theta per parameter tensor) against a float64 statement of it (run with ``-m gpu``).

A launch maps 4096-element chunks to at most 24 segments through a table in its arguments; a longer list -- a module with more
than 22 parameter tensors -- takes further launches. So: 1, 24, 25 and 49 segments, lengths on either side of a chunk
and of a group of 4, an empty segment in the middle, every combination of absent terms, outputs that alias the state and
outputs that do not, layouts on either side of the per-segment vector / scalar decision, a segment with more chunks
than the grid has blocks -- and, end to end, the adjoint of a module with 26 parameter tensors against the oracle.

The bound. out = ((s + sF*(F*cF)) + sG*(cG*G)) + sD*D has two roundings per product term and three additions, each
relative to a partial sum that S = |s| + |sF*F*cF| + |sG*cG*G| + |sD*D| bounds: |got - want| <= 8 u S (u the unit roundoff
of the dtype; doubled in float64, where the reference is float64 arithmetic itself). cF and cG are taken as the launch
dtype stores them."""
import itertools
import math

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
KID_AUG_UPDATE = 5
MAX_SEG, CHUNK = 24, 4096            # csrc/steps.hip: kAugMaxSeg, kAugChunk
LENGTHS = (1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 4)
SUBSETS = [tuple(name for name, on in zip("FGD", bits) if on) for bits in itertools.product((0, 1), repeat=3)]
CF, CG = 0.07, -0.3
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
WORST = {}


def _K():
    from torchsde_amd import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the largest error / bound of the run, per dtype."""
    yield
    for label in sorted(WORST):
        print(f"WORST aug_update {label}: error / bound = {WORST[label]:.4f}")
    torch.cuda.empty_cache()      # the large cases' blocks go back to the device, not to the rest of the suite's process


def _plan(count):
    """`count` non-empty segments, lengths and term subsets in rotation (7 lengths against 8 subsets: each meets each
    within 56 segments), and -- from two segments on -- an empty one in the middle. [(n, terms present)]"""
    plan = [(LENGTHS[i % len(LENGTHS)], SUBSETS[(i + 7) % len(SUBSETS)]) for i in range(count)]     # segment 0: F, G and D
    if count > 1:
        plan.insert(count // 2, (0, ("F", "G", "D")))
    return plan


def _values(plan, seed):
    """float64 host values of every operand of every segment; the layouts below are made from these and leave them alone."""
    rng = np.random.default_rng(seed)
    return [{name: rng.standard_normal(n) for name in ("s",) + terms} for n, terms in plan]


def _place(values, dtype, layout, guard):
    """The values on the device: `aligned`, or (`offset`) as a view one element into a larger buffer; `guard`: in a
    NaN-filled buffer with a spare element behind the view (and, with `offset`, the one in front of it)."""
    lead, n = (1 if layout == "offset" else 0), len(values)
    buf = torch.full((lead + n + 1,), float("nan"), dtype=dtype, device=DEV) if guard else \
        torch.empty(lead + n + 1, dtype=dtype, device=DEV)
    view = buf[lead:lead + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(dtype))
    return view, buf, lead


def _run(plan, values, dtype, layout, alias, cut=0):
    """One `kernels.aug_update` over the segments (each shortened by `cut` elements). Returns the outputs and the float64
    operands as stored; has checked the launch count, that no NaN is left and that the guards are intact."""
    K = _K()
    segments, stored, guards = [], [], []
    for i, ((n, terms), vals) in enumerate(zip(plan, values)):
        n = max(n - cut, 0)
        s, sbuf, lead = _place(vals["s"][:n], dtype, layout, guard=True)
        sign = -1.0 if i == 0 else 1.0            # adjoint._update: the y segment carries the reference's sign
        seg = {"s": s, "sF": sign, "sG": sign, "sD": 1.0}
        kept = {"s": s.double().clone()}
        for name in terms:
            seg[name] = _place(vals[name][:n], dtype, layout, guard=False)[0]
            kept[name] = seg[name].double()
        if alias:
            seg["out"], obuf = s, sbuf
        else:
            seg["out"], obuf, _ = _place(np.full(n, np.nan), dtype, layout, guard=True)
        segments.append(seg)
        stored.append(kept)
        guards.append((obuf, lead, n))
    nonempty = sum(1 for seg in segments if seg["s"].numel() > 0)
    K.prof_begin(KID_AUG_UPDATE, 8)
    K.aug_update(segments, CF, CG, dtype, torch.device(DEV))
    torch.cuda.synchronize()
    assert K.prof_end()[1] == math.ceil(nonempty / MAX_SEG), "launches"
    for i, (seg, (obuf, lead, n)) in enumerate(zip(segments, guards)):
        assert not torch.isnan(seg["out"]).any(), f"segment {i} (n = {n}, {layout}): NaN left in the output"
        assert torch.isnan(obuf[:lead]).all() and torch.isnan(obuf[lead + n:]).all(), \
            f"segment {i} (n = {n}, {layout}): wrote outside its output"
    return [seg["out"] for seg in segments], stored


def _check_bound(outs, stored, dtype, what):
    cF, cG = (torch.tensor(c, dtype=dtype).double().item() for c in (CF, CG))
    for i, (got, ops) in enumerate(zip(outs, stored)):
        if got.numel() == 0:
            continue
        sign = -1.0 if i == 0 else 1.0
        zero = torch.zeros_like(ops["s"])
        tF = sign * (ops["F"] * cF) if "F" in ops else zero
        tG = sign * (cG * ops["G"]) if "G" in ops else zero
        tD = ops.get("D", zero)
        want = ((ops["s"] + tF) + tG) + tD
        S = ops["s"].abs() + tF.abs() + tG.abs() + tD.abs()
        bound = 8 * UNIT[dtype] * S * (2.0 if dtype == torch.float64 else 1.0)
        err = (got.double() - want).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        label = "f64" if dtype == torch.float64 else "f32"
        WORST[label] = max(WORST.get(label, 0.0), ratio)
        print(f"RATIO aug_update {label} {what}, segment {i}: error / bound = {ratio:.4f}")
        assert (err <= bound).all(), f"{what}, segment {i} (n = {got.numel()}, terms {sorted(ops)}): error / bound {ratio:.3f}"


@pytest.mark.parametrize("alias", [False, True], ids=["out_distinct", "out_is_s"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("count", [1, 24, 25, 49])
def test_segments_against_float64_in_every_layout(count, dtype, alias):
    """1, 24 (one full table), 25 and 49 (a second and a third launch) segments: within the bound; aligned operands, views
    one element into larger buffers and segments shortened by one element agree bit for bit on the elements they share."""
    plan = _plan(count)
    values = _values(plan, 100 + count)
    aligned, stored = _run(plan, values, dtype, "aligned", alias)
    _check_bound(aligned, stored, dtype, f"{count} segments aligned")
    offset, stored = _run(plan, values, dtype, "offset", alias)
    _check_bound(offset, stored, dtype, f"{count} segments offset")
    shorter, _ = _run(plan, values, dtype, "aligned", alias, cut=1)
    for i, (a, b, c) in enumerate(zip(aligned, offset, shorter)):
        assert torch.equal(a, b), f"segment {i}: offset views differ from the aligned operands"
        assert torch.equal(a[:c.numel()], c), f"segment {i}: the first n - 1 elements differ from the aligned n"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("terms", SUBSETS, ids=["".join(t) or "none" for t in SUBSETS])
def test_single_segment_with_every_subset_of_terms(terms, dtype):
    """F, G, D present or null in every combination, on the vector path and on the scalar path, with the y segment's sign."""
    for n in (3, 4097, 4 * 4096 + 4):
        plan = [(n, terms)]
        values = _values(plan, n + len(terms))
        for alias in (False, True):
            outs, stored = _run(plan, values, dtype, "aligned", alias)
            _check_bound(outs, stored, dtype, f"n = {n} terms {terms}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_more_chunks_than_blocks(dtype):
    """2049 * 4096 + 1 elements (scalar path) and + 4 (vector path): 2050 chunks each, more than the 2048 blocks of the
    grid, so blocks come round a second time -- and, with both in one call, into the next segment."""
    plan = [(2049 * CHUNK + 1, ("F", "G", "D")), (2049 * CHUNK + 4, ("F", "D"))]
    values = _values(plan, 9)
    for alias in (False, True):
        outs, stored = _run(plan, values, dtype, "aligned", alias)
        _check_bound(outs, stored, dtype, "more chunks than blocks")


# ---- end to end: the adjoint of a module with 26 parameter tensors ------------------------------------------------------------
class _Deep(nn.Module):
    """Diagonal noise; 13 linear layers (ten in the drift, three in the diffusion): y, a_y and 26 a_theta are 28 segments."""
    noise_type, sde_type = "diagonal", "ito"

    def __init__(self, d):
        super().__init__()
        torch.manual_seed(3)
        self.drift = nn.ModuleList([nn.Linear(d, d) for _ in range(10)])
        self.diffusion = nn.ModuleList([nn.Linear(d, d) for _ in range(3)])
        self.double()

    def f(self, t, y):
        x = y
        for layer in self.drift:
            x = x + torch.tanh(layer(x))
        return torch.sin(t) - x

    def g(self, t, y):
        x = y
        for layer in self.diffusion:
            x = torch.tanh(layer(x))
        return 0.2 * torch.sigmoid(x)


def test_adjoint_of_a_module_with_26_parameter_tensors_matches_the_oracle():
    """sdeint_adjoint, float64, Euler / Euler, 16 steps of 2^-5, outputs at steps 0, 6 and 16: every update of the backward
    sweep is two launches (24 + 4 segments). Against the oracle's adjoint on the counter path, at the tolerances of
    tests/test_gpu_adjoint.py::test_adjoint_matches_oracle_on_counter_rng_path."""
    import copy

    import torchsde_amd
    from oracle import adjoint_ref, counter
    K = _K()
    B, d, dtype = 5, 3, torch.float64
    steps, dt = 16, 2.0 ** -5
    ts_list = [0.0, 6 * dt, steps * dt]
    edges = np.arange(steps + 1) * dt
    sde = _Deep(d)
    assert len(list(sde.parameters())) == 26
    wt = torch.linspace(-1, 1, 3 * B * d, dtype=dtype).reshape(3, B, d)

    def bm_cpu(ta, tb, return_U=False):
        W, U, _ = counter.query(B * d, 404, edges, float(ta), float(tb), dtype=np.float64, have_h=False)
        return torch.from_numpy(W).reshape(B, d)

    ys_ref, gy_ref, gp_ref = adjoint_ref.adjoint_gradients(sde, torch.full((B, d), 0.1, dtype=dtype),
                                                           torch.tensor(ts_list, dtype=dtype), bm_cpu, dt, "euler", "euler", wt)
    sde_g = copy.deepcopy(sde).to(DEV)
    y0 = torch.full((B, d), 0.1, dtype=dtype, device=DEV, requires_grad=True)
    bm = torchsde_amd.BrownianInterval(0.0, steps * dt, size=(B, d), dtype=dtype, device=DEV, entropy=404, dt=dt)
    ys = torchsde_amd.sdeint_adjoint(sde_g, y0, torch.tensor(ts_list, dtype=dtype, device=DEV), bm=bm, method="euler",
                                     adjoint_method="euler", dt=dt, adjoint_options={"hip_graph": False})
    K.prof_begin(KID_AUG_UPDATE, 16 * steps)
    (ys * wt.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    launches = K.prof_end()[1]
    assert launches >= 2 * steps and launches % 2 == 0, launches      # 28 segments: two launches per update
    torch.testing.assert_close(ys.detach().cpu(), ys_ref, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(y0.grad.cpu(), gy_ref, rtol=1e-8, atol=1e-10)
    for p, ref in zip(sde_g.parameters(), gp_ref):
        torch.testing.assert_close(p.grad.cpu(), ref, rtol=1e-8, atol=1e-9)
