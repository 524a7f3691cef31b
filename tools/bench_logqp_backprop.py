"""Forward + backward of ``sdeint(..., logqp=True)`` at the BASELINE configs[4] shape (workloads/problems.py: LatentDiagLogqp,
Euler): (a) the KL instantiations of the perceptron kernels (mlp_adjoint.plan_logqp_sdeint, kernels._MlpLogqpTrajectoryFn) vs
(b) the same call with ``options={"trajectory_kernel": False}`` -- back-propagation through the stepwise solver, the path this
call took before the route existed -- vs (c) the same dynamics without the KL column on `_MlpTrajectoryFn`
(torchsde_amd.MLPDriftDiagonalSDE holding LatentDiagLogqp's weights). The three run in one process after warm-up, in interleaved
rounds; medians and spread per variant; each variant asserts that its route was taken. Expectation for (a) / (c): the KL sweep
runs four matrix products per step against three, the KL sampling kernel draws two Philox quads per four increments against one.
Run on the GPU box.

    python tools/bench_logqp_backprop.py [--B 32768] [--d 128] [--steps 500] [--reps 7] [--out profiles/logqp_backprop_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torchsde_amd  # noqa: E402
from workloads import problems  # noqa: E402


def graph_has(tensor, name, depth=6):
    seen, frontier = set(), [tensor.grad_fn]
    for _ in range(depth):
        nxt = []
        for fn in frontier:
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            if type(fn).__name__.startswith(name):
                return True
            nxt.extend(f for f, _ in fn.next_functions)
        frontier = nxt
    return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32768)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    dt = 2.0 ** -9
    ts = torch.tensor([0.0, args.steps * dt], device=dev)
    kl_module = problems.LatentDiagLogqp(args.d).to(dev)
    plain_module = torchsde_amd.MLPDriftDiagonalSDE(args.d, args.d, activation="softplus", diffusion="sigmoid", diff_scale=0.1,
                                                    diff_rate=torch.zeros(args.d), diff_shift=torch.zeros(args.d)).to(dev)
    with torch.no_grad():
        for mine, theirs in zip(plain_module.closed_form_parameters(),
                                (kl_module.net[0].weight, kl_module.net[0].bias, kl_module.net[2].weight,
                                 kl_module.net[2].bias, kl_module.w, kl_module.b)):
            mine.copy_(theirs)

    def step(i, sde, logqp, options):
        y0 = torch.full((args.B, args.d), 0.1, device=dev, requires_grad=True)
        bm = torchsde_amd.BrownianInterval(0.0, args.steps * dt, size=(args.B, args.d + (1 if logqp else 0)),
                                           dtype=torch.float32, device=dev, entropy=20240601 + i, dt=dt)
        sde.zero_grad()
        out = torchsde_amd.sdeint(sde, y0, ts, bm=bm, method="euler", dt=dt, logqp=logqp, options=options)
        if logqp:       # (as bench.py: a term of the path and the KL term)
            ys, log_ratio = out
            loss = ys[-1].sum() + log_ratio.sum()
        else:
            ys, loss = out, out[-1].sum()
        loss.backward()
        return ys, y0.grad

    variants = (
        ("(a) logqp=True, KL perceptron kernels", kl_module, True, None, "_MlpLogqpTrajectoryFn", True),
        ("(b) logqp=True, trajectory_kernel: False (stepwise)", kl_module, True, {"trajectory_kernel": False},
         "_MlpLogqpTrajectoryFn", False),
        ("(c) logqp=False, perceptron kernels (no KL column)", plain_module, False, None, "_MlpTrajectoryFn", True),
    )
    for label, sde, logqp, options, route, expected in variants:
        for i in range(3):          # (the first solve of a form runs both routes and compares)
            ys, _ = step(i, sde, logqp, options)
        assert graph_has(ys, route) == expected, f"{label}: route {route} taken: {not expected}"
    times = {label: [] for label, *_ in variants}
    for i in range(args.reps):      # interleaved rounds
        for label, sde, logqp, options, route, expected in variants:
            torch.cuda.synchronize()
            t = time.perf_counter()
            ys, g = step(10 + i, sde, logqp, options)
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t) * 1e3)
            assert torch.isfinite(g).all() and graph_has(ys, route) == expected
    lines = [f"B={args.B} d={args.d} hidden={args.d} steps={args.steps}  sdeint forward + backward per call, Euler, "
             f"{args.reps} interleaved rounds after 3 warm-up solves each, one process, {torch.cuda.get_device_name(0)}"]
    med = {}
    for label, *_ in variants:
        t = times[label]
        med[label[:3]] = statistics.median(t)
        lines.append(f"  {label:<58s} median {statistics.median(t):8.2f} ms   min {min(t):8.2f}   max {max(t):8.2f}")
    a, b, c = (times[label] for label, *_ in variants)
    lines.append(f"  (b) / (a): {med['(b)'] / med['(a)']:.1f}    (a)'s slowest run {max(a):.2f} ms against (b)'s fastest "
                 f"{min(b):.2f} ms: (a)'s whole spread lies {'below' if max(a) < min(b) else 'NOT below'} (b)'s")
    lines.append(f"  (a) / (c): {med['(a)'] / med['(c)']:.2f}    expected from the sweep alone: 4 matrix products per step "
                 "against 3 = 1.33, plus the second Philox quad per four increments both ways")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert max(a) < min(b), "the KL kernels are not faster than the stepwise route"


if __name__ == "__main__":
    main()
