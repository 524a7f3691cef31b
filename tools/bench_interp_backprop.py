"""Forward + backward of ``sdeint`` on the perceptron kernels when the output times do not sit on step boundaries, at the
BASELINE configs[4] shape (workloads/problems.py: LatentDiagLogqp, Euler), with and without ``logqp=True``:
(1) ``ts = linspace(0, steps * dt, 100)`` on the kernels (kernels._MlpLogqpTrajectoryFn / _MlpTrajectoryFn: one sampling launch
that writes every boundary and the 99 outputs, the weighted reverse sweep) vs (2) the same call with
``options={"trajectory_kernel": False}`` -- back-propagation through the stepwise solver, the path this call took before the sweep
took interpolation weights -- vs (3) ``ts = [0, steps * dt]`` on the kernels. All run in one process after warm-up, in
interleaved rounds; medians and spread per variant; each variant asserts its route. (1) / (3) is reported, not bounded: above the
step work (1) writes 99 output rows, copies the boundary states out from between them and reads 99 cotangent rows.
Run on the GPU box.

    python tools/bench_interp_backprop.py [--B 32768] [--d 128] [--steps 500] [--reps 7] [--out profiles/interp_backprop_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torchsde_amd  # noqa: E402
from tools.bench_logqp_backprop import graph_has  # noqa: E402
from workloads import problems  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32768)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--outputs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 7
    dev = torch.device("cuda")
    dt = 2.0 ** -9
    t1 = args.steps * dt
    grids = {"linspace": torch.linspace(0.0, t1, args.outputs, device=dev), "ends": torch.tensor([0.0, t1], device=dev)}
    kl_module = problems.LatentDiagLogqp(args.d).to(dev)
    plain_module = torchsde_amd.MLPDriftDiagonalSDE(args.d, args.d, activation="softplus", diffusion="sigmoid", diff_scale=0.1,
                                                    diff_rate=torch.zeros(args.d), diff_shift=torch.zeros(args.d)).to(dev)
    with torch.no_grad():
        for mine, theirs in zip(plain_module.closed_form_parameters(),
                                (kl_module.net[0].weight, kl_module.net[0].bias, kl_module.net[2].weight,
                                 kl_module.net[2].bias, kl_module.w, kl_module.b)):
            mine.copy_(theirs)

    def step(i, sde, logqp, grid, options):
        y0 = torch.full((args.B, args.d), 0.1, device=dev, requires_grad=True)
        bm = torchsde_amd.BrownianInterval(0.0, t1, size=(args.B, args.d + (1 if logqp else 0)), dtype=torch.float32,
                                           device=dev, entropy=20240601 + i, dt=dt)
        sde.zero_grad()
        out = torchsde_amd.sdeint(sde, y0, grids[grid], bm=bm, method="euler", dt=dt, logqp=logqp, options=options)
        if logqp:       # (a term of the path at every output and the KL term)
            ys, log_ratio = out
            loss = ys.sum() + log_ratio.sum()
        else:
            ys, loss = out, out.sum()
        loss.backward()
        return ys, y0.grad

    stepwise = {"trajectory_kernel": False}
    variants = []
    for tag, sde, logqp, route in (("logqp=True", kl_module, True, "_MlpLogqpTrajectoryFn"),
                                   ("logqp=False", plain_module, False, "_MlpTrajectoryFn")):
        variants += [(f"(1) {tag}, linspace({args.outputs}), kernels", sde, logqp, "linspace", None, route, True),
                     (f"(2) {tag}, linspace({args.outputs}), trajectory_kernel: False", sde, logqp, "linspace", stepwise, route,
                      False),
                     (f"(3) {tag}, ts = [0, T], kernels", sde, logqp, "ends", None, route, True)]
    for label, sde, logqp, grid, options, route, expected in variants:
        for i in range(3):          # (the first solve of a form and kind of grid runs both routes and compares)
            ys, _ = step(i, sde, logqp, grid, options)
        assert graph_has(ys, route) == expected, f"{label}: route {route} taken: {not expected}"
    times = {label: [] for label, *_ in variants}
    for i in range(args.reps):      # interleaved rounds
        for label, sde, logqp, grid, options, route, expected in variants:
            torch.cuda.synchronize()
            t = time.perf_counter()
            ys, g = step(10 + i, sde, logqp, grid, options)
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t) * 1e3)
            assert torch.isfinite(g).all() and graph_has(ys, route) == expected
    lines = [f"B={args.B} d={args.d} hidden={args.d} steps={args.steps} dt=2^-9  sdeint forward + backward per call, Euler, "
             f"{args.reps} interleaved rounds after 3 warm-up solves each, one process, {torch.cuda.get_device_name(0)}"]
    for label, *_ in variants:
        t = times[label]
        lines.append(f"  {label:<62s} median {statistics.median(t):8.2f} ms   min {min(t):8.2f}   max {max(t):8.2f}")
    below = True
    for k in (0, 3):
        one, two, three = (times[variants[k + j][0]] for j in range(3))
        ok = max(one) < min(two)
        below = below and ok
        lines.append(f"  {variants[k][0].split(',')[0][4:]}: (2) / (1) = {statistics.median(two) / statistics.median(one):.1f}; "
                     f"(1)'s slowest run {max(one):.2f} ms against (2)'s fastest {min(two):.2f} ms: (1)'s whole spread lies "
                     f"{'below' if ok else 'NOT below'} (2)'s; (1) / (3) = {statistics.median(one) / statistics.median(three):.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert below, "the kernels are not faster than the stepwise route on a grid that interpolates"


if __name__ == "__main__":
    main()
