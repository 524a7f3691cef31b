"""Forward + backward of ``sdeint`` on a row-coupled system: the stochastic Lorenz module with its six constants as parameters
(examples/fit_lorenz_parameters.py), Euler, on two output grids -- the two ends, and 100 `linspace` outputs:
(1) the generated tangent unit (kernels._RowsTrajectoryFn: one launch that carries d/dy0 and one tangent per parameter in
registers and writes the sensitivities of every output; the backward pass a few reductions) vs (2) the same call with
``options={"trajectory_kernel": False}`` -- back-propagation through the stepwise solver -- and, as the floor, (3) the `no_grad`
rows solve of the same shape (forward only). All run in one process after warm-up, in interleaved rounds; medians and ranges of
the wall time of a call, and for (1) and (3) of the trajectory launch alone (the library's event brackets: a call of either is
mostly host work at this size); each variant asserts its route. Run on the GPU box.

    python tools/bench_rows_grad.py [--B 65536] [--steps 1000] [--reps 7] [--out profiles/rows_grad_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torchsde_amd  # noqa: E402
from examples.fit_lorenz_parameters import Lorenz  # noqa: E402
from torchsde_amd import _native, kernels as K, specialise  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--outputs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 7
    specialise.MODE = "sync"
    dev = torch.device("cuda")
    dt = 2.0 ** -10
    t1 = args.steps * dt
    grids = {"ends": torch.tensor([0.0, t1], device=dev), "linspace": torch.linspace(0.0, t1, args.outputs, device=dev)}
    sde = Lorenz().to(dev)
    start = torch.randn(args.B, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def step(i, grid, options, grad):
        y0 = start.clone().requires_grad_(grad)
        bm = torchsde_amd.BrownianInterval(0.0, t1, size=(args.B, 3), dtype=torch.float32, device=dev, entropy=20240601 + i)
        sde.zero_grad()
        with (torch.enable_grad() if grad else torch.no_grad()):
            ys = torchsde_amd.sdeint(sde, y0, grids[grid], bm=bm, method="euler", dt=dt, options=options)
        if grad:
            ys.square().mean().backward()
            assert torch.isfinite(y0.grad).all() and all(torch.isfinite(p.grad).all() for p in sde.parameters())
        return ys

    def routed(ys):
        return type(ys.grad_fn).__name__ == "_RowsTrajectoryFnBackward"

    stepwise, eager = {"trajectory_kernel": False}, {"hip_graph": False}
    variants = []
    for grid in grids:
        variants += [(f"(1) {grid}, tangent unit", grid, eager, True, True),
                     (f"(2) {grid}, trajectory_kernel: False", grid, stepwise, True, False),
                     (f"(3) {grid}, no_grad rows solve (forward only)", grid, eager, False, False)]
    for label, grid, options, grad, expected in variants:
        for i in range(3):          # (the first solve of a form runs both routes and compares)
            ys = step(i, grid, options, grad)
        assert routed(ys) == expected, f"{label}: tangent unit taken: {not expected}"
    times = {label: [] for label, *_ in variants}
    launch = {label: [] for label, _, options, *_ in variants if options is eager}
    for i in range(args.reps):      # interleaved rounds
        for label, grid, options, grad, expected in variants:
            torch.cuda.synchronize()
            if label in launch:
                K.prof_begin(_native.KID_TRAJECTORY, 64)
            t = time.perf_counter()
            ys = step(10 + i, grid, options, grad)
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t) * 1e3)
            if label in launch:
                ms, n = K.prof_end()
                assert n == 1, f"{label}: {n} trajectory launches"
                launch[label].append(ms)
            assert routed(ys) == expected
    lines = [f"Lorenz, six trainable parameters and y0 (NT = 9), B={args.B} d=3 steps={args.steps} dt=2^-10, float32, Euler, "
             f"sdeint forward + backward per call, {args.reps} interleaved rounds after 3 warm-up solves each, one process, "
             f"{torch.cuda.get_device_name(0)}"]
    for label, *_ in variants:
        t = times[label]
        lines.append(f"  {label:<52s} median {statistics.median(t):9.2f} ms   min {min(t):9.2f}   max {max(t):9.2f}"
                     + (f"   its launch alone: median {statistics.median(launch[label]):7.3f} ms   min {min(launch[label]):7.3f}"
                        f"   max {max(launch[label]):7.3f}" if label in launch else ""))
    for k in (0, 3):
        one, two, three = (times[variants[k + j][0]] for j in range(3))
        lines.append(f"  {variants[k][1]}: (2) / (1) = {statistics.median(two) / statistics.median(one):.1f}; (1)'s slowest run "
                     f"{max(one):.2f} ms against (2)'s fastest {min(two):.2f} ms; launch of (1) / launch of (3) = "
                     f"{statistics.median(launch[variants[k][0]]) / statistics.median(launch[variants[k + 2][0]]):.1f} "
                     "(arithmetic alone: 1 + NT = 10)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
