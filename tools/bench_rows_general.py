"""`sdeint` under no_grad on row-coupled systems with a diffusion matrix: (1) the generated row kernel
(kernels.trajectory_rows_general: one launch, one lane per row) vs (2) the same call with
``options={"trajectory_kernel": False}`` -- the stepwise route: the user's f and g in torch and the general-noise step kernel,
once per step. Shapes: the Heston module of examples/heston_monte_carlo.py (d = 2, m = 2, Euler) at 65536 and at 1024 rows, and a
4-channel Langevin system whose noise enters the momentum rows only (d = 4, m = 2, additive, Stratonovich, Heun) at 65536 rows;
1000 steps each. All run in one process after warm-up, in interleaved rounds; medians and ranges of the wall time of a call,
and for (1) of the trajectory launch alone (the library's event brackets); each variant asserts its route. Run on the GPU box.

    python tools/bench_rows_general.py [--steps 1000] [--reps 7] [--out profiles/rows_general_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch import nn  # noqa: E402

import torchsde_amd  # noqa: E402
from examples.heston_monte_carlo import Heston  # noqa: E402
from torchsde_amd import _native, kernels as K, specialise  # noqa: E402


class Langevin(nn.Module):
    """Two coupled underdamped oscillators (q1, q2, p1, p2); the noise enters the momentum rows only."""
    noise_type, sde_type = "additive", "stratonovich"

    def __init__(self):
        super().__init__()
        self.gamma = nn.Parameter(torch.tensor(0.7))
        self.k = nn.Parameter(torch.tensor([1.3, 0.8]))
        self.sigma = nn.Parameter(torch.tensor([[0.3, 0.1], [-0.2, 0.25]]))

    def f(self, t, y):
        q, p = y[:, :2], y[:, 2:]
        return torch.cat([p, -self.k * q - self.gamma * p - 0.1 * q ** 3], dim=1)

    def g(self, t, y):
        B = y.shape[0]
        return torch.cat([torch.zeros(B, 2, 2, dtype=y.dtype, device=y.device), self.sigma.expand(B, 2, 2)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 7
    specialise.MODE = "sync"
    dev = torch.device("cuda")
    dt = 2.0 ** -10
    t1 = args.steps * dt
    ts = torch.tensor([0.0, t1], device=dev)
    shapes = [("Heston d=2 m=2 Euler, B=65536", Heston().to(dev), (1.0, 0.09), 2, 65536, "euler"),
              ("Heston d=2 m=2 Euler, B=1024", Heston().to(dev), (1.0, 0.09), 2, 1024, "euler"),
              ("Langevin d=4 m=2 Heun, B=65536", Langevin().to(dev), (0.4, -0.3, 0.1, 0.2), 2, 65536, "heun")]

    def solve(shape, i, options):
        _, sde, start, m, B, method = shape
        y0 = torch.tensor(start, device=dev).expand(B, len(start)).contiguous()
        bm = torchsde_amd.BrownianInterval(0.0, t1, size=(B, m), dtype=torch.float32, device=dev, entropy=20240601 + i)
        with torch.no_grad():
            return torchsde_amd.sdeint(sde, y0, ts, bm=bm, method=method, dt=dt, options=options)

    def launches(fn):
        K.prof_begin(_native.KID_TRAJECTORY, 64)
        fn()
        torch.cuda.synchronize()
        return K.prof_end()

    kernel, stepwise = {"hip_graph": False}, {"trajectory_kernel": False}
    variants = []
    for shape in shapes:
        variants += [(f"(1) {shape[0]}, generated row kernel", shape, kernel, 1),
                     (f"(2) {shape[0]}, trajectory_kernel: False", shape, stepwise, 0)]
    for label, shape, options, expected in variants:
        for i in range(3):          # (the first solve of a form runs both routes and compares)
            solve(shape, i, options)
        assert launches(lambda: solve(shape, 3, options))[1] == expected, f"{label}: expected {expected} trajectory launches"
    times = {label: [] for label, *_ in variants}
    launch = {label: [] for label, _, options, _ in variants if options is kernel}
    for i in range(args.reps):      # interleaved rounds
        for label, shape, options, expected in variants:
            torch.cuda.synchronize()
            K.prof_begin(_native.KID_TRAJECTORY, 64)
            t = time.perf_counter()
            solve(shape, 10 + i, options)
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t) * 1e3)
            ms, n = K.prof_end()
            assert n == expected, f"{label}: {n} trajectory launches"
            if label in launch:
                launch[label].append(ms)
    lines = [f"row-coupled systems with a diffusion matrix, steps={args.steps} dt=2^-10, float32, sdeint under no_grad per call, "
             f"{args.reps} interleaved rounds after 4 warm-up solves each, one process, {torch.cuda.get_device_name(0)}"]
    for label, *_ in variants:
        t = times[label]
        lines.append(f"  {label:<62s} median {statistics.median(t):9.2f} ms   min {min(t):9.2f}   max {max(t):9.2f}"
                     + (f"   its launch alone: median {statistics.median(launch[label]):7.3f} ms   min {min(launch[label]):7.3f}"
                        f"   max {max(launch[label]):7.3f}" if label in launch else ""))
    for k in range(0, len(variants), 2):
        one, two = times[variants[k][0]], times[variants[k + 1][0]]
        lines.append(f"  {variants[k][1][0]}: (2) / (1) = {statistics.median(two) / statistics.median(one):.1f}; (1)'s slowest run "
                     f"{max(one):.2f} ms against (2)'s fastest {min(two):.2f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
