"""Forward + backward of ``sdeint_adjoint(..., logqp=True)`` at the BASELINE configs[4] shape (workloads/problems.py:
LatentDiagLogqp, euler / euler): the KL instantiations of the perceptron kernels (mlp_adjoint.plan_logqp) vs the stepwise
stochastic adjoint of the same call (``trajectory_kernel: False``, what `bench.py --workload
c5_logqp_adjoint_latent_b32768_d128_s500` measures) vs the same dynamics without the KL column on `_MlpAdjointFn`
(LatentDiag: `mlp_adjoint.route` takes a module whose parameters are the six tensors only). The three run in one process after
warm-up; medians and spread per variant. Run on the GPU box.

    python tools/bench_logqp_adjoint.py [--B 32768] [--d 128] [--steps 500] [--reps 7] [--no-stepwise]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32768)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-stepwise", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    dt = 2.0 ** -9
    ts = torch.tensor([0.0, args.steps * dt], device=dev)
    kl_module = problems.LatentDiagLogqp(args.d).to(dev)
    plain_module = problems.LatentDiag(args.d).to(dev)

    def step(i, sde, logqp, adjoint_options):
        y0 = torch.full((args.B, args.d), 0.1, device=dev, requires_grad=True)
        bm = torchsde_amd.BrownianInterval(0.0, args.steps * dt, size=(args.B, args.d + (1 if logqp else 0)),
                                           dtype=torch.float32, device=dev, entropy=20240601 + i, dt=dt)
        sde.zero_grad()
        out = torchsde_amd.sdeint_adjoint(sde, y0, ts, bm=bm, method="euler", adjoint_method="euler", dt=dt, logqp=logqp,
                                          adjoint_options=adjoint_options)
        if logqp:       # (as bench.py: a term of the path and the KL term)
            ys, log_ratio = out
            loss = ys[-1].sum() + log_ratio.sum()
        else:
            ys, loss = out, out[-1].sum()
        loss.backward()
        return ys, y0.grad

    def timed(label, sde, logqp, adjoint_options, route):
        for i in range(3):          # (the first solve of a form runs both routes and compares)
            ys, _ = step(i, sde, logqp, adjoint_options)
        node, taken = ys.grad_fn, False
        for _ in range(4):
            taken = taken or type(node).__name__.startswith(route)
            node = node.next_functions[0][0] if node is not None and node.next_functions else None
        assert taken, f"{label}: the route {route} was not taken"
        times = []
        for i in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            _, g = step(10 + i, sde, logqp, adjoint_options)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        assert torch.isfinite(g).all()
        med = statistics.median(times)
        print(f"  {label:<58s} median {med:8.2f} ms   min {min(times):8.2f}   max {max(times):8.2f}   ({args.reps} runs)")
        return med

    print(f"B={args.B} d={args.d} hidden={args.d} steps={args.steps}  forward + backward per call")
    kl = timed("logqp=True, KL perceptron kernels", kl_module, True, None, "_MlpLogqpAdjointFn")
    plain = timed("logqp=False, perceptron kernels (no KL column)", plain_module, False, None, "_MlpAdjointFn")
    print(f"  ratio KL / no KL: {kl / plain:.2f}")
    if not args.no_stepwise:
        slow = timed("logqp=True, stepwise stochastic adjoint", kl_module, True,
                     {"trajectory_kernel": False}, "_SdeintAdjointMethod")
        print(f"  ratio stepwise / KL kernels: {slow / kl:.1f}")


if __name__ == "__main__":
    main()
