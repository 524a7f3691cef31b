"""The factor the KL perceptron kernels under `sdeint(..., logqp=True)` need under `helpers.assert_within_reference_rounding`,
measured on the GPU: for every case, cotangent and quantity of tests/test_gpu_mlp_logqp_backprop.py (the solves with a stash
budget of five steps and with re-run chunks included, and the sampling solves with interpolated outputs) the ratio

    (|kernels - oracle64| - BACKPROP_FLOOR * scale) / |oracle32 - oracle64|

and its maximum (0 where the floor alone covers the difference). The oracle is autograd through the oracle's stepwise solver
over `LogqpRef`, never the route itself. `tests/helpers_logqp_backprop.py BACKPROP_FACTOR` is twice that maximum, rounded up, and
at least 4.

    python tools/mlp_logqp_backprop_rounding_ratios.py [output file]   (default: profiles/mlp_logqp_backprop_rounding_ratios.txt)
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    import torch

    from tests import helpers_logqp as L
    from tests import helpers_logqp_backprop as P
    from torchsde_amd import kernels
    fn = kernels._MlpLogqpTrajectoryFn
    lines, worst, count = [], (0.0, ""), 0
    names = None

    def note(case, ref, variant, records):
        nonlocal worst, count
        rows = {}
        for what, err_new, err_ref, ratio in records:
            label, name = what.rsplit(" ", 1)
            plain = err_new / err_ref if err_ref > 0.0 else (0.0 if err_new == 0.0 else float("inf"))
            rows.setdefault(label, {})[name] = (ratio, plain)
            count += 1
            if ratio > worst[0]:
                worst = (ratio, f"{case.id} {variant} {what}: {err_new:.3e} against {err_ref:.3e}")
        for label, cells in rows.items():
            ratios = " ".join(f"{cells[name][0]:.2f}" for name in names if name in cells)
            lines.append(f"{case.id} (min |g| {ref['min_g']:.3f}) {variant} {label}: {ratios} | "
                         f"{max(c[1] for c in cells.values()):.2f}")

    for case in P.cases():
        ref = P.oracle(case)
        names = L.quantities(case.module())
        keep = fn.STASH_BYTES, fn.STATE_BYTES
        for variant in ("whole", "chunked", "re-run"):
            if variant != "whole":
                if case.B == 16:
                    continue
                fn.STASH_BYTES = 5 * case.B * (case.d + 2 * case.hidden) * 4
            if variant == "re-run":
                fn.STATE_BYTES = 1
            try:
                got = P.solve(case, "cuda", expect_route=True)
            finally:
                fn.STASH_BYTES, fn.STATE_BYTES = keep
            note(case, ref, variant, P.compare(got, ref)[0])
        ts = [0.0, 2.5 * P.DT, 9 * P.DT, 16 * P.DT]
        ref = P.oracle(case, ts=ts, gradients=False)
        sde = case.module().to("cuda")
        for _ in range(2):
            with torch.no_grad():
                ys, log_ratio, _ = P.call(case, sde, "cuda", y0=case.y0().to("cuda"), ts=ts)
        note(case, ref, "sampling", P.compare({"values": {"ys": ys, "log_ratio": log_ratio}}, ref)[0])
    factor = max(4, math.ceil(2 * worst[0])) if math.isfinite(worst[0]) else float("inf")
    head = [f"# {__doc__.strip().splitlines()[0]}",
            f"# floor {P.BACKPROP_FLOOR:g}; {count} comparisons; worst ratio {worst[0]:.3f}; twice that, rounded up, at least 4: "
            f"{factor}",
            f"# worst: {worst[1]}",
            "# case, solve, cotangent: the ratio of " + ", ".join(names) + " (sampling: ys, log_ratio) | for information, the "
            "line's largest |kernels - oracle64| / |oracle32 - oracle64|, no floor taken off"]
    with open(path, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(head[:3]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mlp_logqp_backprop_rounding_ratios.txt"))
