"""The factor the perceptron training kernels need under `helpers.assert_within_reference_rounding` on output grids that
interpolate, measured on the GPU: for every case of tests/test_gpu_interp_backprop.py (both routes, every grid, shape, scheme),
every cotangent and quantity -- and, on `chunk_edges`, the solves with a stash budget of five steps and with re-run chunks -- the
ratio

    (|kernels - oracle64| - INTERP_FLOOR * scale) / |oracle32 - oracle64|

and its maximum (0 where the floor alone covers the difference). The oracle is autograd through the oracle's stepwise solver,
never the route itself. `tests/helpers_interp_backprop.py INTERP_FACTOR` is twice that maximum, rounded up, and at least 4.

    python tools/interp_backprop_rounding_ratios.py [output file]   (default: profiles/interp_backprop_rounding_ratios.txt)
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from tests import helpers_interp_backprop as I
    from torchsde_amd import kernels
    lines, worst, count = [], (0.0, ""), 0

    def note(case, variant, records):
        nonlocal worst, count
        rows = {}
        for what, err_new, err_ref, ratio in records:
            label, name = what.rsplit(" ", 1)
            plain = err_new / err_ref if err_ref > 0.0 else (0.0 if err_new == 0.0 else float("inf"))
            rows.setdefault(label, []).append((name, ratio, plain))
            count += 1
            if ratio > worst[0]:
                worst = (ratio, f"{case.id} {variant} {what}: {err_new:.3e} against {err_ref:.3e}")
        for label, cells in rows.items():
            lines.append(f"{case.id} {variant} {label}: " + " ".join(f"{name} {ratio:.2f}" for name, ratio, _ in cells)
                         + f" | {max(c[2] for c in cells):.2f}")

    for case in I.plain_cases() + I.kl_cases():
        ref = I.oracle(case)
        fn = kernels._MlpTrajectoryFn if case.route == "plain" else kernels._MlpLogqpTrajectoryFn
        keep = fn.STASH_BYTES, fn.STATE_BYTES
        for variant in ("whole", "chunked", "re-run"):
            if variant != "whole":
                if case.grid != "chunk_edges" or case.B == 16:
                    continue
                fn.STASH_BYTES = 5 * case.B * (case.d + 2 * case.hidden) * 4
            if variant == "re-run":
                fn.STATE_BYTES = 1
            try:
                got = I.solve(case, "cuda")
            finally:
                fn.STASH_BYTES, fn.STATE_BYTES = keep
            note(case, variant, I.compare(got, ref)[0])
        print(case.id, f"worst so far {worst[0]:.3f}", flush=True)
    factor = max(4, math.ceil(2 * worst[0])) if math.isfinite(worst[0]) else float("inf")
    head = [f"# {__doc__.strip().splitlines()[0]}",
            f"# floor {I.INTERP_FLOOR:g}; {count} comparisons; worst ratio {worst[0]:.3f}; twice that, rounded up, at least 4: "
            f"{factor}",
            f"# worst: {worst[1]}",
            "# case, solve, cotangent: the ratio of each quantity | for information, the line's largest "
            "|kernels - oracle64| / |oracle32 - oracle64|, no floor taken off"]
    with open(path, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(head[:3]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "interp_backprop_rounding_ratios.txt"))
