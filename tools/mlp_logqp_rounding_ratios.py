"""The factor the KL perceptron kernels (`sdeint_adjoint(..., logqp=True)`) need under `helpers.assert_within_reference_rounding`,
measured on the GPU: for every case, cotangent and quantity of tests/test_gpu_mlp_logqp_adjoint.py (the solves with a stash
budget of five steps included) the ratio

    (|kernels - oracle64| - LOGQP_FLOOR * scale) / |oracle32 - oracle64|

and its maximum (0 where the floor alone covers the difference). `tests/helpers_logqp.py LOGQP_FACTOR` is twice that maximum,
rounded up, and at least 4.

    python tools/mlp_logqp_rounding_ratios.py [output file]     (default: profiles/mlp_logqp_adjoint_rounding_ratios.txt)
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from tests import helpers_logqp as L
    from torchsde_amd import mlp_adjoint
    lines, worst, count = [], (0.0, ""), 0
    names = None
    for index, case in enumerate(L.cases()):
        ref = L.oracle(case)
        names = L.quantities(case.module())
        keep = mlp_adjoint._MlpAdjointFn.STASH_BYTES
        for variant in ("whole", "chunked"):
            if variant == "chunked":
                if case.B == 16:
                    continue
                mlp_adjoint._MlpAdjointFn.STASH_BYTES = 5 * case.B * (2 * case.d + 2 * case.hidden) * 4
            try:
                got = L.solve(case, "cuda", expect_route=True)
            finally:
                mlp_adjoint._MlpAdjointFn.STASH_BYTES = keep
            records, _ = L.compare(got, ref)
            rows = {}
            for what, err_new, err_ref, ratio in records:
                label, name = what.rsplit(" ", 1)
                plain = err_new / err_ref if err_ref > 0.0 else (0.0 if err_new == 0.0 else float("inf"))
                rows.setdefault(label, {})[name] = (ratio, plain)
                count += 1
                if ratio > worst[0]:
                    worst = (ratio, f"{case.id} {variant} {what}: {err_new:.3e} against {err_ref:.3e}")
            for label, cells in rows.items():
                ratios = " ".join(f"{cells[name][0]:.2f}" for name in names)
                lines.append(f"{case.id} (min |g| {ref['min_g']:.3f}) {variant} {label}: {ratios} | "
                             f"{max(c[1] for c in cells.values()):.2f}")
    factor = max(4, math.ceil(2 * worst[0])) if math.isfinite(worst[0]) else float("inf")
    head = [f"# {__doc__.strip().splitlines()[0]}",
            f"# floor {L.LOGQP_FLOOR:g}; {count} comparisons; worst ratio {worst[0]:.3f}; twice that, rounded up, at least 4: "
            f"{factor}",
            f"# worst: {worst[1]}",
            "# case, solve, cotangent: the ratio of " + ", ".join(names) + " | for information, the line's largest "
            "|kernels - oracle64| / |oracle32 - oracle64|, no floor taken off"]
    with open(path, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(head[:3]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mlp_logqp_adjoint_rounding_ratios.txt"))
