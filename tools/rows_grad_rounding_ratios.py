"""The factor the row-coupled tangent kernel needs under `helpers.assert_within_reference_rounding`, measured on the GPU: for
every case of tests/helpers_rows_grad.py CASES, every cotangent and quantity (ys, the gradient of y0 and of every parameter),
the ratio

    (|kernel - oracle64| - ROWS_GRAD_FLOOR * scale) / |oracle32 - oracle64|

and its maximum (0 where the floor alone covers the difference). The oracle is autograd through the oracle's stepwise solver on
the counter path. `tests/helpers_rows_grad.py ROWS_GRAD_FACTOR` is twice that maximum, rounded up, and at least 4.

    python tools/rows_grad_rounding_ratios.py [output file]   (default: profiles/rows_grad_rounding_ratios.txt)
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from tests import helpers_rows_grad as H
    from torchsde_amd import specialise
    specialise.MODE = "sync"
    lines, worst, count = [], (0.0, ""), 0
    for index, case in enumerate(H.CASES):
        cells = {}
        for label, name, new32, ref32, ref64 in H.measured(index, "cuda"):
            new32, ref32, ref64 = (x.detach().double().cpu() for x in (new32, ref32, ref64))
            scale = max(1.0, float(ref64.abs().max()))
            err_new, err_ref = float((new32 - ref64).abs().max()), float((ref32 - ref64).abs().max())
            over = max(0.0, err_new - H.ROWS_GRAD_FLOOR * scale)
            ratio = over / err_ref if err_ref > 0.0 else (0.0 if over == 0.0 else float("inf"))
            plain = err_new / err_ref if err_ref > 0.0 else float("inf")
            cells.setdefault(label, []).append((name, ratio, plain))
            count += 1
            if ratio > worst[0]:
                worst = (ratio, f"{case.id} {label} {name}: {err_new:.3e} against {err_ref:.3e}")
        for label, row in cells.items():
            lines.append(f"{case.id} {label}: " + " ".join(f"{name} {ratio:.2f}" for name, ratio, _ in row)
                         + " | " + " ".join(f"{plain:.2f}" for _, _, plain in row))
        print(case.id, f"worst so far {worst[0]:.3f}", flush=True)
    factor = max(4, math.ceil(2 * worst[0])) if math.isfinite(worst[0]) else float("inf")
    carried = ("every difference lies within the floor: the comparison is carried by ROWS_GRAD_FLOOR of each quantity's scale, "
               "the factor stays at its minimum (tests/test_rows_grad_host.py: a gradient off by 1e-3, or two scalars' gradients "
               "exchanged, is still rejected)") if worst[0] == 0.0 else worst[1]
    head = [f"# {__doc__.strip().splitlines()[0]}",
            f"# floor {H.ROWS_GRAD_FLOOR:g}; {count} comparisons; worst ratio {worst[0]:.3f}; twice that, rounded up, at least 4: "
            f"{factor}",
            f"# worst: {carried}",
            "# case, cotangent: the ratio of each quantity | for information, each quantity's "
            "|kernel - oracle64| / |oracle32 - oracle64|, no floor taken off"]
    with open(path, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(head[:3]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rows_grad_rounding_ratios.txt"))
