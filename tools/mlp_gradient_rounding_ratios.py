"""The factor the perceptron training kernels need under `helpers.assert_within_reference_rounding`, measured on the GPU:
for every case, cotangent and quantity of tests/test_gpu_mlp_gradient_rounding.py (whole tensors and ragged tiles; the solves
with a stash budget of five steps and with recomputed states included) the ratio

    (|kernels - oracle64| - MLP_GRAD_FLOOR * scale) / |oracle32 - oracle64|

and its maximum (0 where the floor alone covers the difference). `tests/helpers.py MLP_GRAD_FACTOR` is twice that maximum,
rounded up, within [4, 8].

    python tools/mlp_gradient_rounding_ratios.py [output file]     (default: profiles/mlp_gradient_rounding_ratios.txt)
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Patch:
    """The part of pytest's monkeypatch that `_budgets` uses."""

    def __init__(self):
        self.undo = []

    def setattr(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def restore(self):
        for obj, name, value in reversed(self.undo):
            setattr(obj, name, value)


def main(path):
    from tests import helpers
    from tests import test_gpu_mlp_gradient_rounding as T
    lines, worst, count = [], (0.0, ""), 0
    for index, case in enumerate(T.ALL_CASES):
        variants = [("whole", None)]
        if index in T.SMALL:
            variants += [("chunked", False)] + ([("recomputed", True)] if case.route == "backprop" else [])
        for variant, recompute in variants:
            patch = _Patch()
            try:
                if recompute is not None:
                    T._budgets(patch, case, recompute=recompute)
                got = T.solve(case)
            finally:
                patch.restore()
            records, _ = T.compare(case, got, T._oracle(index))
            rows = {}                                 # cotangent -> quantity -> [ratio, quotient], the larger of whole and tiles
            for what, err_new, err_ref, ratio in records:
                label, name = what.split()[:2]
                plain = err_new / err_ref if err_ref > 0.0 else (0.0 if err_new == 0.0 else float("inf"))
                cell = rows.setdefault(label, {}).setdefault(name, [0.0, 0.0])
                cell[0], cell[1] = max(cell[0], ratio), max(cell[1], plain)
                count += 1
                if ratio > worst[0]:
                    worst = (ratio, f"{case.id} {variant} {' '.join(what.split())}: {err_new:.3e} against {err_ref:.3e}")
            for label, cells in rows.items():
                ratios = " ".join(f"{cells[name][0]:.2f}" for name in helpers.MLP_GRAD_QUANTITIES)
                lines.append(f"{case.id} {variant} {label}: {ratios} | {max(c[1] for c in cells.values()):.2f}")
    factor = min(8, max(4, math.ceil(2 * worst[0]))) if math.isfinite(worst[0]) else float("inf")
    head = [f"# {__doc__.strip().splitlines()[0]}",
            f"# floor {helpers.MLP_GRAD_FLOOR:g}; {count} comparisons; worst ratio {worst[0]:.3f}; "
            f"twice that, rounded up, within [4, 8]: {factor}" + (" (the worst needs MORE than 8: a finding)"
                                                                  if 2 * worst[0] > 8 else ""),
            f"# worst: {worst[1]}",
            "# case, solve, cotangent: the ratio of " + ", ".join(helpers.MLP_GRAD_QUANTITIES) + " (each the larger of the whole "
            "tensor and its ragged tiles) | for information, the line's largest |kernels - oracle64| / |oracle32 - oracle64|, "
            "no floor taken off"]
    with open(path, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(head[:3]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mlp_gradient_rounding_ratios.txt"))
