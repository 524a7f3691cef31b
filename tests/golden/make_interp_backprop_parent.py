"""Records what training through ``sdeint`` on the perceptron kernels returns for solves whose outputs ALL sit on step boundaries
-- values, dL/dy0 and every parameter gradient, with and without ``logqp=True`` -- so that a later build can be held to the same
bits (tests/test_gpu_interp_backprop.py, part D). interp_backprop_parent.npz was written by this script on the build BEFORE the
reverse sweep learnt outputs inside steps (commit b6b625f), on an MI355X:

    python tests/golden/make_interp_backprop_parent.py --package-root <checkout of that commit, built> [--out FILE]

`--package-root`: where `torchsde_amd` is imported from (default: this tree). Cases, seeds and cotangents are those of
tests/helpers_interp_backprop.py of THIS tree, which touches the package through its public calls only."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPE = (37, 20, 36)
SCHEMES = {"euler-sigmoid": ("euler", "sigmoid"), "milstein-affine": ("milstein", "affine")}
GRIDS = ("aligned", "every_step")
INDEX = 900


def case_of(route, scheme, grid):
    from tests import helpers_interp_backprop as I
    method, diffusion = SCHEMES[scheme]
    if route == "plain":
        return I.PlainCase(INDEX, SHAPE, (method, "ito", diffusion), "tanh", grid)
    return I.KlCase(INDEX, SHAPE, (method, None, diffusion), "softplus", grid)


def solve(route, scheme, grid, device):
    """{quantity: tensor} of the cotangent on every output: ys, [log_ratio,] y0 and every parameter's gradient."""
    from tests import helpers_interp_backprop as I
    return I.solve(case_of(route, scheme, grid), device)["all"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "interp_backprop_parent.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torchsde_amd
    assert os.path.abspath(torchsde_amd.__file__).startswith(os.path.abspath(args.package_root)), torchsde_amd.__file__
    sys.path.insert(0, ROOT)           # (`tests` of this tree; torchsde_amd stays the one imported above)
    import numpy as np
    out = {}
    for route in ("plain", "logqp"):
        for scheme in SCHEMES:
            for grid in GRIDS:
                for name, value in solve(route, scheme, grid, "cuda").items():
                    out[f"{route}/{scheme}/{grid}/{name}"] = value.cpu().numpy()
    np.savez_compressed(args.out, **out)
    print(f"{len(out)} arrays from {torchsde_amd.__file__} -> {args.out}")


if __name__ == "__main__":
    main()
