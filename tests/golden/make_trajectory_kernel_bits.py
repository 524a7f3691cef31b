"""Records ``trajectory_kernel_bits.json``: for every case of tests/test_gpu_trajectory_bits.py, the SHA-256 of the bytes the
kernel wrote and eight sampled values. Run on an MI355X, from the root of a tree whose library is the build to pin (the commit
before a refactor of csrc/trajectory.hip), with that tree's own copy of the test module:

    python tests/golden/make_trajectory_kernel_bits.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests import test_gpu_trajectory_bits as bits  # noqa: E402


def main(path):
    import torch
    cases = {case: bits.digest(bits.run_case(case)) for case in bits.CASES}
    with open(path, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "cases": cases}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{path}: {len(cases)} cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "trajectory_kernel_bits.json"))
