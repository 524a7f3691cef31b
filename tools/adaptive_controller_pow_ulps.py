"""Measure how far the device controller's proposed step sizes (csrc/adaptive.hip: two `pow` calls of the device's libm) lie
from CPython's (tests/adaptive_model.py) and from the correctly rounded value (mpmath), over every unclamped call of the
sequences of tests/test_gpu_adaptive_controller.py. Needs the GPU:

    python tools/adaptive_controller_pow_ulps.py > profiles/adaptive_controller_pow_ulps.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_adaptive_controller as G  # noqa: E402


def main():
    records, worst, worst_dev, worst_py = G.measure_pow_ulps()
    print("Proposed step size of adaptive_control_kernel against tests/adaptive_model.py (CPython doubles), one controller call at a")
    print("time from the same state; calls whose factor is clamped (facmin, facmax, dt_min) are compared exactly and not listed.")
    print(f"{'error':>24} {'prev step':>24} {'prev ratio':>24} {'device':>24} {'CPython':>24} ulps")
    for err, step, ratio, d, m in records:
        print(f"{err!r:>24} {step!r:>24} {ratio!r:>24} {d.hex():>24} {m.hex():>24} {G.ulps_apart(d, m)}")
    print(f"unclamped calls: {len(records)}")
    print(f"worst device - CPython: {worst} ulps of a double")
    if worst_dev is not None:
        print(f"worst device - correctly rounded (mpmath, 200 bits): {worst_dev:.3f} ulps")
        print(f"worst CPython - correctly rounded (mpmath, 200 bits): {worst_py:.3f} ulps")
    else:
        print("mpmath not importable: no correctly rounded column")
    print(f"bound asserted per call: max(4, 2 x {worst}) = {max(4, 2 * worst)} ulps "
          f"(POW_ULPS_MEASURED = {G.POW_ULPS_MEASURED} in the test module)")


if __name__ == "__main__":
    main()
