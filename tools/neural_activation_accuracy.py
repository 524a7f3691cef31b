"""profiles/neural_activation_accuracy.txt: the error of the activations and slopes the matrix-core kernels form (the eleven sites
of tests/neural_activation_forms.py), per site, quantity, sign and binade, next to the CPU emulation of the site's formula and
to torch float32's own operator on the device -- the measurements tests/test_gpu_neural_activations.py asserts on
(`python tools/neural_activation_accuracy.py > profiles/neural_activation_accuracy.txt` on the MI355X)."""
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from tests import test_gpu_neural_activations
    with contextlib.redirect_stdout(io.StringIO()):          # (the tests print each figure before they assert)
        table = test_gpu_neural_activations.accuracy_table()
    sys.stdout.write(table)
