"""profiles/prog_machine_accuracy.txt: the ulp errors of the program kernels' function opcodes and of torch's operators of the
same name on the device, per opcode, dtype, sign and binade -- the measurements tests/test_gpu_prog_machine.py asserts on
(`python tools/prog_machine_accuracy.py > profiles/prog_machine_accuracy.txt` on the MI355X)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TSDE_SPECIALISE", "0")

if __name__ == "__main__":
    from tests import test_gpu_prog_machine
    sys.stdout.write(test_gpu_prog_machine.accuracy_table())
