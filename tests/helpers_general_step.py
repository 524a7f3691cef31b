"""What `launch_step_general` (csrc/steps.hip) decides, restated in Python, and the table of cases that
tests/test_gpu_general_step.py runs: every entry says which kernel, instantiation and rows-per-wave it is there to reach.
tests/test_general_step_cases.py holds the table to the restatement on the CPU, so a change of the launcher's thresholds --
once it is made here too -- shows which class lost its case, instead of a kernel going quietly uncovered."""
import collections
import os

K_BLOCK = 256            # csrc/tsde_common.h: kBlock
K_GEN_MAX_NOISE = 2048   # csrc/steps.hip: kGenMaxNoise, the staged increments of the generic kernel (and the largest m)
NC_SERVED = (1, 2, 4, 8)


def default_min_waves():
    """`min_waves` of the launcher: TSDE_GENERAL_MIN_WAVES, else 4096."""
    e = os.environ.get("TSDE_GENERAL_MIN_WAVES")
    return int(e) if e else 4096


def path(B, d, m, g_aligned=True, noise_ok=True, min_waves=None):
    """The kernel a launch takes: ("rows", NC, RW), ("fast",), ("generic", rows_per_tile) or ("error",); ("empty",) for
    the launch that is none (B or d zero). `g_aligned`: g sits on a 16-byte boundary; `noise_ok`: external increments
    do too, or a generated cell starts at an element offset that is a multiple of 4 (`general_noise_ok`)."""
    if min_waves is None:
        min_waves = default_min_waves()
    if B <= 0 or d <= 0:
        return ("empty",)
    if m <= 0 or m > K_GEN_MAX_NOISE:
        return ("error",)
    G = m // 4
    pow2 = m % 4 == 0 and 1 <= G <= 64 and (G & (G - 1)) == 0
    fast = pow2 and g_aligned and noise_ok
    if fast and (d * G) % 64 == 0 and (d * G) // 64 in NC_SERVED:
        rw = 64 // G
        while rw > 1 and (B + rw - 1) // rw < min_waves:
            rw >>= 1
        return ("rows", (d * G) // 64, rw)
    if fast:
        return ("fast",)
    rows = min(K_GEN_MAX_NOISE // m, (2 * K_BLOCK + d - 1) // d)
    return ("generic", max(rows, 1))


# `view`: which operand is a view one element into a larger buffer (off its 16-byte boundary): "g", "dW" (external increments;
# the generated twin of that case starts its cell at element offset 2, the other way to fail `general_noise_ok`), or None.
Case = collections.namedtuple("Case", "B d m view expect")

ROWS_SHAPES = {1: [(64, 4), (16, 16), (2, 128)], 2: [(32, 16), (128, 4)], 4: [(32, 32), (16, 64)], 8: [(64, 32), (8, 256)]}
FAST_SHAPES = [(3, 4), (48, 4), (5, 8), (7, 16), (100, 8), (192, 4), (3, 256)]
GENERIC_SHAPES = {(5, 3): 103, (4, 6): 128, (9, 1): 57, (16, 12): 32, (2, 2048): 1, (600, 5): 1}      # -> rows_per_tile
SMALL_BATCHES = (1, 37)          # both below 8191 rows: RW = 1


def _small_cases():
    out = []
    for B in SMALL_BATCHES:
        for nc, shapes in ROWS_SHAPES.items():
            out += [Case(B, d, m, None, ("rows", nc, 1)) for d, m in shapes]
        out += [Case(B, d, m, None, ("fast",)) for d, m in FAST_SHAPES]
        out += [Case(B, d, m, None, ("generic", rows)) for (d, m), rows in GENERIC_SHAPES.items()]
        # a rows shape (NC = 2) whose g, or whose increments, are off the 16-byte boundary: the generic kernel, 16 rows a tile
        out += [Case(B, 32, 16, "g", ("generic", 16)), Case(B, 32, 16, "dW", ("generic", 16))]
    return out


CASES = _small_cases()
ERROR_CASE = Case(1, 1, K_GEN_MAX_NOISE + 1, None, ("error",))

# The ladder of rows per wave at min_waves = 4096: RW starts at 64 / G and halves while ceil(B / RW) < 4096.
# `last`: rows in the last group (ragged: 0 < last < RW). The largest g, (64, 4) at B = 262147, is 268 MB in float32.
Ladder = collections.namedtuple("Ladder", "d m nc B rw last dtypes")
LADDER = [
    Ladder(16, 16, 1, 8195, 2, 1, ("float32",)),
    Ladder(32, 16, 2, 16387, 4, 3, ("float32",)),
    Ladder(32, 32, 4, 32771, 8, 3, ("float32",)),
    Ladder(64, 32, 8, 32771, 8, 3, ("float32",)),
    Ladder(16, 16, 1, 65541, 16, 5, ("float32", "float64")),
    Ladder(64, 4, 1, 262147, 64, 3, ("float32",)),
]
SHARD_ROWS = 37


def shard_ranges(case):
    """Row ranges [lo, lo + 37) of a ladder case that are launched alone (RW = 1) and compared with the big launch: the
    first rows, a range that straddles a group boundary, and the last rows with the ragged group."""
    return [0, case.rw * 1000 + case.rw - 3, case.B - SHARD_ROWS]


def noise_ok_of(case):
    return case.view != "dW"


def expected_path(case, min_waves=4096):
    return path(case.B, case.d, case.m, g_aligned=case.view != "g", noise_ok=noise_ok_of(case), min_waves=min_waves)
