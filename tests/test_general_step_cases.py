"""The case table of tests/test_gpu_general_step.py reaches every class of `launch_step_general` (csrc/steps.hip) that it
says it reaches -- checked on the CPU against the restatement of the launcher's decision in tests/helpers_general_step.py."""
from tests import helpers_general_step as H

MIN_WAVES = 4096


def test_every_annotation_is_what_the_launcher_decides():
    for case in H.CASES + [H.ERROR_CASE]:
        assert H.expected_path(case, MIN_WAVES) == case.expect, case
    for lad in H.LADDER:
        assert H.path(lad.B, lad.d, lad.m, min_waves=MIN_WAVES) == ("rows", lad.nc, lad.rw), lad
        assert lad.B % lad.rw == lad.last, lad
        # a shard of 37 rows runs one row per wave, on the same instantiation
        assert H.path(H.SHARD_ROWS, lad.d, lad.m, min_waves=MIN_WAVES) == ("rows", lad.nc, 1), lad
        lo_first, lo_straddle, lo_last = H.shard_ranges(lad)
        assert lo_first == 0 and lo_last + H.SHARD_ROWS == lad.B
        assert lo_straddle % lad.rw != 0 or lad.rw == 1                                  # starts inside a group ...
        assert lo_straddle // lad.rw < (lo_straddle + H.SHARD_ROWS - 1) // lad.rw        # ... and ends in a later one
        assert 0 < lo_straddle and lo_straddle + H.SHARD_ROWS <= lo_last, lad


def test_the_table_contains_every_class():
    paths = [c.expect for c in H.CASES + [H.ERROR_CASE]] + [("rows", lad.nc, lad.rw) for lad in H.LADDER]
    rows = [p for p in paths if p[0] == "rows"]
    assert {p[1] for p in rows} == {1, 2, 4, 8}
    assert {p[2] for p in rows} == {1, 2, 4, 8, 16, 64}
    for nc in (1, 2, 4, 8):       # a ragged last group on more than one row per wave, in every instantiation
        assert any(lad.nc == nc and lad.rw > 1 and 0 < lad.last < lad.rw for lad in H.LADDER), nc
    # a partial sub-batch (SB = 8 / NC rows are loaded together) in the ragged group of the instantiations that have one
    for nc in (1, 2, 4):
        assert any(lad.nc == nc and lad.last % (8 // nc) != 0 for lad in H.LADDER), nc
    assert ("fast",) in paths
    generic = [p[1] for p in paths if p[0] == "generic"]
    assert 1 in generic and any(r > 1 for r in generic)
    assert ("error",) in paths
    # the fallbacks: a rows shape that goes to the generic kernel because g, or the increments, are unaligned
    assert {c.view for c in H.CASES if c.expect[0] == "generic" and (c.d, c.m) == (32, 16)} == {"g", "dW"}
    # every shape at both small batches
    for B in H.SMALL_BATCHES:
        shapes = {(c.d, c.m) for c in H.CASES if c.B == B}
        wanted = set(H.FAST_SHAPES) | set(H.GENERIC_SHAPES) | {s for v in H.ROWS_SHAPES.values() for s in v}
        assert shapes == wanted


def test_restatement_edges():
    assert H.path(0, 3, 4) == ("empty",) and H.path(5, 0, 4) == ("empty",)
    assert H.path(5, 3, 0, min_waves=MIN_WAVES) == ("error",)
    assert H.path(5, 3, 2048, min_waves=MIN_WAVES) == ("generic", 1)
    # every launch below 8191 rows runs one row per wave; 8191 rows are 4096 pairs
    assert H.path(8190, 16, 16, min_waves=MIN_WAVES) == ("rows", 1, 1)
    assert H.path(8191, 16, 16, min_waves=MIN_WAVES) == ("rows", 1, 2)
    assert H.path(8191, 16, 16, min_waves=1) == ("rows", 1, 16)
    # NC = 3 is not served; G = 128 is not a lane count
    assert H.path(37, 48, 16, min_waves=MIN_WAVES) == ("fast",)
    assert H.path(37, 4, 512, min_waves=MIN_WAVES) == ("generic", 4)
