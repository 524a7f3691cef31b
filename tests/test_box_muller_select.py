"""The float32 two-pair Box-Muller (torchsde_amd/csrc/tsde_rng.h: `box_muller2`) chooses between the log value and the
small-radius series with the execution mask instead of selects: the series runs on the first word where it is hot and on the
second elsewhere, its product is written into the first radius under the lanes of h0 and into the second under the lanes of h1,
the mask at entry is put back, and a block entered when h0 & h1 has a lane writes the series of the second word into the second
radius under h0 & h1. (The issue's other form -- the series on max(r.x, r.z), the block giving series(min) to the pair with the
smaller word -- measured slower and was not kept; `_two_pair_wave_max` restates it and is held to the same check, so that the
comparison of the two rests on equal results.)

This is a NumPy restatement of that selection, wave by wave (64 lanes, lane masks as boolean vectors, an entry mask that need
not be full), compared bit for bit with the per-pair definition (`box_muller`: the series of the pair's own word when it is
hot, its log value otherwise). The series is evaluated in exact rational arithmetic rounded to float32
(tests/test_box_muller_series.py). No GPU involved."""
from fractions import Fraction

import numpy as np

from tests.test_box_muller_series import _f32, _fma, _series_two_folded

HOT_FROM = 0xF0000000
WAVE = 64
EDGE = (0, 0xEFFFFFFF, 0xF0000000, 0xF0000001, 0xFFFFFFFE, 0xFFFFFFFF)
UNTOUCHED = np.float32(-7.0)            # what the registers of a lane hold that is not active at entry

_series_cache = {}


def _series_factors(a):
    """(w, p) of the series of first word `a` as float32: the series value is the float32 product w * p."""
    a = int(a)
    if a not in _series_cache:
        w = _fma(_f32(np.float32(np.uint32(~a & 0xFFFFFFFF))), Fraction(1, 1 << 32), Fraction(1, 1 << 33))
        ser, p = _series_two_folded(w)
        w32, p32 = np.float32(float(w)), np.float32(float(p))
        assert Fraction(float(w32)) == w and Fraction(float(p32)) == p
        assert Fraction(float(w32 * p32)) == ser            # NumPy's float32 product is the one rounding of w * p
        _series_cache[a] = (w32, p32)
    return _series_cache[a]


def _series(words):
    wp = [_series_factors(a) for a in words]
    return np.array([w for w, _ in wp], np.float32), np.array([p for _, p in wp], np.float32)


def _log(words):
    """-2 ln u1 on the log path. The selection only moves this value around; any function of the word would do."""
    u1 = (words.astype(np.float64) + 0.5) * 2.0 ** -32
    return (np.float32(-1.3862943611198906) * np.log2(u1).astype(np.float32)).astype(np.float32)


def _per_pair(words):
    w, p = _series(words)
    return np.where(words >= HOT_FROM, w * p, _log(words)).astype(np.float32)


def _masked_write(dst, value, exec_mask):
    """A vector instruction writes its result in the lanes of the execution mask and leaves the others alone."""
    dst[exec_mask] = value[exec_mask]


def _two_pair_wave(x, z, entry):
    """`box_muller2` on one wave: words x, z per lane, `entry` the lanes active on entry. Returns (s0, s1, entered, exec)."""
    assert x.shape == z.shape == entry.shape == (WAVE,)
    exec_mask = entry.copy()
    s0 = np.full(WAVE, UNTOUCHED, np.float32)
    s1 = np.full(WAVE, UNTOUCHED, np.float32)
    _masked_write(s0, _log(x), exec_mask)
    _masked_write(s1, _log(z), exec_mask)
    m0 = (x >= HOT_FROM) & exec_mask                # a compare writes a zero bit for a lane that is not active
    m1 = (z >= HOT_FROM) & exec_mask
    w, p = _series(np.where(m0, x, z))              # v_cndmask_b32 on the first mask
    saved = exec_mask.copy()
    exec_mask = m0
    _masked_write(s0, w * p, exec_mask)
    exec_mask = m1
    _masked_write(s1, w * p, exec_mask)
    exec_mask = saved
    both = m0 & m1                                  # scalar AND of the two masks
    entered = bool(both.any())
    if entered:
        w, p = _series(z)
        saved = exec_mask.copy()
        exec_mask = both
        _masked_write(s1, w * p, exec_mask)
        exec_mask = saved
    return s0, s1, entered, exec_mask


def _two_pair_wave_max(x, z, entry):
    """The form that was measured and not kept: the series on max(x, z), series(min) to the pair with the smaller word."""
    assert x.shape == z.shape == entry.shape == (WAVE,)
    exec_mask = entry.copy()
    s0 = np.full(WAVE, UNTOUCHED, np.float32)
    s1 = np.full(WAVE, UNTOUCHED, np.float32)
    _masked_write(s0, _log(x), exec_mask)
    _masked_write(s1, _log(z), exec_mask)
    m0 = (x >= HOT_FROM) & exec_mask
    m1 = (z >= HOT_FROM) & exec_mask
    w, p = _series(np.maximum(x, z))
    saved = exec_mask.copy()
    exec_mask = m0
    _masked_write(s0, w * p, exec_mask)
    exec_mask = m1
    _masked_write(s1, w * p, exec_mask)
    exec_mask = saved
    entered = bool((m0 & m1).any())
    if entered:
        lo = np.minimum(x, z)
        wl, pl = _series(lo)
        both = lo >= HOT_FROM
        first_smaller = x < z
        _masked_write(s0, np.where(both & first_smaller, wl * pl, s0), exec_mask)
        _masked_write(s1, np.where(both & ~first_smaller, wl * pl, s1), exec_mask)
    return s0, s1, entered, exec_mask


FORMS = [_two_pair_wave, _two_pair_wave_max]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_waves(pairs, entry_masks):
    """Every pair of `pairs` through the wave mirror, 64 at a time (the last wave padded with cold lanes), under each entry
    mask; returns how many waves entered the both-hot block."""
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    pad = (-len(pairs)) % WAVE
    pairs = np.concatenate([pairs, np.zeros((pad, 2), np.uint32)])
    entered_count = 0
    for k in range(0, len(pairs), WAVE):
        x, z = pairs[k:k + WAVE, 0].copy(), pairs[k:k + WAVE, 1].copy()
        want0, want1 = _per_pair(x), _per_pair(z)
        for entry, form in ((e, f) for e in entry_masks for f in FORMS):
            s0, s1, entered, exec_after = form(x, z, entry)
            assert np.array_equal(exec_after, entry)                        # the mask at entry, restored exactly
            assert entered == bool(((x >= HOT_FROM) & (z >= HOT_FROM) & entry).any())
            assert np.array_equal(_bits(s0[entry]), _bits(want0[entry])), [hex(v) for v in x[entry]]
            assert np.array_equal(_bits(s1[entry]), _bits(want1[entry])), [hex(v) for v in z[entry]]
            assert (s0[~entry] == UNTOUCHED).all() and (s1[~entry] == UNTOUCHED).all()
            entered_count += entered and form is _two_pair_wave
    return entered_count


def _entry_masks():
    full = np.ones(WAVE, bool)
    ragged5 = np.arange(WAVE) < 5
    ragged3 = np.arange(WAVE) < 3
    odd = np.arange(WAVE) % 2 == 1
    return [full, ragged5, ragged3, odd]


def test_series_of_distinct_hot_words_differ():
    """The mirror can tell whose series a lane was given."""
    hot = [a for a in EDGE if a >= HOT_FROM]
    values = {int(_bits(w * p)[0]) for w, p in (_series_factors(a) for a in hot)}
    assert len(values) == len(hot) - 1      # ~0xF0000000 and ~0xF0000001 round to the same float32, 2^28: one series value


def test_masked_selection_equals_the_per_pair_definition_on_the_edge_words():
    every = [(a0, a1) for a0 in EDGE for a1 in EDGE]           # all ordered pairs, equal words included
    assert len(every) == 36
    kinds = {(a0 >= HOT_FROM, a1 >= HOT_FROM) for a0, a1 in every}
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    assert _check_waves(every, _entry_masks()) >= 1
    # one pair per wave in lane 0, so that a wave holds nothing but that pair's class; waves without a both-hot lane stay out
    for a0, a1 in every:
        entered = _check_waves([(a0, a1)], [np.ones(WAVE, bool), np.arange(WAVE) < 1])
        assert entered == (2 if (a0 >= HOT_FROM and a1 >= HOT_FROM) else 0)
    # both-hot lanes only, of either order and equal
    hot = [a for a in EDGE if a >= HOT_FROM]
    assert _check_waves([(a0, a1) for a0 in hot for a1 in hot], _entry_masks()) == len(_entry_masks())


def test_masked_selection_equals_the_per_pair_definition_on_random_pairs_forced_hot():
    rng = np.random.default_rng(20241019)
    n = 1024
    pairs = rng.integers(0, 1 << 32, size=(4 * n, 2), dtype=np.uint64).astype(np.uint32)
    hot = np.uint32(HOT_FROM)
    pairs[0 * n:1 * n, 0] |= hot                      # first word hot, the second as drawn
    pairs[1 * n:2 * n, 1] |= hot                      # second word hot
    pairs[2 * n:3 * n] |= hot                         # both hot
    pairs[3 * n:4 * n] = pairs[3 * n:4 * n][:, ::-1] | hot      # both hot, and ...
    pairs[3 * n:3 * n + 64, 1] = pairs[3 * n:3 * n + 64, 0]    # ... a wave of equal words
    rng.shuffle(pairs[:3 * n])                       # waves that mix the classes
    x, z = pairs[:, 0] >= HOT_FROM, pairs[:, 1] >= HOT_FROM
    assert (x & z).sum() >= 2 * n and (x & ~z).sum() >= n // 2 and (~x & z).sum() >= n // 2
    assert _check_waves(pairs, _entry_masks()[:2]) > 0
