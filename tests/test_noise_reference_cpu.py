"""CPU: the seeded-noise contract as tests/_noise_ref.py implements it -- pinned known answers, the range of
the variate in both storage types, its distribution, and that every plausible implementation slip is caught by a pinned vector."""
import math

import numpy as np
import pytest

import _noise_ref as R


def _hex(ws):
    return " ".join(f"{int(w):08x}" for w in ws)


# Philox4x32-10 known answers: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
W_1234 = "2090b348 da7cf0ab 4401906f cbca470e 9eeede35 1cbe137c fa277093 147edd50"
E_1234 = "2.0619323 0.15844612 1.3255798 0.22808668 0.47669414 2.1868014 0.02310045 2.524969".split()
W_1234_FIRST = "ab2cfba4 d35d7331 f3a5f4c3 79a03acc"
E_1234_FIRST = "0.4024869 0.19159077 0.04945178 0.7442275".split()
# the same variates as fp32 bit patterns (the decimals above name them only to their last printed place), and rounded once more to bf16
B_1234 = "4003f6b3 3e223fb3 3fa9ac99 3e698f8e 3ef41141 400bf48e 3cbd3d25 40219918"
B_1234_FIRST = "3ece12c3 3e44305f 3d4a8df2 3f3e85b2"
H_1234 = "4004 3e22 3faa 3e6a 3ef4 400c 3cbd 4022"


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert _hex([int(x) for x in R.philox(*ctr, *key)]) == want


def _same_f32(got, want):
    """the pinned decimals are fp32 values as NumPy prints an array of them: the shortest decimal that names the value, cut to at most
    8 decimal places.  The value must round to the literal at the literal's own number of places."""
    got = np.asarray(got, np.float32).astype(np.float64)
    if got.shape != (len(want),):
        return False
    return all(abs(g - float(w)) <= 0.5 * 10.0 ** -len(w.split(".")[1]) + 1e-15 for g, w in zip(got, want))


def _pinned_ok(**mutant):
    """Do the two seed-1234 vectors hold under this (possibly mutated) implementation?"""
    shift = mutant.get("shift", 9)
    wm = {k: v for k, v in mutant.items() if k != "shift"}
    w0, w1 = R.words(1234, 0, 0, 8, **wm), R.words(1234, 0, R.FIRST_SLOT, 4, **wm)
    e0, e1 = R.variates(w0, shift), R.variates(w1, shift)
    return (_hex(w0) == W_1234 and _hex(w1) == W_1234_FIRST and _same_f32(e0, E_1234) and _same_f32(e1, E_1234_FIRST)
            and _hex(e0.view(np.uint32)) == B_1234 and _hex(e1.view(np.uint32)) == B_1234_FIRST)


def test_seed_1234_vectors():
    assert _hex(R.words(1234, 0, 0, 8)) == W_1234
    assert _same_f32(R.row(1234, 0, 0, 8), E_1234)
    assert _hex(R.words(1234, 0, R.FIRST_SLOT, 4)) == W_1234_FIRST
    assert _same_f32(R.first_row(1234, 4), E_1234_FIRST)
    # bit for bit, and the bit patterns are the values the decimals name
    assert _hex(R.row(1234, 0, 0, 8).view(np.uint32)) == B_1234 and _hex(R.first_row(1234, 4).view(np.uint32)) == B_1234_FIRST
    assert _same_f32(np.array([int(h, 16) for h in B_1234.split()], np.uint32).view(np.float32), E_1234)
    assert _same_f32(np.array([int(h, 16) for h in B_1234_FIRST.split()], np.uint32).view(np.float32), E_1234_FIRST)
    assert " ".join(f"{int(b):04x}" for b in R.to_bf16_bits(R.row(1234, 0, 0, 8))) == H_1234
    assert _pinned_ok()


@pytest.mark.parametrize("mutant", [dict(rounds=9), dict(swap_multipliers=True), dict(bump_key=False), dict(shift=8),
                                    dict(v_swapped=True), dict(slot_frame_swapped=True)],
                         ids=["nine_rounds", "swapped_multipliers", "key_not_advanced", "shift_8", "v_index_swapped", "slot_frame_swapped"])
def test_every_mutant_is_rejected_by_a_pinned_vector(mutant):
    assert not _pinned_ok(**mutant)


def test_key_halves_and_row_prefix():
    # the high half of the seed is the second key word; a row's prefix does not depend on V
    assert not np.array_equal(R.words(5, 3, 1, 16), R.words(5 + 2 ** 32, 3, 1, 16))
    assert np.array_equal(R.words(2 ** 64 - 1, 3, 1, 1283)[:7], R.words(2 ** 64 - 1, 3, 1, 7))


def test_strictly_positive_and_finite_in_both_storage_types():
    e = R.row(1234, 7, 0, 1 << 20)
    assert np.isfinite(e).all() and (e > 0).all()
    b = R.bf16_bits_to_f32(R.to_bf16_bits(e))
    assert np.isfinite(b).all() and (b > 0).all()
    # the ends of the range: k = 2^23 - 1 and k = 0
    lo, hi = R.variates(np.array([0xFFFFFFFF, 0], np.uint32))
    assert 5.9e-8 < lo < 6.0e-8 and 16.63 < hi < 16.64
    ends = R.bf16_bits_to_f32(R.to_bf16_bits(np.array([lo, hi], np.float32)))
    assert np.isfinite(ends).all() and (ends > 0).all()


@pytest.mark.parametrize("seed", [1234, 2 ** 63 + 5])
def test_kolmogorov_smirnov_against_exp1(seed):
    n = 1 << 20
    x = np.sort(R.row(seed, 7, 0, n).astype(np.float64))
    cdf = -np.expm1(-x)
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    print(f"seed {seed}: D sqrt(n) = {d * math.sqrt(n):.3f}")
    assert d * math.sqrt(n) < 1.95          # the 0.1 % point of the Kolmogorov distribution


def test_consecutive_frames_are_uncorrelated():
    a, b = R.row(1234, 7, 0, 1 << 16).astype(np.float64), R.row(1234, 8, 0, 1 << 16).astype(np.float64)
    r = float(np.corrcoef(a, b)[0, 1])
    print(f"correlation of frames 7 and 8: {r:.4f}")
    assert abs(r) < 0.02
