"""CPU: the segment join stage's contract (include/fq3hip.h): hand-computed known answers of the NumPy
reference (tests/_join_ref.py), and the host-only half of the library -- fq3_join_bound against the reference's worst case, the
range errors of fq3_join_create / fq3_join_bound / fq3_join_push, all answered before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import _join_ref as R
from fq3hip import _lib

RATE, H = 24000, 240
THR, LEAD, TAIL, HOLD = 0.25, 1, 2, 4


def _seg(*parts):
    """('t' | 'q', hops or samples as a float of hops) -> a tone of 0.5 / a quiet 0.1, so that every kept sample is recognisable"""
    out = []
    for kind, n in parts:
        out.append(np.full(int(n), 0.5 if kind == "t" else 0.1, np.float32))
    x = np.concatenate(out) if out else np.zeros(0, np.float32)
    return x + np.arange(x.size, dtype=np.float32) * np.float32(1e-6)         # every sample distinct: a shifted copy would show


def _join(segs, lead=LEAD, tail=TAIL, hold=HOLD, thr=THR, **kw):
    return R.join(segs, RATE, thr, lead, tail, hold, **kw)


def test_silence_tone_silence():
    x = _seg(("q", 5 * H), ("t", 6 * H), ("q", 7 * H))
    # a = 5, b = 10, last = 17, L = 7, R = min(max(0, 7 - 2), 4) = 4: hops [4, 13] = one hop of lead, the tone, L - R = 3 hops of tail
    assert np.array_equal(_join([(x, 100)]), x[4 * H: 14 * H])
    # followed by another segment: the pause of zeros goes behind it
    y = _seg(("t", 2 * H))
    got = _join([(x, 100), (y, 7)])
    assert np.array_equal(got, np.concatenate([x[4 * H: 14 * H], np.zeros(100, np.float32), y]))
    assert np.array_equal(_join([(x, 100)], last_pause=True), np.concatenate([x[4 * H: 14 * H], np.zeros(100, np.float32)]))


def test_all_silent_segment_gives_nothing_and_no_pause():
    s = _seg(("q", 9 * H + 17))
    y = _seg(("t", 2 * H))
    assert _join([(s, 500)]).size == 0
    assert np.array_equal(_join([(s, 500), (y, 0)]), y)
    assert np.array_equal(_join([(y, 3), (s, 500), (y, 0)]), np.concatenate([y, np.zeros(3, np.float32), y]))
    assert _join([(np.zeros(0, np.float32), 500)]).size == 0                  # an empty segment as well


def test_no_silence_at_all():
    x = _seg(("t", 5 * H + 100))
    assert np.array_equal(_join([(x, 0)]), x)


@pytest.mark.parametrize("trail, kept", [(0, 0), (1, 1), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (7, 3), (20, 16)])
def test_trailing_silence_against_tail_and_hold(trail, kept):
    """tail 2, hold 4.  L <= tail: everything stays; tail < L <= tail + hold: R = L - tail, `tail` hops stay; beyond: R = hold, L - hold
    hops stay (the queue released them before the segment's end was known)."""
    x = _seg(("t", 3 * H), ("q", trail * H))
    assert np.array_equal(_join([(x, 0)]), x[: (3 + kept) * H])


def test_hold_equal_and_shorter_than_tail_edge():
    # tail == hold == 3: L = 3 stays whole, L = 4 keeps 3, L = 7 keeps max(3, 7 - 3) = 4
    for trail, kept in ((3, 3), (4, 3), (6, 3), (7, 4)):
        x = _seg(("t", 2 * H), ("q", trail * H))
        assert np.array_equal(_join([(x, 0)], tail=3, hold=3), x[: (2 + kept) * H]), trail
    # hold == 0: nothing can wait, so every trailing hop was released before the end was known (R = min(L, 0) = 0); lead 0: no pre-roll
    x = _seg(("q", 2 * H), ("t", 2 * H), ("q", 5 * H))
    assert np.array_equal(_join([(x, 0)], lead=0, tail=0, hold=0), x[2 * H:])
    # tail 0 under a hold that covers the silence: every trailing silent hop goes
    assert np.array_equal(_join([(x, 0)], lead=0, tail=0, hold=5), x[2 * H: 4 * H])


def test_sample_exactly_at_the_threshold_is_active():
    x = np.full(3 * H, 0.1, np.float32)
    assert _join([(x, 0)]).size == 0
    x[H + 7] = np.float32(THR)
    assert np.array_equal(_join([(x, 0)]), x)                                   # hop 1 active; one hop of lead, one of tail
    x[H + 7] = np.nextafter(np.float32(THR), np.float32(0))
    assert _join([(x, 0)]).size == 0
    x[H + 7] = -np.float32(THR)
    assert np.array_equal(_join([(x, 0)]), x)                                   # |x|
    x[H + 7] = np.float32("nan")
    assert _join([(x, 0)]).size == 0                                            # a NaN compares false


def test_short_last_hop():
    # active short hop: kept to the segment's end
    x = _seg(("q", 4 * H), ("t", H + 31))
    assert np.array_equal(_join([(x, 0)]), x[3 * H:])
    # silent short hop counts as a hop: last = 6, b = 3, L = 3, R = 1 -> the short hop goes, two whole ones stay
    x = _seg(("t", 4 * H), ("q", 2 * H + 1))
    assert np.array_equal(_join([(x, 0)]), x[: 6 * H])
    # L = 2 with a short last hop: everything stays, the end is the segment's end
    x = _seg(("t", 4 * H), ("q", H + 1))
    assert np.array_equal(_join([(x, 0)]), x)
    # a segment shorter than a hop; a lead that reaches in front of the segment
    x = _seg(("t", 100))
    assert np.array_equal(_join([(x, 0)]), x)
    x = _seg(("q", H // 2), ("t", 2 * H))
    assert np.array_equal(_join([(x, 0)], lead=5), x)


def test_internal_silence_is_never_touched():
    x = _seg(("q", 3 * H), ("t", 2 * H), ("q", (HOLD + 3) * H), ("t", 2 * H), ("q", 6 * H))
    assert np.array_equal(_join([(x, 0)]), x[2 * H: (3 + 2 + HOLD + 3 + 2 + 2) * H])


# ---- the library's host-only half -------------------------------------------------------------------------------------------------
def _bound(cfg, n, pause):
    return _lib.load().fq3_join_bound(None if cfg is None else C.byref(cfg), n, pause)


def test_bound_against_the_reference_worst_case():
    lib = _lib.load()
    for rate, lead, tail, hold in ((24000, 1, 2, 4), (8000, 0, 0, 0), (48000, 16, 400, 400), (24000, 2, 5, 100)):
        cfg = _lib.JoinConfig(rate, 0.005, lead, tail, hold)
        h = rate // 100
        for n, pause in ((0, 0), (1, 0), (h, 5), (23040, 7200), (1 << 40, 5 * rate)):
            assert _bound(cfg, n, pause) == R.bound(rate, lead, hold, n, pause) == n + (hold + lead + 1) * h + pause
    # the worst a push can settle: everything the object may hold from earlier pushes (the queue or the pre-roll, and a partial hop)
    # plus all of its own samples plus the pause -- e.g. `hold` silent hops and H - 1 samples pending, then one loud sample ends the segment
    rate, lead, tail, hold, h = 24000, 1, 2, 4, 240
    cfg = _lib.JoinConfig(rate, THR, lead, tail, hold)
    seg = np.concatenate([np.full(h, 0.5, np.float32), np.full(hold * h + h - 1, 0.1, np.float32), np.full(1, 0.5, np.float32)])
    whole = R.join([(seg, 2400)], rate, THR, lead, tail, hold, last_pause=True)
    before = R.join([(seg[:h], 0)], rate, THR, lead, tail, hold)               # what left before the last one-sample push: the first hop
    settled = whole.size - before.size
    assert settled == hold * h + h - 1 + 1 + 2400
    assert settled <= _bound(cfg, 1, 2400)
    assert max(hold, lead) * h + h - 1 <= (hold + lead + 1) * h                # the state bound covers both phases' pending samples
    assert isinstance(lib.fq3_last_error(), bytes)


def test_bound_and_create_range_errors():
    lib = _lib.load()
    ok = dict(in_rate=24000, threshold=0.005, lead_hops=2, tail_hops=5, hold_hops=100)
    assert _bound(_lib.JoinConfig(*ok.values()), 0, 0) > 0
    bad = [dict(in_rate=7900), dict(in_rate=48100), dict(in_rate=22050), dict(in_rate=0), dict(threshold=0.0), dict(threshold=1.0),
           dict(threshold=-0.1), dict(threshold=float("nan")), dict(lead_hops=-1), dict(lead_hops=17), dict(tail_hops=-1),
           dict(tail_hops=101), dict(hold_hops=401), dict(hold_hops=-1), dict(hold_hops=4, tail_hops=5)]
    for change in bad:
        c = dict(ok, **change)
        cfg = _lib.JoinConfig(c["in_rate"], c["threshold"], c["lead_hops"], c["tail_hops"], c["hold_hops"])
        h = C.c_void_p()
        assert lib.fq3_join_create(C.byref(cfg), C.byref(h)) == _lib.FQ3_EINVAL, change       # before any HIP call: safe without a GPU
        assert not h.value and b"join" in lib.fq3_last_error()
        assert _bound(cfg, 10, 0) == _lib.FQ3_EINVAL, change
    cfg = _lib.JoinConfig(*ok.values())
    assert _bound(cfg, -1, 0) == _lib.FQ3_EINVAL and _bound(cfg, (1 << 40) + 1, 0) == _lib.FQ3_EINVAL
    assert _bound(cfg, 0, -1) == _lib.FQ3_EINVAL and _bound(cfg, 0, 5 * 24000 + 1) == _lib.FQ3_EINVAL
    assert _bound(None, 0, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_join_create(None, None) == _lib.FQ3_EINVAL and lib.fq3_join_create(C.byref(cfg), None) == _lib.FQ3_EINVAL
    assert lib.fq3_join_destroy(None) == 0
    assert lib.fq3_join_reset(None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_join_push(None, None, 0, 0, 0, None, 0, None, None) == _lib.FQ3_EINVAL


def test_python_spec_refuses_what_the_library_refuses():
    from fq3hip.long_form import join_bound
    assert join_bound(24000, 0.005, 2, 5, 100, 23040, 7200) == 23040 + 103 * 240 + 7200
    for args in ((22050, 0.005, 2, 5, 100), (24000, 1.5, 2, 5, 100), (24000, 0.005, 2, 6, 5)):
        with pytest.raises(ValueError):
            join_bound(*args, 0, 0)
