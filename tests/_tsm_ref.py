"""Shared by tests/test_tsm_cpu.py and tests/test_gpu_tsm.py: the test signal and a float64 reference of the time-scale stage
(WSOLA as include/fq3hip.h and DESIGN.md section 4.9 define it).  numpy only."""
import numpy as np

RATE = 24000
HS, N, DELTA = 240, 480, 240
N_SIGNAL = 24000

_cache = {}


def signal():
    """24000 float32 samples (seed 11): a vibrato voice of 8 harmonics gated into voiced stretches and near-silence, plus noise; the
    last quarter is uniform noise.  Made once, read-only."""
    if "x" not in _cache:
        rng = np.random.default_rng(11)
        n = N_SIGNAL
        t = np.arange(n) / 24000.0
        f0 = 110.0 * (1.0 + 0.08 * np.sin(2 * np.pi * 3.0 * t))
        phase = 2 * np.pi * np.cumsum(f0) / 24000.0
        voiced = sum((0.5 / k) * np.sin(k * phase + k) for k in range(1, 9))
        env = np.where(np.mod(t, 0.25) < 0.19, 1.0, 0.02)
        x = 0.6 * voiced * env + 0.05 * rng.standard_normal(n)
        x[n - n // 4:] = 0.5 * rng.uniform(-1.0, 1.0, n // 4)
        x = x.astype(np.float32)
        x.setflags(write=False)
        _cache["x"] = x
    return _cache["x"]


def hann(n=N):
    """periodic Hann window in float64"""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def a_of(s, P, hs=HS):
    return (int(s) * hs * int(P)) // 1000


def total(n, P):
    """T(n) = ceil(1000 n / P)"""
    return -((-int(n) * 1000) // int(P))


def need(s, P, hs=HS):
    if s == 0:
        return hs
    return max(a_of(s, P, hs), a_of(s - 1, P, hs) + hs) + hs + 2 * hs


def reach(S, P, hs=HS):
    """the oldest input sample segment S can still read: the start of its candidates or of its template, whichever is earlier"""
    return 0 if S == 0 else min(a_of(S, P, hs), a_of(S - 1, P, hs) + hs) - hs


def history_bound(P, hs=HS):
    """The history length the stage keeps (plan_ in csrc/fq3_tsm.hip, restated).  The next segment S is held back either by need(S) > n:
    then n - reach(S) is below |a(S) - a(S-1) - Hs| + 2 DELTA + N; or by the cap: then n <= a(S+1).  Steps of a() are floor or ceil of
    Hs P / 1000."""
    q = hs * int(P)
    dlo, dhi = q // 1000, -(-q // 1000)
    return max(max(abs(dhi - hs), abs(dlo - hs)) + 4 * hs, max(dhi, 2 * dhi - hs) + hs + 1)


def padded(x, lo, hi):
    """x[lo:hi] in float64 with zeros outside the stream"""
    out = np.zeros(hi - lo, dtype=np.float64)
    a, b = max(lo, 0), min(hi, len(x))
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def correlations(x, s, P, prev_pos):
    """(c64[2 DELTA + 1], abs64[2 DELTA + 1]) of segment s >= 1: sum_j x[a(s) + d + j] t[j] and sum_j |x t| for d in [-DELTA, DELTA],
    template t[j] = x[prev_pos + HS + j]"""
    a = a_of(s, P)
    t = padded(x, prev_pos + HS, prev_pos + HS + N)
    cand = padded(x, a - DELTA, a + DELTA + N)
    win = np.lib.stride_tricks.sliding_window_view(cand, N)          # [2 DELTA + 1, N]
    prod = win * t[None, :]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def wsola(x, P, w=None, deltas=None, dtype=np.float64):
    """Reference of a finished stream: (y[T(n)], delta[segments]) in float64.  ``deltas`` given: teacher-forced with them (the search
    is skipped); ``w``: the window to use (default: the float64 Hann).  ``dtype`` float32: the search accumulates in float32 (ascending
    j), for the margin study."""
    x64 = np.asarray(x, dtype=np.float64)
    w = hann() if w is None else np.asarray(w, dtype=np.float64)
    T = total(len(x64), P)
    n_seg = -(-T // HS)
    y = np.zeros(n_seg * HS, dtype=np.float64)
    out_d = np.zeros(n_seg, dtype=np.int64)
    prev = -HS
    for s in range(n_seg):
        a = a_of(s, P)
        if deltas is not None:
            d = int(deltas[s])
        elif s == 0:
            d = 0
        elif dtype == np.float32:
            t = padded(x64, prev + HS, prev + HS + N).astype(np.float32)
            cand = padded(x64, a - DELTA, a + DELTA + N).astype(np.float32)
            win = np.lib.stride_tricks.sliding_window_view(cand, N)
            acc = np.zeros(2 * DELTA + 1, dtype=np.float32)
            for j in range(N):
                acc = (acc + win[:, j] * t[j]).astype(np.float32)
            d = int(np.argmax(acc)) - DELTA
        else:
            c, _ = correlations(x64, s, P, prev)
            d = int(np.argmax(c)) - DELTA                            # the first maximum: ties to the smallest d
        pos = a + d
        y[s * HS:(s + 1) * HS] = w[:HS] * padded(x64, pos, pos + HS) + w[HS:] * padded(x64, prev + HS, prev + 2 * HS)
        out_d[s] = d
        prev = pos
    return y[:T], out_d
