"""NumPy reference of the provenance watermark (include/fq3hip.h states the formulas): chips, embed and detect,
in float64 by default and in float32 (``dtype=np.float32``: the same formulas, every table and product in fp32) for the tests' error
bounds, and the deterministic synthetic voiced signal the tests mark.  A helper, not a test."""
import numpy as np

import _noise_ref

N, H, LO, BINS, PERIOD, SLOT = 512, 256, 11, 64, 128, 0xFFFFFFFE
OFFSETS = np.arange(0, 256, 8)
THRESHOLD = 6.0


def chips(key):
    """[128][64] of -1 / +1: bit (j & 31) of word 2 p + (j >> 5) of the Philox row (seed key, frame 0, slot 0xFFFFFFFE)."""
    w = _noise_ref.words(key, 0, SLOT, 2 * PERIOD).reshape(PERIOD, 2)
    j = np.arange(BINS)
    return ((w[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(np.float64) * 2.0 - 1.0


def _tables(dtype):
    i = np.arange(N)
    w = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * i / N))
    ang = 2 * np.pi * ((np.arange(LO, LO + BINS)[:, None] * i[None, :]) % N) / N                 # [bins][N]
    return (w * np.cos(ang)).astype(dtype), (-w * np.sin(ang)).astype(dtype)


def _frames(x, first, T, dtype):
    """frames 0 .. T - 1, frame t = x[first + t H - H, first + t H + H), zeros outside x"""
    pad = np.zeros((T + 1) * H, dtype=dtype)
    lo = first - H
    a, b = max(lo, 0), min(lo + len(pad), len(x))
    if b > a:
        pad[a - lo:b - lo] = x[a:b]
    return np.lib.stride_tricks.sliding_window_view(pad, N)[::H][:T]


def embed(x, key, a, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    T = -(-len(x) // H) + 1
    wc, ws = _tables(dtype)
    fr = _frames(x, 0, T, dtype)
    g = (dtype(a) * chips(key)[np.arange(T) % PERIOD]).astype(dtype)
    re, im = g * (fr @ wc.T), g * (fr @ ws.T)
    delta = (re @ (wc * dtype(2.0 / N)) + im @ (ws * dtype(2.0 / N))).astype(dtype)              # [T][N], windowed
    y = np.concatenate([x, np.zeros(T * H - len(x), dtype=dtype)])
    y[:(T - 1) * H] = (y[:(T - 1) * H] + delta[:-1, H:].reshape(-1)) + delta[1:, :H].reshape(-1)
    return y[:len(x)]


def detect_table(r, key, dtype=np.float64):
    """z[32][128]"""
    r = np.asarray(r, dtype=dtype)
    T = -(-len(r) // H) + 1
    wc, ws = _tables(dtype)
    c = chips(key).astype(dtype)
    rows = (np.arange(1, T - 1)[:, None] + np.arange(PERIOD)[None, :]) % PERIOD                   # [t][phase]
    z = np.zeros((len(OFFSETS), PERIOD), dtype=dtype)
    for oi, o in enumerate(OFFSETS):
        fr = _frames(r, int(o), T, dtype)
        re, im = fr @ wc.T, fr @ ws.T
        L = np.log(np.sqrt(re * re + im * im) + dtype(1e-9))
        d = np.clip(L[1:-1] - dtype(0.5) * (L[:-2] + L[2:]), -2, 2).astype(dtype)
        e = np.sum(d * d)
        if e > 0:
            z[oi] = np.einsum("tj,tpj->p", d, c[rows]) / np.sqrt(e)
    return z


def verdict(z):
    """(max z, offset, phase, present)"""
    oi, ph = np.unravel_index(int(np.argmax(z)), z.shape)
    return float(z[oi, ph]), int(OFFSETS[oi]), int(ph), bool(z[oi, ph] >= THRESHOLD)


def voiced(seconds, seed=7, rate=24000):
    """a harmonic stack with moving f0, a 2.3 Hz envelope and a noise floor; float32, peak below 0.5"""
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    f0 = 140.0 + 35.0 * np.sin(2 * np.pi * 0.7 * t) + 12.0 * np.sin(2 * np.pi * 3.1 * t)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k ** 1.2 for k in range(1, 40))
    x = x * (0.55 + 0.45 * np.sin(2 * np.pi * 2.3 * t)) + 0.02 * rng.standard_normal(n)
    return (0.45 * x / np.max(np.abs(x))).astype(np.float32)
