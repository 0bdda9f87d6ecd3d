"""CPU reference of the loudness stage (include/fq3hip.h, "Loudness").  Three pieces:

``measure64`` / ``hop_energies64``   the float64 measure: ``scipy.signal.lfilter`` with the double-precision design run as the TRUE
                                     recursive filter over the whole signal (no per-hop restart), float gating
``emulate_hops``                     the contract in float32: per-hop restart from zero state, the contract's op order, ``fmaf`` emulated
                                     as a float64 product and sum rounded once to float32, integer energies
``gate``                             the integer gating and the gain with Python ints and floats, fed with hop integers and a peak

The gain constants and the absolute gate come from the library's design call (``fq3hip.loudness.design``), as the contract says: ``pow``
may differ by an ulp between libraries."""
import math

import numpy as np
from scipy.signal import lfilter

SCALE = 1099511627776.0          # 2^40
ABS_GATE_POWER = 10.0 ** ((-70.0 + 0.691) / 10.0)


def design64(rate):
    """(shelf b, shelf a, high-pass b, high-pass a) in double: the bilinear-transform construction of the K-weighting"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    sa = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return sb, sa, [1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def kweight64(x, rate):
    sb, sa, hb, ha = design64(rate)
    return lfilter(hb, ha, lfilter(sb, sa, np.asarray(x, dtype=np.float64)))


def hop_energies64(x, rate):
    """sum of y^2 over every whole hop of rate / 10 samples, float64, from the true recursive filter"""
    H = rate // 10
    y = kweight64(x, rate)
    n = len(y) // H
    return (y[:n * H].reshape(n, H) ** 2).sum(axis=1)


def measure64(x, rate):
    """integrated gated loudness in LUFS (BS.1770-4, mono) by the float64 measure; -inf without a block above the absolute gate"""
    H = rate // 10
    e = hop_energies64(x, rate)
    if len(e) < 4:
        return float("-inf")
    z = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * H)
    g1 = z[z > ABS_GATE_POWER]
    if len(g1) == 0:
        return float("-inf")
    g2 = g1[g1 > 0.1 * g1.mean()]
    return -0.691 + 10.0 * math.log10(g2.mean())


def _fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _biquad(c, x, s1, s2):
    b0, b1, b2, a1, a2 = c
    u = _fmaf(b0, x, s1)
    s1 = _fmaf(-a1, u, _fmaf(b1, x, s2))
    s2 = _fmaf(-a2, u, b2 * x)
    return u, s1, s2


def emulate_hops(x, coef32, H):
    """The contract in float32 -> the hop integers E_h as a uint64 array (whole hops only).  ``coef32``: the ten float32 coefficients
    of the design call."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x) // H
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    c = [np.float32(v) for v in coef32]
    shelf = [np.full(n, v, dtype=np.float32) for v in c[:5]]
    hp = [np.full(n, v, dtype=np.float32) for v in c[5:]]
    xp = np.concatenate([np.zeros(H, dtype=np.float32), x[:n * H]])
    rows = np.lib.stride_tricks.as_strided(xp, shape=(n, 2 * H), strides=(H * 4, 4))       # row h: hops h - 1 and h
    s1 = s2 = t1 = t2 = np.zeros(n, dtype=np.float32)
    e = np.zeros(n, dtype=np.uint64)
    for j in range(2 * H):
        u, s1, s2 = _biquad(shelf, np.ascontiguousarray(rows[:, j]), s1, s2)
        y, t1, t2 = _biquad(hp, u, t1, t2)
        if j >= H:
            p = np.minimum(y * y, np.float32(64.0))
            e += np.rint(p.astype(np.float64) * SCALE).astype(np.uint64)
    return e


def peak_and_bad(x):
    x = np.asarray(x, dtype=np.float32)
    ok = np.isfinite(x)
    return (np.float32(np.abs(x[ok]).max()) if ok.any() else np.float32(0.0)), int((~ok).sum())


def _split_sum(vals):
    hi = sum(v >> 32 for v in vals)
    lo = sum(v & 0xffffffff for v in vals)
    return float(hi) * 4294967296.0 + float(lo)


def gate(E, peak, n_bad, d):
    """Gating and gain of the contract.  ``E``: hop integers; ``peak``: float32; ``d``: ``fq3hip.loudness.design(...)``.  -> dict with the
    fields of ``fq3_loud_stats`` (``gain`` and ``peak`` as ``np.float32``)."""
    E = [int(v) for v in E]
    n = len(E)
    out = dict(mean_power=0.0, peak=np.float32(peak), gain=np.float32(1.0), n_hops=n, n_abs=0, n_rel=0, n_bad=int(n_bad), valid=0)
    B = [E[b] + E[b + 1] + E[b + 2] + E[b + 3] for b in range(n - 3)]
    g1 = [v for v in B if v > d.abs_gate]
    n1 = len(g1)
    out["n_abs"] = n1
    if n1 == 0:
        return out
    s1d = _split_sum(g1)
    g2 = [v for v in g1 if float(v) * float(10 * n1) > s1d]
    n2 = len(g2)
    out["n_rel"] = n2
    if n2 == 0:
        return out
    out["mean_power"] = _split_sum(g2) / (float(n2) * float(4 * d.H) * SCALE)
    if n_bad:
        return out
    g = math.sqrt(d.target_power / out["mean_power"])
    g = min(g, d.max_gain)
    if float(peak) > 0.0:
        g = min(g, d.ceiling / float(np.float32(peak)))
    out["gain"], out["valid"] = np.float32(g), 1
    return out


def lufs_of(mean_power):
    return -0.691 + 10.0 * math.log10(mean_power) if mean_power > 0 else float("-inf")


def burst_signal(rate, seed=0, level=0.25, hops=70, tail=137):
    """The GPU tests' signal: ``hops`` hops of rate / 10 samples plus ``tail`` samples.  Hop-aligned bursts of 140 + 280 + 2300 Hz with
    low noise inside them, exact-zero gaps of at least 5 hops between them, one burst 20 dB below the rest."""
    H = rate // 10
    rng = np.random.default_rng(seed)
    x = np.zeros(hops * H + tail, dtype=np.float64)
    t = np.arange(len(x)) / rate
    tone = (np.sin(2 * np.pi * 140 * t) + 0.7 * np.sin(2 * np.pi * 280 * t + 0.4) + 0.5 * np.sin(2 * np.pi * 2300 * t + 1.1)) / 2.2
    # (first hop, hops, relative level): 60 of 70 hops sound, gaps of 5 hops, the tail is silent.  Every burst fades in and out over
    # 20 ms inside its own hops: a burst cut off at full level leaves a high-pass transient in the gap behind it that puts the gap's
    # first block 8 dB ABOVE the absolute gate; with the fade it lies more than 20 dB below.
    nf = rate // 50
    fade = 0.5 - 0.5 * np.cos(np.pi * (np.arange(nf) + 0.5) / nf)
    for h0, n, rel in BURSTS:
        seg = slice(h0 * H, (h0 + n) * H)
        b = level * rel * (tone[seg] + 0.01 * rng.standard_normal(n * H))
        b[:nf] *= fade
        b[-nf:] *= fade[::-1]
        x[seg] = b
    return x.astype(np.float32)


BURSTS = ((0, 25, 1.0), (30, 12, 0.1), (47, 23, 1.0))


def block_levels64(x, rate):
    """the float64 measure's block powers (mean square of the K-weighted signal per 400 ms block, 100 ms apart)"""
    e = hop_energies64(x, rate)
    return (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * (rate // 10))
