"""CPU reference of the leveller (include/fq3hip.h, "Leveller") in numpy float32 and Python ints and floats.

The hop integers, the peak and the gating are the loudness reference's (``_loud_ref.emulate_hops`` / ``peak_and_bad`` / ``gate``); this
module adds what the leveller adds: the target per prefix, the smoothing, the ramp and the multiply.

``level``        a whole stream at once -> the output and everything in between
``RefLeveller``  the same rule fed push by push (keeps the one hop of history the hop filter needs): what cut independence is
                 checked with on the CPU
``level64``      the rule in float64 on the float64 measure (``_loud_ref.hop_energies64``): what the convergence figures in the issue
                 were taken with

The gain constants and the absolute gate come from the library's design call (``fq3hip.loudness.design``), as in ``_loud_ref``."""
import math

import numpy as np

from _loud_ref import ABS_GATE_POWER, _fmaf, emulate_hops, gate, hop_energies64, peak_and_bad


def design_of(rate, spec):
    from fq3hip.loudness import design
    return design(rate, spec.loudness)


def hop_measures(x, d):
    """(E uint64, peak float32, bad int) per whole hop"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x) // d.H
    pb = [peak_and_bad(x[h * d.H:(h + 1) * d.H]) for h in range(n)]
    return emulate_hops(x, d.coef32, d.H), np.array([p for p, _ in pb], dtype=np.float32), np.array([b for _, b in pb], dtype=np.int64)


def target(E, peaks, bads, h, d, spec):
    """T(h) and the measure of the prefix E[0 .. h) -> (np.float32, gate dict with ``valid`` = T is the measured gain)"""
    g0 = spec.g0
    if h < 0:
        return g0, None
    pk = np.float32(peaks[:h].max()) if h > 0 else np.float32(0.0)
    r = gate(E[:h], pk, int(bads[:h].sum()), d)
    ok = bool(r["valid"]) and r["n_abs"] >= spec.min_blocks
    r["valid"] = int(ok)
    return (np.float32(r["gain"]) if ok else g0), r


def smooth(T, h, k, g0):
    """S(h): ``T`` holds T(0 .. len - 1)"""
    acc = 0.0
    for i in range(h - k + 1, h + 1):
        acc += float(g0 if i < 0 else T[i])
    return np.float32(acc / float(k))


def ramp(x, n0, S_at, H):
    """y for the samples ``x`` at stream positions n0 ..; ``S_at(h)`` for h >= -1"""
    x = np.asarray(x, dtype=np.float32)
    n = n0 + np.arange(len(x), dtype=np.int64)
    h = n // H
    j = (n - h * H).astype(np.float32)
    if not len(x):
        return x, x
    hs = np.arange(int(h.min()) - 1, int(h.max()) + 1)         # S of hops h.min() - 1 .. h.max()
    S = np.array([S_at(int(v)) for v in hs], dtype=np.float32)
    prev, cur = S[h - 1 - hs[0]], S[h - hs[0]]
    g = _fmaf(cur - prev, j / np.float32(H), prev)
    return x * g, g


def level(x, rate, spec):
    """-> dict: ``y`` and ``g`` per sample, ``energy`` / ``peak`` / ``bad`` per whole hop, ``T`` = T(0 .. n_hops), ``S`` = S(-1 .. n_hops)
    (index h + 1), ``stats`` = the fields of ``fq3_level_report`` for hop n_hops"""
    d = design_of(rate, spec)
    x = np.asarray(x, dtype=np.float32)
    E, pk, bad = hop_measures(x, d)
    n = len(E)
    T, last = [], None
    for h in range(n + 1):
        t, last = target(E, pk, bad, h, d, spec)
        T.append(t)
    T = np.array(T, dtype=np.float32)
    S = np.array([smooth(T, h, spec.smooth_hops, spec.g0) for h in range(-1, n + 1)], dtype=np.float32)
    y, g = ramp(x, 0, lambda h: S[h + 1], d.H)
    stats = dict(mean_power=last["mean_power"], target_gain=T[n], smooth_gain=S[n + 1], n_hops=n, n_abs=last["n_abs"], n_rel=last["n_rel"],
                 n_bad=last["n_bad"], valid=last["valid"])
    return dict(y=y, g=g, energy=E, peak=pk, bad=bad, T=T, S=S, stats=stats, design=d)


class RefLeveller:
    """The rule fed push by push."""

    def __init__(self, rate, spec):
        self.spec, self.d = spec, design_of(rate, spec)
        self.hist = np.zeros(0, dtype=np.float32)          # from the start of the hop in front of the first incomplete one
        self.total = 0
        self.E, self.pk, self.bad, self.T = [], [], [], []

    def push(self, x):
        x = np.asarray(x, dtype=np.float32)
        d, H = self.d, self.d.H
        h0, n0 = self.total // H, self.total
        v0 = max(h0 - 1, 0) * H                             # stream position of hist[0]
        v = np.concatenate([self.hist, x])
        self.total += len(x)
        h1 = self.total // H
        if h1 > h0:
            first = v0 // H
            e = emulate_hops(v[:(h1 - first) * H], d.coef32, H)
            for h in range(h0, h1):
                seg = v[(h - first) * H:(h - first + 1) * H]
                p, b = peak_and_bad(seg)
                self.E.append(int(e[h - first])), self.pk.append(p), self.bad.append(b)
        E, pk, bad = np.array(self.E, dtype=np.uint64), np.array(self.pk, dtype=np.float32), np.array(self.bad, dtype=np.int64)
        while len(self.T) <= h1 and len(x):
            self.T.append(target(E, pk, bad, len(self.T), d, self.spec)[0])
        self.hist = v[max(h1 - 1, 0) * H - v0:]
        if not len(x):
            return x
        return ramp(x, n0, lambda h: smooth(self.T, h, self.spec.smooth_hops, self.spec.g0), H)[0]


HOPS, TAIL = 30, 37
BURSTS = ((1, 11, 1.0), (15, 4, 0.1), (20, 9, 1.0))          # (first hop, hops, relative level): gaps of exact zeros between them


def burst_signal(rate, seed=0, level=0.25, hops=HOPS, tail=TAIL):
    """The tests' stream: ``hops`` hops plus ``tail`` samples; hop-aligned bursts of 140 + 280 + 2300 Hz with low noise, each faded in
    and out over 20 ms inside its own hops (as ``_loud_ref.burst_signal``, laid out for 30 hops), one burst 20 dB below the rest;
    the tail behind the last whole hop carries sound."""
    H = rate // 10
    rng = np.random.default_rng(seed)
    x = np.zeros(hops * H + tail, dtype=np.float64)
    t = np.arange(len(x)) / rate
    tone = (np.sin(2 * np.pi * 140 * t) + 0.7 * np.sin(2 * np.pi * 280 * t + 0.4) + 0.5 * np.sin(2 * np.pi * 2300 * t + 1.1)) / 2.2
    nf = rate // 50
    fade = 0.5 - 0.5 * np.cos(np.pi * (np.arange(nf) + 0.5) / nf)
    for h0, n, rel in BURSTS:
        seg = slice(h0 * H, (h0 + n) * H)
        b = level * rel * (tone[seg] + 0.01 * rng.standard_normal(n * H))
        b[:nf] *= fade
        b[-nf:] *= fade[::-1]
        x[seg] = b
    x[hops * H:] = 0.1 * level * tone[hops * H:]
    return x.astype(np.float32)


def signals(rate):
    """name -> stream, the cases of the GPU test: bursts, a signal below the absolute gate, one NaN, 10 hops of leading zeros"""
    H = rate // 10
    b = burst_signal(rate)
    nan = b.copy()
    nan[12 * H + 5] = np.nan
    lead = np.concatenate([np.zeros(10 * H, dtype=np.float32), burst_signal(rate, seed=1)[:(HOPS - 10) * H + TAIL]])
    return {"bursts": b, "quiet": (b * np.float32(1e-4)).astype(np.float32), "nan": nan, "lead": lead}


def level64(x, rate, spec):
    """The rule in float64 on the float64 measure (true recursive filter, float gating) -> (y, T): for figures, not for bit checks"""
    d = design_of(rate, spec)
    H, k, m = d.H, spec.smooth_hops, spec.min_blocks
    x = np.asarray(x, dtype=np.float64)
    e = hop_energies64(x, rate)
    n = len(e)
    g0 = 10.0 ** (spec.initial_gain_db / 20.0)
    ax = np.abs(x)
    T = []
    for h in range(n + 1):
        t = g0
        if h >= 4:
            z = (e[:h - 3] + e[1:h - 2] + e[2:h - 1] + e[3:h]) / (4.0 * H)
            g1 = z[z > ABS_GATE_POWER]
            if len(g1) >= m:
                g2 = g1[g1 > 0.1 * g1.mean()]
                t = min(math.sqrt(d.target_power / g2.mean()), d.max_gain)
                pk = ax[:h * H].max()
                if pk > 0:
                    t = min(t, d.ceiling / pk)
        T.append(t)
    S = [np.mean([g0 if i < 0 else T[i] for i in range(h - k + 1, h + 1)]) for h in range(-1, n + 1)]
    S = np.array(S)
    pos = np.arange(len(x))
    h = pos // H
    j = (pos - h * H) / H
    return x * (S[h] + (S[h + 1] - S[h]) * j), np.array(T)
