"""CPU reference of the limiter stage (include/fq3hip.h, "Limiter").  Two models:

``emulate``      (a) the contract in float32, operation by operation: the detector rows as separately rounded numpy float32 multiplies
                 and adds over ascending taps, the correctly rounded float32 division, then integers.  Its constants (``c``, the rows,
                 ``A``, ``H``) come from the library's design call (``fq3hip.limiter.design``): it never recomputes ``pow`` or the window.
``true_peak64``  (b) a float64 yardstick: 32x windowed-sinc oversampling (48 taps each side, Kaiser beta 10) of any waveform, to read
                 its true peak.

and the test signals both test files share, with the two measured figures the GPU test's true-peak bound is derived from."""
import functools
from types import SimpleNamespace

import numpy as np

ONE = 1 << 23
RATES = (24000, 8000, 44100)
CEILINGS = (-1.0, -6.0)
MARGIN = 1.05                      # on (overshoot - 1): covers the yardstick's own truncation, nothing else


def emulate(x, d):
    """The whole stream at once -> a namespace with ``y`` (float32, ``len(x)``), ``p`` (float32), ``q`` / ``g`` (int64; ``g[i]`` is the
    gain applied to sample i, i.e. the contract's g[i + A]) and the stats ``true_peak`` (float32), ``min_gain_q23``, ``n_limited``,
    ``n_bad``."""
    x = np.asarray(x, dtype=np.float32)
    n, A, H, c = len(x), int(d.A), int(d.H), np.float32(d.c)
    bad = ~np.isfinite(x)
    xc = np.where(bad, np.float32(0), x).astype(np.float32)
    if n == 0:
        return SimpleNamespace(y=xc, p=xc, q=np.zeros(0, np.int64), g=np.zeros(0, np.int64), true_peak=np.float32(0), min_gain_q23=ONE,
                               n_limited=0, n_bad=0)
    xp = np.concatenate([np.zeros(5, np.float32), xc, np.zeros(6, np.float32)])
    p = np.abs(xc)
    with np.errstate(over="ignore"):
        for row in d.rows:
            u = np.zeros(n, np.float32)
            for t in range(12):
                prod = np.float32(row[t]) * xp[t:t + n]               # one rounding
                u = u + prod                                          # one rounding
            assert u.dtype == np.float32 and prod.dtype == np.float32
            p = np.maximum(p, np.abs(u))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (c / p).astype(np.float32)                            # correctly rounded float32 division
        q = np.where(p <= c, ONE, np.floor(ratio * np.float32(8388608.0))).astype(np.int64)
    # m[k] for stream index k in [0, n + A): the minimum over q[k - A - H .. k], q = 2^23 outside the stream
    qp = np.concatenate([np.full(A + H, ONE, np.int64), q, np.full(A, ONE, np.int64)])
    m = np.lib.stride_tricks.sliding_window_view(qp, A + H + 1).min(axis=1)
    assert len(m) == n + A
    cs = np.concatenate([[0], np.cumsum(m)])
    s = cs[A + 1:] - cs[:n]                                           # s[i + A] = m[i] + ... + m[i + A]
    g = s // (A + 1)
    y = xc * (g.astype(np.float32) * np.float32(2.0 ** -23))
    assert y.dtype == np.float32 and len(y) == n
    return SimpleNamespace(y=y, p=p, q=q, g=g, true_peak=np.float32(p.max()), min_gain_q23=int(g.min()), n_limited=int((g < ONE).sum()),
                           n_bad=int(bad.sum()))


def stats_tuple(e):
    return (np.float32(e.true_peak).tobytes(), int(e.min_gain_q23), int(e.n_limited), int(e.n_bad))


# ---- (b) the float64 yardstick ---------------------------------------------------------------------------------------------------------
_OS, _HALF, _BETA = 32, 48, 10.0


@functools.lru_cache(maxsize=None)
def _phases():
    t = np.arange(-_HALF + 1, _HALF + 1, dtype=np.float64)            # taps on x[n - 47 .. n + 48]
    rows = []
    for k in range(1, _OS):
        dd = t - k / _OS
        w = np.i0(_BETA * np.sqrt(np.maximum(0.0, 1.0 - (dd / _HALF) ** 2))) / np.i0(_BETA)
        h = np.sinc(dd) * w
        rows.append(h / h.sum())
    return t.astype(int), rows


def true_peak64(x):
    """max |x(t)| over the 32x oversampled waveform (x = 0 outside; non-finite samples read as 0)"""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(np.isfinite(x), x, 0.0)
    if len(x) == 0:
        return 0.0
    peak = float(np.abs(x).max())
    t, rows = _phases()
    xp = np.concatenate([np.zeros(_HALF, np.float64), x, np.zeros(_HALF, np.float64)])
    n = len(x) + 1                                                    # points n + k / 32 for n = -1 .. len(x) - 1
    for h in rows:
        acc = np.zeros(n)
        for off, coef in zip(t, h):
            acc += coef * xp[_HALF - 1 + off:_HALF - 1 + off + n]
        peak = max(peak, float(np.abs(acc).max()))
    return peak


# ---- the signals -----------------------------------------------------------------------------------------------------------------------
def _frozen(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def signals(rate, d):
    """0.5 s each, read-only.  ``bursts``: noise bursts at +12 dB over the ceiling (peak), separated by quiet stretches shorter and
    longer than A + H, with runs of exact zeros among them; ``sine``: in_rate / 4 at 45 degrees, amplitude 1.2 -- samples +-0.849,
    true peak 1.2; ``bad``: the bursts with a NaN and an Inf in them; ``quiet``: entirely below the ceiling, true peak included."""
    n, A, H, c = rate // 2, int(d.A), int(d.H), float(d.c)
    rng = np.random.default_rng(rate)
    x = (rng.standard_normal(n) * 0.02).astype(np.float32)
    pos, gaps, k = A + 3, [(A + H) // 3, 2 * (A + H), (A + H) - 1, (A + H) + 1, 5, 3 * (A + H)], 0
    while pos < n - 8:
        ln = min(int(rng.integers(A // 2, 3 * A)), n - pos)
        b = rng.uniform(-1.0, 1.0, ln)
        x[pos:pos + ln] = (b / np.abs(b).max() * c * 10.0 ** (12.0 / 20.0)).astype(np.float32)
        pos += ln
        gap = gaps[k % len(gaps)]
        if k % 2:
            x[pos:pos + gap] = 0.0                                    # a run of exact zeros
        pos += gap
        k += 1
    i = np.arange(n)
    sine = 1.2 * np.sin(np.pi / 2 * i + np.pi / 4)
    bad = x.copy()
    bad[n // 3] = np.nan
    bad[n // 3 + A + 2] = np.inf
    bad[5] = -np.inf
    quiet = (rng.uniform(-1.0, 1.0, n) * 0.2 * c).astype(np.float32)
    quiet[n // 4:n // 4 + 300] = 0.0
    return {"bursts": _frozen(x), "sine": _frozen(sine), "bad": _frozen(bad), "quiet": _frozen(quiet)}


@functools.lru_cache(maxsize=None)
def case(rate, ceiling_db):
    """(design, signals, emulations) of one rate and ceiling at the default 5 ms / 20 ms, computed once and shared"""
    from fq3hip import limiter as M
    d = M.design(rate, M.LimiterSpec(ceiling_db=ceiling_db))
    sig = signals(rate, d)
    return d, sig, {k: emulate(v, d) for k, v in sig.items()}


@functools.lru_cache(maxsize=None)
def measured(rate, ceiling_db):
    """The two measurements behind the GPU test's true-peak bound, per signal: ``under_read`` = true peak of the INPUT by (b) over the
    detector's largest p (above 1: the 4x detector reads low), ``overshoot`` = true peak of the reference OUTPUT by (b) over c."""
    d, sig, emu = case(rate, ceiling_db)
    out = {}
    for k in ("bursts", "sine", "bad"):
        out[k] = dict(under_read=true_peak64(sig[k]) / float(emu[k].true_peak), overshoot=true_peak64(emu[k].y) / float(d.c))
    return out


def true_peak_bound(rate, ceiling_db):
    """c * (1 + MARGIN * (worst overshoot - 1)): the device equals (a) bit for bit, so the margin only covers the yardstick"""
    d = case(rate, ceiling_db)[0]
    worst = max(max(v["overshoot"] for v in measured(rate, ceiling_db).values()), 1.0)
    return float(d.c) * (1.0 + MARGIN * (worst - 1.0))
