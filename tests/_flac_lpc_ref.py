"""CPU reference of the FLAC stage with LPC subframes (``lpc_order`` = M in 1..8; the rule in include/fq3hip.h): a
numpy encoder that follows the rule literally -- integer window, exact autocorrelation, Levinson-Durbin in numpy float64 scalars (every
operation rounded on its own), 12-bit quantisation, exact costs -- and a decoder that also reads LPC subframes and checks both CRCs.
Headers, CRCs, fold and bit packing are tests/_flac_ref.py's; a frame whose choice is not LPC is that module's frame."""
from __future__ import annotations

import struct

import numpy as np

import _flac_ref as R

MAX_LPC, PRECISION, MIN_BLOCK = 8, 12, 64


def windowed(x: np.ndarray) -> np.ndarray:
    n = len(x)
    t, i = n // 4, np.arange(n, dtype=np.int64)
    d = np.where(i < t, t - i, np.where(i >= n - t, i - (n - 1 - t), 0))
    return (x.astype(np.int64) * (32768 - (32768 * d * d) // ((t + 1) * (t + 1))) + 2048) >> 12


def predictors(x: np.ndarray, M: int) -> dict:
    """{order: (q[0 .. order), s)} of the orders that are candidates"""
    n, out = len(x), {}
    if n < MIN_BLOCK:
        return out
    y = windowed(x)
    r = [np.float64(int(np.dot(y[: n - l], y[l:]))) for l in range(M + 1)]
    a, err = [], r[0]
    with np.errstate(all="ignore"):
        for i in range(M):
            if not (np.isfinite(err) and err > 0):
                break
            acc = r[i + 1]
            for j in range(i):
                acc = acc - a[j] * r[i - j]
            k = acc / err
            a = [a[j] - k * a[i - 1 - j] for j in range(i)] + [k]
            err = err * (np.float64(1) - k * k)
            cmax = max(abs(c) for c in a)
            if not all(np.isfinite(c) for c in a) or cmax == 0:
                continue
            s = min(15, 11 - int(np.frexp(cmax)[1]))
            if s >= 0:
                out[i + 1] = ([int(min(max(np.rint(np.ldexp(c, s)), -2048), 2047)) for c in a], s)
    return out


def lpc_residuals(x: np.ndarray, q, s: int) -> np.ndarray:
    o, x = len(q), x.astype(np.int64)
    return x[o:] - (sum(c * x[o - 1 - j: len(x) - 1 - j] for j, c in enumerate(q)) >> s)


def choose(x: np.ndarray, M: int):
    """-> _flac_ref.choose's tuples, or ("lpc", order, partition order, [k per partition], q, s)"""
    n = len(x)
    if np.all(x == x[0]):
        return ("constant",)
    cands = [("fixed", o, R.residuals(x, o), ()) for o in range(min(R.MAX_ORDER, n - 1) + 1)]
    cands += [("lpc", o, lpc_residuals(x, q, s), (q, s)) for o, (q, s) in sorted(predictors(x, M).items())]
    best = None
    ks15 = np.arange(R.MAX_K + 1)[:, None]
    for kind, o, res, extra in cands:                          # FIXED first, orders ascending, then p ascending: ties keep the earlier
        sums = np.concatenate([np.zeros((R.MAX_K + 1, 1), np.int64), np.cumsum(R._fold(res)[None, :] >> ks15, axis=1)], axis=1)
        for p in range(R.MAX_PORDER + 1):
            if n % (1 << p) or (n >> p) <= o:
                continue
            edges = np.maximum(np.arange((1 << p) + 1) * (n >> p) - o, 0)
            bits = np.diff(edges)[None, :] * (1 + ks15) + sums[:, edges[1:]] - sums[:, edges[:-1]]
            ks = np.argmin(bits, axis=0)                       # the lowest k on ties
            cost = 16 * o + 6 + (9 + PRECISION * o if kind == "lpc" else 0) + int((4 + bits.min(axis=0)).sum())
            if best is None or cost < best[0]:
                best = (cost, (kind, o, p, [int(k) for k in ks]) + extra)
    return ("verbatim",) if best[0] >= 16 * n else best[1]


def encode_frame(x: np.ndarray, rate: int, number: int, M: int, stats: list | None = None) -> bytes:
    x = np.asarray(x, dtype=np.int16)
    ch = choose(x, M) if M > 0 else ("fixed-only",)
    if ch[0] != "lpc":                                         # the fixed-only encoder makes the same choice among the same candidates
        return R.encode_frame(x, rate, number, stats)
    if stats is not None:
        stats.append(ch)
    _, o, p, ks, q, s = ch
    u, size, bits = R._fold(lpc_residuals(x, q, s)), len(x) >> p, R._bits_of
    parts = [bits(np.array([(0x20 | (o - 1)) << 1]), 8), bits(x[:o], 16), bits(np.array([PRECISION - 1]), 4), bits(np.array([s]), 5),
             bits(np.array(q), PRECISION), bits(np.array([p]), 6)]
    for part, k in zip((u[max(i * size - o, 0): (i + 1) * size - o] for i in range(1 << p)), ks):
        parts.append(bits(np.array([k]), 4))
        for v in part:                                         # unary quotient, stop bit, k low bits
            parts += [np.zeros(int(v >> k), np.uint8), bits(np.array([(1 << k) | (int(v) & ((1 << k) - 1))]), k + 1)]
    f = R.frame_header(rate, len(x), number) + np.packbits(np.concatenate(parts)).tobytes()
    return f + struct.pack(">H", R.crc16(f))


def encode_frames(x: np.ndarray, rate: int, block: int = 0, M: int = MAX_LPC, stats: list | None = None) -> bytes:
    x = np.asarray(x, dtype=np.int16).reshape(-1)
    block = block or R.default_block(rate)
    return b"".join(encode_frame(x[i: i + block], rate, i // block, M, stats) for i in range(0, len(x), block))


def decode(data: bytes) -> np.ndarray:
    """the samples of a stream of this stage (header and frames), LPC subframes included; ``R.FlacError`` on a bad CRC or a frame
    this stage does not write (``_flac_ref.decode`` is the strict reader of everything but the LPC subframe)"""
    data = bytes(data)
    if data[:8] != b"fLaC\x80\x00\x00\x22" or len(data) < 42:
        raise R.FlacError("no fLaC marker and STREAMINFO")
    out, pos, number = [], 42, 0
    while pos < len(data):
        b = R._Bits(data, pos)
        if b.read(16) != 0xFFF8:
            raise R.FlacError(f"no frame sync at byte {pos}")
        bcode, rcode, rest = b.read(4), b.read(4), b.read(8)
        lead = b.read(8)
        extra = 0 if lead < 0x80 else 8 - (lead ^ 0xFF).bit_length() - 1
        got = lead if lead < 0x80 else lead & ((1 << (6 - extra)) - 1)
        for _ in range(extra):
            got = (got << 6) | (b.read(8) & 0x3F)
        n = b.read(8) + 1 if bcode == 6 else b.read(16) + 1 if bcode == 7 else R._BLOCK_BY_CODE[bcode]
        if rcode == 13:
            b.read(16)
        if rest != 0x08 or got != number or R.crc8(data[pos: b.byte]) != b.read(8):
            raise R.FlacError(f"frame {number}: header")
        kind = b.read(8) >> 1
        o = 0 if kind < 2 else kind - 8 if kind < 32 else kind - 31
        x = [b.signed(16) for _ in range(n if kind == 1 else 1 if kind == 0 else o)]
        if kind == 0:
            x = x * n
        elif kind != 1:
            q, s = list(R.FIXED_COEFFS[o]) if kind < 32 else None, 0
            if q is None:
                if b.read(4) != PRECISION - 1:
                    raise R.FlacError("coefficient precision")
                s = b.read(5)
                q = [b.signed(PRECISION) for _ in range(o)]
            if b.read(2):
                raise R.FlacError("residual coding method")
            p = b.read(4)
            for part in range(1 << p):
                k = b.read(4)
                for _ in range((n >> p) - (o if part == 0 else 0)):
                    u = (b.unary() << k) | b.read(k)
                    x.append(((u >> 1) ^ -(u & 1)) + (sum(c * x[-1 - j] for j, c in enumerate(q)) >> s))
        b.align()
        if R.crc16(data[pos: b.byte]) != b.read(16):
            raise R.FlacError(f"frame {number}: CRC-16")
        out, pos, number = out + x, b.byte, number + 1
    return np.asarray(out, dtype=np.int16)


def signals(n: int, seed: int = 0) -> dict:
    """n samples of each piece: an AR(2) resonance under noise, two sines, a constant, full-scale noise, a full-scale alternation, +-1"""
    g = np.random.default_rng(seed)
    e, ar = g.standard_normal(n + 2) * 300.0, np.zeros(n + 2)
    for i in range(2, n + 2):
        ar[i] = 1.8 * ar[i - 1] - 0.97 * ar[i - 2] + e[i]
    t = np.arange(n)
    pieces = dict(ar2=ar[2:] * (12000.0 / np.abs(ar).max()), sines=9000 * np.sin(t / 7.3) + 6000 * np.sin(t / 2.1 + 1.0),
                  constant=np.full(n, -1234), noise=g.integers(-32768, 32768, n), alternation=np.where(t % 2 == 0, 32767, -32768),
                  quiet=g.integers(-1, 2, n))
    return {k: np.round(v).astype(np.int16) for k, v in pieces.items()}
