"""CPU reference of the FLAC output stage: a numpy encoder that implements the emitted subset and its selection
rule literally, and a pure-Python decoder that checks everything a frame carries (marker, STREAMINFO, both CRCs, frame numbers,
reserved codes).  The device stage must reproduce the encoder's bytes exactly; the decoder is the independent half: it shares no code
with the encoder beyond the two CRC routines, which are pinned by their check values."""
from __future__ import annotations

import struct

import numpy as np

MAX_ORDER, MAX_PORDER, MAX_K = 4, 6, 14
BLOCK_TABLE = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_TABLE = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
EMITTED_RATES = {r: c for r, c in RATE_TABLE.items() if c not in (2, 3)}      # the stage's table (section 1 of the format)
FIXED_COEFFS = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def crc8(data: bytes) -> int:
    """polynomial 0x07, init 0, no reflection"""
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16_TABLE = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16_TABLE.append(_c)


def crc16(data: bytes) -> int:
    """polynomial 0x8005, init 0, no reflection"""
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16_TABLE[(c >> 8) ^ b]
    return c


def default_block(rate: int) -> int:
    return 1152 if rate > 16000 else 576


def stream_header(rate: int, block: int = 0, total: int = 0) -> bytes:
    """``fLaC`` + one STREAMINFO block (last, 34 bytes): 42 bytes"""
    block = block or default_block(rate)
    v = (rate << 44) | (0 << 41) | (15 << 36) | total          # 20 + 3 + 5 + 36 bits
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + struct.pack(">HH", block, block) + b"\0" * 6 + v.to_bytes(8, "big") + b"\0" * 16


def _utf8(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for n, lead in ((2, 0xC0), (3, 0xE0), (4, 0xF0), (5, 0xF8), (6, 0xFC)):
        if v < 1 << (5 * n + 1):
            return bytes([lead | (v >> (6 * (n - 1)))] + [0x80 | ((v >> (6 * j)) & 0x3F) for j in range(n - 2, -1, -1)])
    raise ValueError("frame number above 2^31")


def frame_header(rate: int, n: int, number: int) -> bytes:
    if n in BLOCK_TABLE:
        bcode, btail = BLOCK_TABLE[n], b""
    elif n <= 256:
        bcode, btail = 6, bytes([n - 1])
    else:
        bcode, btail = 7, struct.pack(">H", n - 1)
    if rate in EMITTED_RATES:
        rcode, rtail = EMITTED_RATES[rate], b""
    elif rate <= 65535:
        rcode, rtail = 13, struct.pack(">H", rate)
    else:
        raise ValueError(f"no frame-header code for {rate} Hz")
    h = bytes([0xFF, 0xF8, (bcode << 4) | rcode, 0x08]) + _utf8(number) + btail + rtail
    return h + bytes([crc8(h)])


def residuals(x: np.ndarray, order: int) -> np.ndarray:
    """r[i] for i >= order (int64 arithmetic; the values fit int32)"""
    x = x.astype(np.int64)
    r = x[order:].copy()
    for j, c in enumerate(FIXED_COEFFS[order]):
        r -= c * x[order - 1 - j: len(x) - 1 - j]
    return r


def _fold(r: np.ndarray) -> np.ndarray:
    return np.where(r >= 0, 2 * r, -2 * r - 1)                 # (r << 1) ^ (r >> 31)


def choose(x: np.ndarray):
    """The selection rule.  -> ("constant",) | ("verbatim",) | ("fixed", order, partition order, [k per partition])"""
    n = len(x)
    if np.all(x == x[0]):
        return ("constant",)
    best = None
    for o in range(min(MAX_ORDER, n - 1) + 1):
        u = _fold(residuals(x, o))
        for p in range(MAX_PORDER + 1):
            if n % (1 << p) or (n >> p) <= o:
                continue
            size, cost, ks = n >> p, 16 * o + 6, []
            for q in range(1 << p):
                part = u[max(q * size - o, 0): (q + 1) * size - o]
                bits = [len(part) * (1 + k) + int((part >> k).sum()) for k in range(MAX_K + 1)]
                k = int(np.argmin(bits))                       # the lowest k on ties
                ks.append(k)
                cost += 4 + bits[k]
            if best is None or cost < best[0]:                 # o ascending, then p ascending: ties keep the earlier
                best = (cost, o, p, ks)
    cost, o, p, ks = best
    return ("verbatim",) if cost >= 16 * n else ("fixed", o, p, ks)


def _bits_of(values: np.ndarray, width: int) -> np.ndarray:
    v = values.astype(np.int64) & ((1 << width) - 1)
    return ((v[:, None] >> np.arange(width - 1, -1, -1)) & 1).astype(np.uint8).reshape(-1)


def encode_frame(x: np.ndarray, rate: int, number: int, stats: list | None = None) -> bytes:
    x = np.asarray(x, dtype=np.int16)
    n, ch = len(x), choose(np.asarray(x, dtype=np.int16))
    if stats is not None:
        stats.append(ch)
    if ch[0] == "constant":
        bits = np.concatenate([_bits_of(np.array([0]), 8), _bits_of(x[:1], 16)])
    elif ch[0] == "verbatim":
        bits = np.concatenate([_bits_of(np.array([1 << 1]), 8), _bits_of(x, 16)])
    else:
        _, o, p, ks = ch
        u = _fold(residuals(x, o))
        size = n >> p
        parts = [_bits_of(np.array([(8 | o) << 1]), 8), _bits_of(x[:o], 16), _bits_of(np.array([0]), 2), _bits_of(np.array([p]), 4)]
        for q, k in enumerate(ks):
            part = u[max(q * size - o, 0): (q + 1) * size - o]
            quo = part >> k
            lens = quo + 1 + k
            ends = np.cumsum(lens)
            b = np.zeros(int(ends[-1]) if len(ends) else 0, dtype=np.uint8)
            stop = ends - k - 1
            b[stop] = 1
            for j in range(k):
                b[stop + 1 + j] = (part >> (k - 1 - j)) & 1
            parts += [_bits_of(np.array([k]), 4), b]
        bits = np.concatenate(parts)
    body = np.packbits(bits).tobytes()                         # zero bits up to the byte boundary
    f = frame_header(rate, n, number) + body
    return f + struct.pack(">H", crc16(f))


def encode_frames(x: np.ndarray, rate: int, block: int = 0, stats: list | None = None) -> bytes:
    """the frames alone (what the device stage writes)"""
    x = np.asarray(x, dtype=np.int16).reshape(-1)
    block = block or default_block(rate)
    return b"".join(encode_frame(x[i: i + block], rate, i // block, stats) for i in range(0, len(x), block))


def encode(x: np.ndarray, rate: int, block: int = 0, total: int | None = None, stats: list | None = None) -> bytes:
    x = np.asarray(x, dtype=np.int16).reshape(-1)
    return stream_header(rate, block, len(x) if total is None else total) + encode_frames(x, rate, block, stats)


# ---- decoder -------------------------------------------------------------------------------------------------------------------
class FlacError(ValueError):
    pass


class _Bits:
    def __init__(self, data: bytes, pos: int):
        self.d, self.p = data, pos * 8

    def read(self, n: int) -> int:
        if n == 0:
            return 0
        a, b = self.p >> 3, (self.p + n + 7) >> 3
        if b > len(self.d):
            raise FlacError("stream ends inside a frame")
        v = int.from_bytes(self.d[a:b], "big") >> (b * 8 - self.p - n)
        self.p += n
        return v & ((1 << n) - 1)

    def signed(self, n: int) -> int:
        v = self.read(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self) -> int:
        q = 0
        while True:
            room = min(32, len(self.d) * 8 - self.p)
            if room <= 0:
                raise FlacError("stream ends inside a Rice code")
            v = self.read(room)
            if v:
                lead = room - v.bit_length()
                self.p -= room - lead - 1
                return q + lead
            q += room

    def align(self) -> None:
        pad = -self.p % 8
        if pad and self.read(pad):
            raise FlacError("non-zero padding bits")

    @property
    def byte(self) -> int:
        assert self.p % 8 == 0
        return self.p >> 3


_BLOCK_BY_CODE = {c: b for b, c in BLOCK_TABLE.items()}
_RATE_BY_CODE = {c: r for r, c in RATE_TABLE.items()}


def decode(data: bytes):
    """-> (int16 samples, info).  ``info``: rate, block, total, frames (one dict per frame: n, kind, order, porder, ks, bytes).
    Raises ``FlacError`` on anything a conforming mono 16-bit fixed-blocksize stream may not contain."""
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    if len(data) < 42 or data[4] != 0x80 or data[5:8] != b"\0\0\x22":
        raise FlacError("the first and only metadata block must be a 34-byte STREAMINFO marked last")
    bmin, bmax = struct.unpack(">HH", data[8:12])
    v = int.from_bytes(data[18:26], "big")
    rate, ch, bps, total = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    if bmin != bmax or bmin < 16 or ch != 1 or bps != 16 or rate == 0:
        raise FlacError(f"STREAMINFO: blocks {bmin}..{bmax}, {ch} channels, {bps} bits, {rate} Hz")
    out, frames, pos = [], [], 42
    while pos < len(data):
        if frames and frames[-1]["n"] != bmin:
            raise FlacError("a short block that is not the last one")
        start = pos
        b = _Bits(data, pos)
        if b.read(15) != 0x7FFC:
            raise FlacError(f"no frame sync at byte {pos}")
        if b.read(1) != 0:
            raise FlacError("variable-blocksize frame in a fixed-blocksize stream")
        bcode, rcode = b.read(4), b.read(4)
        chan, ssize, reserved = b.read(4), b.read(3), b.read(1)
        if bcode == 0 or rcode == 15 or chan >= 11 or ssize in (3, 7) or reserved:
            raise FlacError(f"reserved code in the frame header at byte {pos}")
        if chan != 0 or ssize != 4:
            raise FlacError("not mono 16-bit")
        lead = b.read(8)
        if lead < 0x80:
            number = lead
        else:
            extra = 8 - (lead ^ 0xFF).bit_length() - 1
            if extra < 1 or extra > 5:
                raise FlacError("bad frame-number lead byte")
            number = lead & ((1 << (6 - extra)) - 1)
            for _ in range(extra):
                c = b.read(8)
                if c >> 6 != 2:
                    raise FlacError("bad frame-number continuation byte")
                number = (number << 6) | (c & 0x3F)
            if number < (0x80 if extra == 1 else 1 << (5 * extra + 1)):
                raise FlacError("over-long frame number")
        if number != len(frames):
            raise FlacError(f"frame number {number}, expected {len(frames)}")
        n = b.read(8) + 1 if bcode == 6 else b.read(16) + 1 if bcode == 7 else _BLOCK_BY_CODE[bcode]
        fr = (rate if rcode == 0 else b.read(8) * 1000 if rcode == 12 else b.read(16) if rcode == 13 else b.read(16) * 10 if rcode == 14
              else _RATE_BY_CODE[rcode])
        if fr != rate:
            raise FlacError(f"frame rate {fr}, STREAMINFO {rate}")
        if n > bmin:
            raise FlacError(f"block of {n} above the stream's {bmin}")
        if crc8(data[start: b.byte]) != b.read(8):
            raise FlacError(f"frame {number}: header CRC-8")
        if b.read(1):
            raise FlacError("subframe padding bit set")
        kind, wasted = b.read(6), b.read(1)
        if wasted:
            raise FlacError("wasted bits are not part of the subset")
        info = dict(n=n, kind=None, order=None, porder=None, ks=[])
        if kind == 0:
            x = [b.signed(16)] * n
            info["kind"] = "constant"
        elif kind == 1:
            x = [b.signed(16) for _ in range(n)]
            info["kind"] = "verbatim"
        elif 8 <= kind <= 12:
            o = kind - 8
            if o > n:
                raise FlacError("predictor order above the block size")
            x = [b.signed(16) for _ in range(o)]
            method = b.read(2)
            if method > 1:
                raise FlacError("reserved residual coding method")
            pbits, p = 4 + method, b.read(4)
            if n % (1 << p) or (n >> p) < o:
                raise FlacError("partition order does not fit the block")
            co = FIXED_COEFFS[o]
            for q in range(1 << p):
                k = b.read(pbits)
                cnt = (n >> p) - (o if q == 0 else 0)
                info["ks"].append(k)
                if k == (1 << pbits) - 1:
                    raw = b.read(5)
                    rs = [b.signed(raw) if raw else 0 for _ in range(cnt)]
                else:
                    rs = []
                    for _ in range(cnt):
                        u = (b.unary() << k) | b.read(k)
                        rs.append((u >> 1) ^ -(u & 1))
                for r in rs:
                    x.append(r + sum(c * x[-1 - j] for j, c in enumerate(co)))
            info.update(kind="fixed", order=o, porder=p)
        elif kind >= 32:
            raise FlacError("LPC subframes are not part of the subset")
        else:
            raise FlacError(f"reserved subframe type {kind:06b}")
        b.align()
        if crc16(data[start: b.byte]) != b.read(16):
            raise FlacError(f"frame {number}: CRC-16")
        if any(not -32768 <= s <= 32767 for s in x):
            raise FlacError("a decoded sample leaves 16 bits")
        pos = b.byte
        info["bytes"] = pos - start
        frames.append(info)
        out.extend(x)
    if total and total != len(out):
        raise FlacError(f"STREAMINFO says {total} samples, the frames hold {len(out)}")
    return np.asarray(out, dtype=np.int16), dict(rate=rate, block=bmin, total=total, frames=frames)


# ---- the signal set ------------------------------------------------------------------------------------------------------------
def signal_set(block: int = 1152, seed: int = 0) -> np.ndarray:
    """One block of each piece, in a fixed order; ``len`` is a multiple of ``block``."""
    g = np.random.default_rng(seed)
    B = block
    t = np.arange(B, dtype=np.float64)
    sweep = np.sin(2 * np.pi * (0.002 * t + 0.00004 * t * t)) * np.hanning(B)
    slow = np.sin(2 * np.pi * t / B)
    half = np.concatenate([g.integers(-20000, 20000, B // 2), g.integers(-2, 3, B - B // 2)])
    alt = np.where(np.arange(B) % 2 == 0, 32767, -32767)
    pieces = [
        np.zeros(B),                                   # digital silence
        np.full(B, -1234),                             # a DC run
        g.integers(-32768, 32768, B),                  # full-scale uniform noise
        g.integers(-3, 4, B),                          # noise of +-3
        np.round(sweep * 30000),                       # an enveloped sine sweep, loud
        np.round(sweep * 900),                         # the same sweep, quiet
        np.round(slow * 20000),                        # one slow period: a high fixed order wins
        np.round(slow * 20000) + g.integers(-1, 2, B),
        half,                                          # loud, then quiet half-way
        alt,                                           # +-32767 alternation
        np.cumsum(g.integers(-40, 41, B)),             # a random walk: order 1
        np.concatenate([np.full(B // 2, 7), np.full(B - B // 2, 7) + (np.arange(B - B // 2) % 2)]),   # k = 0 territory
    ]
    return np.concatenate([np.clip(p, -32768, 32767) for p in pieces]).astype(np.int16)
