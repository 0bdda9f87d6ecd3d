"""A true-peak look-ahead limiter on the device (``fq3_limit_*``): float32 mono in, float32 out at the same
rate, length-preserving, with a fixed latency of ``A + 6`` samples.  No output sample exceeds the ceiling by more than one part in
2^22, whatever the stream does later; the result does not depend on how the stream was cut into pushes, bit for bit.

``LimiterSpec``  what a caller asks for (ceiling, look-ahead, hold); host only, validates without a GPU
``design``       the numbers the device works with (``fq3_limit_design``; no GPU needed)
``count``        output samples that exist after ``n_in`` input samples (``fq3_limit_count``; no GPU needed)
``Limiter``      one stream on a device: ``push`` / ``push_host`` / ``reset`` / ``stats``"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

CEILING_RANGE, LOOKAHEAD_RANGE, HOLD_RANGE = (-20.0, 0.0), (0.0, 60.0), (0.0, 240.0)
STATS_BYTES = C.sizeof(_lib.LimitStats)
ONE_Q23 = 1 << 23


def _number(v, what: str, lo: float, hi: float) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a number in [{lo:g}, {hi:g}], not {v!r}")
    if not lo <= float(v) <= hi:
        raise ValueError(f"{what} {v!r} is outside [{lo:g}, {hi:g}]")
    return float(v)


@dataclass(frozen=True)
class LimiterSpec:
    """``ceiling_db`` in [-20, 0]: the level (dBFS) no output sample exceeds.  ``lookahead_ms``: the attack -- the gain starts to fall
    that long before a peak, and the stage delays the stream by it (plus 6 samples); at the stream's rate it must come to 8 .. 480
    samples.  ``hold_ms``: how long the gain stays down behind a peak before it ramps back over one more attack time; 0 .. 1920
    samples.  The defaults (-1 dBFS, 5 ms, 20 ms) are common figures; they have NOT been tuned on real voices."""
    ceiling_db: float = -1.0
    lookahead_ms: float = 5.0
    hold_ms: float = 20.0

    def __post_init__(self):
        _number(self.ceiling_db, "ceiling_db", *CEILING_RANGE)
        _number(self.lookahead_ms, "lookahead_ms", *LOOKAHEAD_RANGE)
        _number(self.hold_ms, "hold_ms", *HOLD_RANGE)


@dataclass(frozen=True)
class LimiterDesign:
    """What ``fq3_limit_design`` hands back: attack ``A`` and hold ``H`` in samples, the ceiling ``c`` as the device's float32, the
    detector's three fractional-phase rows (12 float32 taps each, tap t on ``x[n - 5 + t]``) and the push kernel's default tile."""
    A: int
    H: int
    c: np.float32
    rows: Tuple[Tuple[np.float32, ...], ...]
    tile: int

    @property
    def latency(self) -> int:
        return self.A + 6

    @property
    def history(self) -> int:
        return 2 * self.A + self.H + 11


def design(in_rate: int, spec: Optional[LimiterSpec] = None) -> LimiterDesign:
    """``fq3_limit_design`` (host only, no GPU needed); ``ValueError`` with the library's reason for what it refuses."""
    spec = LimiterSpec() if spec is None else spec
    lib = _lib.load()
    A, H, tile, c = C.c_int(), C.c_int(), C.c_int(), C.c_float()
    rows = (C.c_float * 36)()
    rc = lib.fq3_limit_design(int(in_rate), float(spec.ceiling_db), float(spec.lookahead_ms), float(spec.hold_ms), C.byref(A), C.byref(H),
                              C.byref(c), rows, C.byref(tile))
    if rc != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    r = tuple(tuple(np.float32(rows[f * 12 + t]) for t in range(12)) for f in range(3))
    return LimiterDesign(A.value, H.value, np.float32(c.value), r, tile.value)


def count(in_rate: int, spec: Optional[LimiterSpec], n_in: int, final: bool) -> int:
    """``fq3_limit_count``: ``n_in`` when ``final``, else ``max(0, n_in - A - 6)``."""
    spec = LimiterSpec() if spec is None else spec
    lib = _lib.load()
    n = lib.fq3_limit_count(int(in_rate), float(spec.lookahead_ms), int(n_in), 1 if final else 0)
    if n < 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return int(n)


@dataclass(frozen=True)
class LimiterStats:
    """``true_peak``: the largest detector value of the stream so far (the 4x oversampled estimate), ``true_peak_db`` in dBFS;
    ``min_gain``: the smallest gain applied (``min_gain_q23 / 2^23``); ``n_limited``: output samples whose gain was below 1;
    ``n_bad``: non-finite input samples (emitted as 0)."""
    true_peak: float
    true_peak_db: float
    min_gain: float
    min_gain_db: float
    min_gain_q23: int
    n_limited: int
    n_bad: int

    @classmethod
    def from_bytes(cls, raw: bytes) -> "LimiterStats":
        s = _lib.LimitStats.from_buffer_copy(raw)
        g = s.min_gain_q23 / ONE_Q23

        def db(v):
            return 20.0 * math.log10(v) if v > 0 else float("-inf")
        return cls(float(s.true_peak), db(s.true_peak), g, db(g), int(s.min_gain_q23), int(s.n_limited), int(s.n_bad))


class Limiter:
    """One stream through the limiter.  ``push(pcm)`` takes the next float32 samples (a device tensor) and returns the samples that
    became final -- ``count(total so far) - count(before)`` of them, a device tensor, one launch, nothing synchronises;
    ``push(..., final=True)`` ends the stream and hands out the held-back ``A + 6`` samples (``pcm`` may be None or empty).
    ``push_host`` is the same for a numpy array and returns one.  ``reset()`` starts a new stream on the same object, ``stats()``
    reads the accumulators.  Work is enqueued on ``stream`` (default: the current stream at the time of the call).  ``tile``: output
    samples per workgroup (0: the default); it changes the speed, never the result."""

    def __init__(self, spec: Optional[LimiterSpec], in_rate: int, device, stream=None, tile: int = 0):
        self.spec = LimiterSpec() if spec is None else spec
        if not isinstance(self.spec, LimiterSpec):
            raise ValueError(f"spec must be a LimiterSpec or None, not {type(spec).__name__}")
        self.in_rate = int(in_rate)
        self.design = design(self.in_rate, self.spec)
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        if self.dev.type != "cuda":
            raise ValueError("Limiter runs on the GPU; there is no CPU fallback")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.stream = stream
        self._lib = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.LimitConfig(self.in_rate, float(self.spec.ceiling_db), float(self.spec.lookahead_ms), float(self.spec.hold_ms), int(tile))
        with torch.cuda.device(self.dev):
            rc = self._lib.fq3_limit_create(C.byref(cfg), C.byref(self._h))
        if rc == _lib.FQ3_EINVAL:
            raise ValueError(self._lib.fq3_last_error().decode("utf-8", "replace"))
        _lib.check(rc)
        self.tile = int(tile) if tile else self.design.tile
        self.n_in, self.n_out, self.finished = 0, 0, False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.fq3_limit_destroy(h)

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    @property
    def latency(self) -> int:
        return self.design.latency

    def reset(self) -> None:
        """A new stream on the same object."""
        s = self._stream()
        with torch.cuda.device(self.dev):
            _lib.check(self._lib.fq3_limit_reset(self._h, C.c_void_p(s.cuda_stream)))
        self.n_in, self.n_out, self.finished = 0, 0, False

    def push(self, pcm: Optional[torch.Tensor], final: bool = False) -> torch.Tensor:
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            x = None if pcm is None else pcm.reshape(-1)
            if x is not None and (x.dtype != torch.float32 or x.device != self.dev or not x.is_contiguous()):
                x = x.to(device=self.dev, dtype=torch.float32).contiguous()
            n = 0 if x is None else int(x.numel())
            total = self.n_in + n
            room = (total if final else max(0, total - self.design.latency)) - self.n_out
            out = torch.empty(max(room, 0), dtype=torch.float32, device=self.dev)
            got = C.c_int64()
            _lib.check(self._lib.fq3_limit_push(self._h, C.c_void_p(x.data_ptr() if n else None), n, 1 if final else 0,
                                                C.c_void_p(out.data_ptr() if room > 0 else None), max(room, 0), C.byref(got),
                                                C.c_void_p(s.cuda_stream)))
            if n:
                x.record_stream(s)
            out.record_stream(s)
        self.n_in = total
        self.n_out += int(got.value)
        self.finished = self.finished or bool(final)
        return out[:got.value]

    def push_host(self, pcm, final: bool = False) -> np.ndarray:
        """``push`` for a numpy array (or None): copied to the device, limited, copied back (waits for it)."""
        x = None if pcm is None else torch.from_numpy(np.array(pcm, dtype=np.float32).reshape(-1)).to(self.dev)
        with torch.cuda.stream(self._stream()):
            return self.push(x, final).cpu().numpy()

    def stats(self) -> LimiterStats:
        """The accumulators of everything pushed so far (waits for it)."""
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            buf = torch.empty(STATS_BYTES, dtype=torch.uint8, device=self.dev)          # torch aligns allocations far beyond 8 bytes
            _lib.check(self._lib.fq3_limit_stats(self._h, C.c_void_p(buf.data_ptr()), C.c_void_p(s.cuda_stream)))
            return LimiterStats.from_bytes(buf.cpu().numpy().tobytes())


# ---- a group of streams in one launch (the lock-step batch) ----------------------------------------------
GROUP_MAX = _lib.FQ3_STAGE_GROUP_MAX


def _push_group(limiters, pcms, finals):
    """The launches of ``push_group``: -> (the float32 device buffer every row's output lies in, [(offset, count)] per row, the stream)."""
    from .leveller import _float_rows, _group_members
    limiters, pcms, finals = list(limiters), list(pcms), [bool(f) for f in finals]
    dev, s = _group_members("limiter.push_group", limiters, pcms, finals)
    if dev is None:
        return None, [], None
    lib = limiters[0]._lib
    with torch.cuda.device(dev), torch.cuda.stream(s):
        rows = _float_rows(pcms, dev)
        cursor, spans = 0, []
        for lim, (x, n), final in zip(limiters, rows, finals):
            if lim.finished:
                lim.push(x, final)                                 # the library's own answer (FQ3_ESTATE), as ``push`` gives it
            total = lim.n_in + n
            room = max((total if final else max(0, total - lim.design.latency)) - lim.n_out, 0)
            spans.append((cursor, room))                           # back to back: a row starts at whatever float offset it falls on
            cursor += room
        buf = torch.empty(cursor, dtype=torch.float32, device=dev)
        base, sp = buf.data_ptr(), C.c_void_p(s.cuda_stream)
        buckets: dict = {}
        for i, lim in enumerate(limiters):
            buckets.setdefault((lim.in_rate, lim.spec, lim.tile), []).append(i)
        for members in buckets.values():
            for a in range(0, len(members), GROUP_MAX):
                part = members[a:a + GROUP_MAX]
                B = len(part)
                n_out = (C.c_int64 * B)()
                _lib.check(lib.fq3_limit_push_group(
                    (C.c_void_p * B)(*[limiters[i]._h.value for i in part]), B,
                    (C.c_void_p * B)(*[rows[i][0].data_ptr() if rows[i][1] else None for i in part]),
                    (C.c_int64 * B)(*[rows[i][1] for i in part]), (C.c_int * B)(*[int(finals[i]) for i in part]),
                    (C.c_void_p * B)(*[base + 4 * spans[i][0] if spans[i][1] else None for i in part]),
                    (C.c_int64 * B)(*[spans[i][1] for i in part]), n_out, sp))
                for i, got in zip(part, n_out):
                    assert int(got) == spans[i][1]
                    limiters[i].n_in += rows[i][1]
                    limiters[i].n_out += int(got)
                    limiters[i].finished = limiters[i].finished or finals[i]
        for x, n in rows:
            if n:
                x.record_stream(s)
        buf.record_stream(s)
    return buf, spans, s


def push_group(limiters, pcms, finals) -> list:
    """``[limiters[i].push(pcms[i], finals[i]) for i]`` -- the same device tensors, bit for bit, and the same counters on every
    object -- with ONE launch per design instead of one per row (``fq3_limit_push_group``, up to 32 rows a call).  The limiters share
    a device and a stream and appear once; rows are bucketed by design (rate, spec, tile).  All rows' outputs lie back to back, in
    row order, in ONE float32 device buffer, and the results are views of it (``_push_group`` hands out the buffer and the rows'
    places in it, for a caller that lands them in one pinned copy)."""
    buf, spans, _s = _push_group(limiters, pcms, finals)
    return [buf[off:off + cnt] for off, cnt in spans]
