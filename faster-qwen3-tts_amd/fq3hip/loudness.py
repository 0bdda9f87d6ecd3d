"""Loudness on the device: an ITU-R BS.1770-4 meter (mono, integrated, gated; ``fq3_loud_*``) over the
vocoder's float32 PCM, the gain that brings an utterance to a target level under a sample-peak ceiling, and the multiply that
applies a gain -- so that no waveform crosses to the host and back to be levelled.  The measure does not depend on how a stream was
cut into pushes: hop energies are integers.

``LoudnessSpec``   what a caller asks for (target, ceiling, largest gain); host only, validates without a GPU
``design``         the numbers the device works with (``fq3_loud_design``; no GPU needed)
``LoudnessMeter``  one stream's meter on a device: ``push`` / ``finish`` / ``stats`` / ``hops`` / ``normalise`` / ``apply``
``apply_gain``     ``wav * gain`` with the gain read from a 1-element device tensor"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

TARGET_RANGE, CEILING_RANGE, MAX_GAIN_RANGE = (-40.0, -5.0), (-20.0, 0.0), (0.0, 40.0)
STATS_BYTES = C.sizeof(_lib.LoudStats)
_GAIN_OFFSET = _lib.LoudStats.gain.offset


def _number(v, what: str, lo: float, hi: float) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a number in [{lo:g}, {hi:g}], not {v!r}")
    if not lo <= float(v) <= hi:
        raise ValueError(f"{what} {v!r} is outside [{lo:g}, {hi:g}]")
    return float(v)


@dataclass(frozen=True)
class LoudnessSpec:
    """``target_lufs`` in [-40, -5]: the integrated loudness an utterance is brought to.  ``ceiling_db`` in [-20, 0]: the sample peak
    (dBFS) the gain may not push the utterance above -- a bound on the gain, not a limiter.  ``max_gain_db`` in [0, 40]: the largest
    gain, so that a near-silent utterance is not blown up.  The defaults (-16 LUFS, -1 dBFS, +20 dB) are common delivery figures; they
    have NOT been tuned on real voices."""
    target_lufs: float = -16.0
    ceiling_db: float = -1.0
    max_gain_db: float = 20.0

    def __post_init__(self):
        _number(self.target_lufs, "target_lufs", *TARGET_RANGE)
        _number(self.ceiling_db, "ceiling_db", *CEILING_RANGE)
        _number(self.max_gain_db, "max_gain_db", *MAX_GAIN_RANGE)


def gain_factor(gain_db) -> float:
    """``10^(gain_db / 20)`` of a fixed gain; ``ValueError`` unless ``gain_db`` is a finite number in [-60, 40]."""
    return 10.0 ** (_number(gain_db, "gain_db", -60.0, 40.0) / 20.0)


@dataclass(frozen=True)
class LoudnessDesign:
    """What ``fq3_loud_design`` hands back: hop length, the K-weighting coefficients (shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2)
    in double and rounded to float32 (the device's), the absolute gate as an integer, and the gain constants as doubles."""
    H: int
    coef64: Tuple[float, ...]
    coef32: Tuple[np.float32, ...]
    abs_gate: int
    target_power: float
    ceiling: float
    max_gain: float


def design(in_rate: int, spec: Optional[LoudnessSpec] = None) -> LoudnessDesign:
    """``fq3_loud_design`` (host only, no GPU needed); ``ValueError`` with the library's reason for a rate it refuses."""
    spec = LoudnessSpec() if spec is None else spec
    lib = _lib.load()
    H, gate = C.c_int(), C.c_uint64()
    c64, c32 = (C.c_double * 10)(), (C.c_float * 10)()
    T, Cc, G = C.c_double(), C.c_double(), C.c_double()
    rc = lib.fq3_loud_design(int(in_rate), float(spec.target_lufs), float(spec.ceiling_db), float(spec.max_gain_db), C.byref(H), c64, c32,
                             C.byref(gate), C.byref(T), C.byref(Cc), C.byref(G))
    if rc != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return LoudnessDesign(H.value, tuple(float(v) for v in c64), tuple(np.float32(v) for v in c32), int(gate.value), T.value, Cc.value,
                          G.value)


def _db(v: float, scale: float) -> float:
    return scale * math.log10(v) if v > 0 else float("-inf")


@dataclass(frozen=True)
class LoudnessStats:
    """A measurement on the host.  ``lufs`` = -0.691 + 10 log10(``mean_power``) (-inf without a gated block), ``peak_db`` the sample
    peak in dBFS, ``gain_db`` the gain the device chose (0 when ``valid`` is False: fewer than 4 hops of 100 ms, nothing above the
    absolute gate, or ``n_bad`` non-finite samples).  ``n_abs`` / ``n_rel``: the 400 ms blocks that passed the absolute / both gates."""
    lufs: float
    peak_db: float
    gain_db: float
    valid: bool
    mean_power: float
    peak: float
    gain: float
    n_hops: int
    n_abs: int
    n_rel: int
    n_bad: int

    @classmethod
    def from_bytes(cls, raw: bytes) -> "LoudnessStats":
        s = _lib.LoudStats.from_buffer_copy(raw)
        return cls(lufs=-0.691 + _db(s.mean_power, 10.0), peak_db=_db(s.peak, 20.0), gain_db=_db(s.gain, 20.0), valid=bool(s.valid),
                   mean_power=float(s.mean_power), peak=float(s.peak), gain=float(s.gain), n_hops=int(s.n_hops), n_abs=int(s.n_abs),
                   n_rel=int(s.n_rel), n_bad=int(s.n_bad))

    @classmethod
    def from_device(cls, buf: torch.Tensor) -> "LoudnessStats":
        """``buf``: what ``LoudnessMeter.finish`` returned (waits for the work queued in front of the copy)"""
        return cls.from_bytes(buf.cpu().numpy().tobytes())


def gain_of(stats_buf: torch.Tensor) -> torch.Tensor:
    """the 1-element float32 device tensor inside a device stats buffer that holds the gain"""
    return stats_buf[_GAIN_OFFSET:_GAIN_OFFSET + 4].view(torch.float32)


def apply_gain(wav: torch.Tensor, gain: torch.Tensor, stream=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = wav * gain[0]`` on the device (``fq3_loud_apply``: one fp32 multiply per sample, the factor read on the device).  ``wav``:
    a contiguous float32 device tensor of any shape; ``out`` (default: a new tensor; may be ``wav`` itself) the same shape.  Enqueued on
    ``stream`` (default: the current stream); nothing synchronises."""
    if not wav.is_cuda or wav.dtype != torch.float32 or not wav.is_contiguous():
        raise ValueError("apply_gain takes a contiguous float32 device tensor; there is no CPU fallback")
    if gain.device != wav.device or gain.dtype != torch.float32 or gain.numel() != 1:
        raise ValueError("the gain must be a 1-element float32 tensor on the waveform's device")
    s = stream if stream is not None else torch.cuda.current_stream(wav.device)
    with torch.cuda.device(wav.device), torch.cuda.stream(s):
        if out is None:
            out = torch.empty_like(wav)
        elif out.shape != wav.shape or out.dtype != wav.dtype or out.device != wav.device or not out.is_contiguous():
            raise ValueError("out must match the waveform")
        n = int(wav.numel())
        _lib.check(_lib.load().fq3_loud_apply(C.c_void_p(gain.data_ptr()), C.c_void_p(wav.data_ptr() if n else None), n,
                                              C.c_void_p(out.data_ptr() if n else None), C.c_void_p(s.cuda_stream)))
        for t in (wav, gain, out):
            t.record_stream(s)
    return out


class LoudnessMeter:
    """One stream through the meter.  ``push(pcm)`` takes the next float32 samples (a device tensor; one launch), ``push(...,
    final=True)`` ends the stream; ``finish()`` runs the gating and the gain on the device and returns the device stats buffer
    (``gain_of(buf)`` is the 1-element gain tensor ``apply`` reads), ``stats()`` brings the last one to the host.  ``normalise(wav)``
    is the whole thing for one utterance: reset, measure, finish, scale -- four launches, no synchronisation.  Work is enqueued on
    ``stream`` (default: the current stream at the time of the call).  ``capacity_hops``: 0 = 4096 hops of 100 ms."""

    def __init__(self, spec: Optional[LoudnessSpec], in_rate: int, device, stream=None, capacity_hops: int = 0):
        self.spec = LoudnessSpec() if spec is None else spec
        if not isinstance(self.spec, LoudnessSpec):
            raise ValueError(f"spec must be a LoudnessSpec or None, not {type(spec).__name__}")
        self.in_rate = int(in_rate)
        self.design = design(self.in_rate, self.spec)
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        if self.dev.type != "cuda":
            raise ValueError("LoudnessMeter runs on the GPU; there is no CPU fallback")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.stream = stream
        self._lib = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.LoudConfig(self.in_rate, float(self.spec.target_lufs), float(self.spec.ceiling_db), float(self.spec.max_gain_db),
                              int(capacity_hops))
        with torch.cuda.device(self.dev):
            rc = self._lib.fq3_loud_create(C.byref(cfg), C.byref(self._h))
        if rc == _lib.FQ3_EINVAL:
            raise ValueError(self._lib.fq3_last_error().decode("utf-8", "replace"))
        _lib.check(rc)
        self.n_in, self.finished, self._stats = 0, False, None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.fq3_loud_destroy(h)

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def reset(self) -> None:
        """A new utterance on the same object."""
        _lib.check(self._lib.fq3_loud_reset(self._h, C.c_void_p(self._stream().cuda_stream)))
        self.n_in, self.finished, self._stats = 0, False, None

    def push(self, pcm: Optional[torch.Tensor], final: bool = False) -> None:
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            x = None if pcm is None else pcm.reshape(-1)
            if x is not None and (x.dtype != torch.float32 or x.device != self.dev or not x.is_contiguous()):
                x = x.to(device=self.dev, dtype=torch.float32).contiguous()
            n = 0 if x is None else int(x.numel())
            _lib.check(self._lib.fq3_loud_push(self._h, C.c_void_p(x.data_ptr() if n else None), n, 1 if final else 0,
                                               C.c_void_p(s.cuda_stream)))
            if n:
                x.record_stream(s)
        self.n_in += n
        self.finished = self.finished or bool(final)

    def finish(self) -> torch.Tensor:
        """Gating and gain on the device -> a fresh device buffer holding ``fq3_loud_stats`` (kept as the meter's last measurement)."""
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            buf = torch.empty(STATS_BYTES, dtype=torch.uint8, device=self.dev)          # torch aligns allocations far beyond 8 bytes
            _lib.check(self._lib.fq3_loud_finish(self._h, C.c_void_p(buf.data_ptr()), C.c_void_p(s.cuda_stream)))
            buf.record_stream(s)
        self._stats = buf
        return buf

    def stats(self) -> LoudnessStats:
        """The last ``finish`` on the host (``finish`` is run first when the stream has ended and it has not been); waits for it."""
        if self._stats is None:
            self.finish()
        with torch.cuda.stream(self._stream()):
            return LoudnessStats.from_device(self._stats)

    def hops(self) -> np.ndarray:
        """The energies of the hops completed so far, ``uint64`` (for tests and probes; waits for them)."""
        s = self._stream()
        n_max = self.n_in // self.design.H
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            out = torch.empty(max(n_max, 1), dtype=torch.int64, device=self.dev)
            got = C.c_int64()
            _lib.check(self._lib.fq3_loud_hops(self._h, C.c_void_p(out.data_ptr()), n_max, C.byref(got), C.c_void_p(s.cuda_stream)))
            return out[:got.value].cpu().numpy().view(np.uint64)

    def normalise(self, wav: torch.Tensor) -> torch.Tensor:
        """One utterance: measured, then scaled to the target -> a new device tensor of ``wav``'s shape.  The stats stay on the device
        (``stats()`` fetches them); an utterance that cannot be measured comes back unscaled (gain 1)."""
        x = wav if wav.is_cuda and wav.dtype == torch.float32 and wav.is_contiguous() else wav.to(device=self.dev, dtype=torch.float32).contiguous()
        self.reset()
        self.push(x, final=True)
        return apply_gain(x, gain_of(self.finish()), self._stream())

    def apply(self, wav: torch.Tensor, gain_tensor: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``wav * gain_tensor[0]`` on this meter's stream (see ``apply_gain``)."""
        return apply_gain(wav, gain_tensor, self._stream(), out)


class LoudnessSession:
    """What ``FasterQwen3TTS.loudness`` yields: the context's ``spec`` and, after every call made inside it, the measurements of that
    call's utterances in output order (one per utterance of a batch call, one per segment of a long-form call) -- kept on the device
    until ``stats`` is read."""

    def __init__(self, spec: LoudnessSpec):
        self.spec = spec
        self._bufs: list = []

    def begin(self, n: Optional[int] = None) -> None:
        """a new call with ``n`` utterances (None: they are appended as they come)"""
        self._bufs = [] if n is None else [None] * int(n)

    def put(self, key, buf: torch.Tensor) -> None:
        if key is None:
            self._bufs.append(buf)
        else:
            self._bufs[key] = buf

    @property
    def stats(self) -> list:
        """``LoudnessStats`` per utterance of the last call (None for one that produced no audio); waits for the device"""
        out = []
        for b in self._bufs:
            if b is not None:
                torch.cuda.synchronize(b.device)
            out.append(None if b is None else LoudnessStats.from_device(b))
        return out
