"""A streaming loudness leveller on the device (``fq3_level_*``): float32 mono in, float32 out at the same
rate, length-preserving, ZERO latency, and independent of how the stream was cut into pushes, bit for bit.  The gain of a sample is
built from the BS.1770 hop integers (the loudness meter's own) of the hops that ended before the sample's hop began, so it converges
to the gain one-shot normalisation (``fq3hip/loudness.py``) would have applied to the whole stream.  The stage does NOT limit: a hop
louder than everything before it can pass the ceiling -- run the limiter (``fq3hip/limiter.py``) behind it for that.

``LevelSpec``  what a caller asks for (target, ceiling, largest and initial gain, smoothing, gate on the first blocks); host only
``Leveller``   one stream on a device: ``push`` / ``reset`` / ``stats`` / ``trace`` / ``final_gain_db``"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .loudness import CEILING_RANGE, MAX_GAIN_RANGE, TARGET_RANGE, LoudnessSpec, _db, _number, design as loud_design

INITIAL_GAIN_RANGE, SMOOTH_RANGE, MIN_BLOCKS_RANGE = (-60.0, 40.0), (1, 64), (1, 64)
MAX_HOPS = 1 << 20
STATS_BYTES = C.sizeof(_lib.LevelReport)


def _count(v, what: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}], not {v!r}")
    return int(v)


@dataclass(frozen=True)
class LevelSpec:
    """``target_lufs`` in [-40, -5], ``ceiling_db`` in [-20, 0] and ``max_gain_db`` in [0, 40] mean what they mean in
    ``LoudnessSpec``: the level the stream is brought to, the sample peak (of what was heard SO FAR) the gain respects -- a bound on
    the gain, not a limiter -- and the largest gain.  ``initial_gain_db`` in [-60, 40]: the gain until enough of the stream was
    measured (a voice's last measured gain, if it is known).  ``smooth_hops`` in [1, 64]: the gain is the mean of the last that many
    100 ms targets, ramped linearly inside a hop.  ``min_blocks`` in [1, 64]: 400 ms blocks above the absolute gate before a
    measurement counts -- the first blocks behind leading silence read low.  The defaults (-16 LUFS, -1 dBFS, +20 dB, 0 dB, 10, 8)
    have NOT been tuned on real voices."""
    target_lufs: float = -16.0
    ceiling_db: float = -1.0
    max_gain_db: float = 20.0
    initial_gain_db: float = 0.0
    smooth_hops: int = 10
    min_blocks: int = 8

    def __post_init__(self):
        _number(self.target_lufs, "target_lufs", *TARGET_RANGE)
        _number(self.ceiling_db, "ceiling_db", *CEILING_RANGE)
        _number(self.max_gain_db, "max_gain_db", *MAX_GAIN_RANGE)
        _number(self.initial_gain_db, "initial_gain_db", *INITIAL_GAIN_RANGE)
        _count(self.smooth_hops, "smooth_hops", *SMOOTH_RANGE)
        _count(self.min_blocks, "min_blocks", *MIN_BLOCKS_RANGE)

    @property
    def loudness(self) -> LoudnessSpec:
        return LoudnessSpec(self.target_lufs, self.ceiling_db, self.max_gain_db)

    @property
    def pooled(self) -> "LevelSpec":
        """the spec without its initial gain: what a kept ``Leveller`` is made and matched for (the gain is set per stream, ``reset``)"""
        return self if self.initial_gain_db == 0.0 else dataclasses.replace(self, initial_gain_db=0.0)

    @property
    def g0(self) -> np.float32:
        """``(float) 10^(initial_gain_db / 20)``: computed in double, rounded once"""
        return np.float32(10.0 ** (float(self.initial_gain_db) / 20.0))


@dataclass(frozen=True)
class LevelStats:
    """The newest hop the stream has entered: ``target_gain`` = T, ``smooth_gain`` = S (the gain its last sample gets); ``valid``:
    T is a measured gain (else it is the initial gain: too few blocks above the gate yet, or a non-finite sample).  ``lufs``,
    ``mean_power``, ``n_abs``, ``n_rel``, ``n_bad``: the measure of the ``n_hops`` whole hops in front of it."""
    target_gain: float
    smooth_gain: float
    target_gain_db: float
    smooth_gain_db: float
    valid: bool
    lufs: float
    mean_power: float
    n_hops: int
    n_abs: int
    n_rel: int
    n_bad: int

    @classmethod
    def from_bytes(cls, raw: bytes) -> "LevelStats":
        s = _lib.LevelReport.from_buffer_copy(raw)
        return cls(float(s.target_gain), float(s.smooth_gain), _db(s.target_gain, 20.0), _db(s.smooth_gain, 20.0), bool(s.valid),
                   -0.691 + _db(s.mean_power, 10.0), float(s.mean_power), int(s.n_hops), int(s.n_abs), int(s.n_rel), int(s.n_bad))


def capacity_for(n_samples: int, in_rate: int) -> int:
    """hops a stream of ``n_samples`` needs; ``ValueError`` beyond 2^20"""
    hops = int(n_samples) // (int(in_rate) // 10) + 1
    if hops > MAX_HOPS:
        raise ValueError(f"a levelled stream of {n_samples} samples at {in_rate} Hz has {hops} hops of 100 ms; the limit is 2^20")
    return hops


class Leveller:
    """One stream through the leveller.  ``push(pcm)`` takes the next float32 samples (a device tensor) and returns as many levelled
    ones (a new device tensor; ``out=`` may name one, ``pcm`` itself included) -- at most three launches, nothing synchronises;
    ``push(..., final=True)`` ends the stream.  ``reset()`` starts a new one on the same object (``reset(initial_gain_db)``: from
    another initial gain), ``stats()`` reads the newest gains, ``trace()`` the hop integers and targets so far.  It does NOT limit (see the module text).  Work is enqueued on ``stream``
    (default: the current stream at the time of the call).  ``capacity_hops``: 0 = 4096 hops of 100 ms."""

    def __init__(self, spec: Optional[LevelSpec], in_rate: int, device, stream=None, capacity_hops: int = 0):
        self.spec = LevelSpec() if spec is None else spec
        if not isinstance(self.spec, LevelSpec):
            raise ValueError(f"spec must be a LevelSpec or None, not {type(spec).__name__}")
        self.in_rate = int(in_rate)
        self.design = loud_design(self.in_rate, self.spec.loudness)
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        if self.dev.type != "cuda":
            raise ValueError("Leveller runs on the GPU; there is no CPU fallback")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.stream = stream
        self._lib = _lib.load()
        self._h = C.c_void_p()
        sp = self.spec
        cfg = _lib.LevelConfig(self.in_rate, float(sp.target_lufs), float(sp.ceiling_db), float(sp.max_gain_db), float(sp.initial_gain_db),
                               int(sp.smooth_hops), int(sp.min_blocks), int(capacity_hops))
        with torch.cuda.device(self.dev):
            rc = self._lib.fq3_level_create(C.byref(cfg), C.byref(self._h))
        if rc == _lib.FQ3_EINVAL:
            raise ValueError(self._lib.fq3_last_error().decode("utf-8", "replace"))
        _lib.check(rc)
        self.capacity_hops = int(capacity_hops) if capacity_hops else 4096
        self.n_in, self.finished = 0, False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.fq3_level_destroy(h)

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def reset(self, initial_gain_db: Optional[float] = None) -> None:
        """A new stream on the same object.  ``initial_gain_db`` (None: the one it had): the gain the new stream starts from -- the
        object's ``spec`` then says so -- which is how ONE kept object serves streams that start from different gains."""
        if initial_gain_db is not None:
            spec = dataclasses.replace(self.spec, initial_gain_db=float(initial_gain_db))        # (ValueError outside [-60, 40])
        _lib.check(self._lib.fq3_level_reset(self._h, C.c_void_p(self._stream().cuda_stream)))
        if initial_gain_db is not None:
            _lib.check(self._lib.fq3_level_set_initial_gain(self._h, float(initial_gain_db)))
            self.spec = spec
        self.n_in, self.finished = 0, False

    def push(self, pcm: Optional[torch.Tensor], final: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            x = None if pcm is None else pcm.reshape(-1)
            if x is not None and (x.dtype != torch.float32 or x.device != self.dev or not x.is_contiguous()):
                x = x.to(device=self.dev, dtype=torch.float32).contiguous()
            n = 0 if x is None else int(x.numel())
            if out is None:
                out = torch.empty(n, dtype=torch.float32, device=self.dev)
            elif out.dtype != torch.float32 or out.device != self.dev or not out.is_contiguous() or int(out.numel()) != n:
                raise ValueError("out must be a contiguous float32 tensor of the input's length on the leveller's device")
            _lib.check(self._lib.fq3_level_push(self._h, C.c_void_p(x.data_ptr() if n else None), n, 1 if final else 0,
                                                C.c_void_p(out.data_ptr() if n else None), C.c_void_p(s.cuda_stream)))
            if n:
                x.record_stream(s)
            out.record_stream(s)
        self.n_in += n
        self.finished = self.finished or bool(final)
        return out.reshape(-1)

    def stats_buffer(self) -> torch.Tensor:
        """``fq3_level_report`` of the pushes so far in a fresh device buffer (one launch, nothing synchronises)"""
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            buf = torch.empty(STATS_BYTES, dtype=torch.uint8, device=self.dev)          # torch aligns allocations far beyond 8 bytes
            _lib.check(self._lib.fq3_level_stats(self._h, C.c_void_p(buf.data_ptr()), C.c_void_p(s.cuda_stream)))
            buf.record_stream(s)
        return buf

    def stats(self) -> LevelStats:
        """The newest gains and the measure behind them (waits for the pushes so far)."""
        buf = self.stats_buffer()
        with torch.cuda.stream(self._stream()):
            return LevelStats.from_bytes(buf.cpu().numpy().tobytes())

    @property
    def final_gain_db(self) -> Optional[float]:
        """The newest target in dB -- what a voice's next stream may start from as ``initial_gain_db`` -- or None while the measure is
        invalid (waits for the pushes so far)."""
        st = self.stats()
        return st.target_gain_db if st.valid and math.isfinite(st.target_gain_db) else None

    def trace(self) -> dict:
        """For tests and probes: ``energy`` (uint64), ``peak`` (float32) and ``bad`` (int32) of the whole hops so far and ``target``
        (float32, T(0 .. n_hops)); waits for them."""
        s = self._stream()
        n_max = self.n_in // self.design.H
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            e = torch.empty(max(n_max, 1), dtype=torch.int64, device=self.dev)
            p = torch.empty(max(n_max, 1), dtype=torch.float32, device=self.dev)
            b = torch.empty(max(n_max, 1), dtype=torch.int32, device=self.dev)
            t = torch.full((n_max + 1,), float(self.spec.g0), dtype=torch.float32, device=self.dev)     # (before the first sample: T(0) = g0)
            got = C.c_int64()
            _lib.check(self._lib.fq3_level_trace(self._h, C.c_void_p(e.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(b.data_ptr()),
                                                 C.c_void_p(t.data_ptr()), n_max, C.byref(got), C.c_void_p(s.cuda_stream)))
            n = int(got.value)
            return dict(energy=e[:n].cpu().numpy().view(np.uint64), peak=p[:n].cpu().numpy(), bad=b[:n].cpu().numpy(),
                        target=t[:n + 1].cpu().numpy())


# ---- a group of streams in one launch set (the lock-step batch) -----------------------------------------
GROUP_MAX = _lib.FQ3_STAGE_GROUP_MAX


def _group_members(what: str, stages, pcms, finals):
    """the checks every group function makes on the host: one pcm and flag per stage, no stage twice, one device and one stream"""
    if not (len(stages) == len(pcms) == len(finals)):
        raise ValueError(f"{what}: one pcm and one final flag per stage")
    if len(set(map(id, stages))) != len(stages):
        raise ValueError(f"{what}: the same stage twice in one call")
    if not stages:
        return None, None
    dev, s = stages[0].dev, stages[0]._stream()
    for st in stages:
        if st.dev != dev or st._stream().cuda_stream != s.cuda_stream:
            raise ValueError(f"{what}: the stages of one call share a device and a stream")
    return dev, s


def _float_rows(pcms, dev):
    """every pcm as a contiguous float32 vector on ``dev`` (None: no samples) -> [(tensor | None, length)]"""
    rows = []
    for pcm in pcms:
        x = None if pcm is None else pcm.reshape(-1)
        if x is not None and (x.dtype != torch.float32 or x.device != dev or not x.is_contiguous()):
            x = x.to(device=dev, dtype=torch.float32).contiguous()
        rows.append((x, 0 if x is None else int(x.numel())))
    return rows


def push_group(levellers, pcms, finals, outs=None) -> list:
    """``[levellers[i].push(pcms[i], finals[i], out=outs[i]) for i]`` -- the same device tensors, bit for bit, and the same counters
    on every object -- with at most THREE launches per design (the meters', the targets', the multiplies') instead of three per row
    (``fq3_leveller_push_group``, up to 32 rows a call).  The levellers share a device and a stream and appear once; rows are bucketed
    by design (rate and ``spec.pooled``: the initial gain may differ per row).  ``outs`` (None, or per row a tensor or None): where
    a row's samples go, ``pcms[i]`` itself included; rows without one lie in one new device buffer.  A row the library would refuse
    is refused before any object moves, with its single push's own error."""
    levellers, pcms, finals = list(levellers), list(pcms), [bool(f) for f in finals]
    outs = [None] * len(levellers) if outs is None else list(outs)
    if len(outs) != len(levellers):
        raise ValueError("leveller.push_group: one out (or None) per leveller")
    dev, s = _group_members("leveller.push_group", levellers, pcms, finals)
    if dev is None:
        return []
    lib = levellers[0]._lib
    with torch.cuda.device(dev), torch.cuda.stream(s):
        rows = _float_rows(pcms, dev)
        cursor, offs = 0, []
        for lev, (x, n), final, out in zip(levellers, rows, finals, outs):
            if out is not None and (out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or int(out.numel()) != n):
                raise ValueError("out must be a contiguous float32 tensor of the input's length on the leveller's device")
            if lev.finished or (lev.n_in + n) // lev.design.H > lev.capacity_hops:
                lev.push(x, final, out=out)                        # the library's own answer (FQ3_ESTATE, FQ3_ETOOLONG), as ``push`` gives it
            if out is None and n:
                # a new row begins where its source does modulo 16 bytes: the multiply then moves 16 bytes per lane
                cursor = (cursor + 3) // 4 * 4 + ((x.data_ptr() >> 2) & 3)
                offs.append(cursor)
                cursor += n
            else:
                offs.append(None)
        buf = torch.empty(cursor, dtype=torch.float32, device=dev)
        result = [out if out is not None else (buf[off:off + n] if n else buf[:0]) for out, off, (_x, n) in zip(outs, offs, rows)]
        buckets: dict = {}
        for i, lev in enumerate(levellers):
            buckets.setdefault((lev.in_rate, lev.spec.pooled), []).append(i)
        sp = C.c_void_p(s.cuda_stream)
        for members in buckets.values():
            for a in range(0, len(members), GROUP_MAX):
                part = members[a:a + GROUP_MAX]
                B = len(part)
                _lib.check(lib.fq3_leveller_push_group(
                    (C.c_void_p * B)(*[levellers[i]._h.value for i in part]), B,
                    (C.c_void_p * B)(*[rows[i][0].data_ptr() if rows[i][1] else None for i in part]),
                    (C.c_int64 * B)(*[rows[i][1] for i in part]), (C.c_int * B)(*[int(finals[i]) for i in part]),
                    (C.c_void_p * B)(*[result[i].data_ptr() if rows[i][1] else None for i in part]), sp))
                for i in part:
                    levellers[i].n_in += rows[i][1]
                    levellers[i].finished = levellers[i].finished or finals[i]
        for (x, n), y in zip(rows, result):
            if n:
                x.record_stream(s)
            y.record_stream(s)
    return [y.reshape(-1) for y in result]
