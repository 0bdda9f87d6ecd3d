"""Device audio output stage: the vocoder's float32 PCM is resampled and encoded on the GPU (``fq3_audio_out_*``, one HIP launch
per chunk) before it is copied to the host, so that a client gets the rate and sample encoding it asked for -- 8 kHz mu-law for
telephony, 16 kHz s16, 44.1 / 48 kHz -- and only those bytes cross the bus.  The result does not depend on how the stream was cut
into chunks.  A ``speed`` other than 1 puts the time-scale stage in front (``fq3_tsm_*``: WSOLA, one more
launch per chunk; duration changes, pitch does not), with the same contract.  The ``flac`` encoding puts the
FLAC stage behind the s16 encoder (``fq3_flac_*``: lossless, a launch pair per chunk): what leaves the chain
then is FLAC frames, and the 42-byte stream header comes from the host (``flac_header``).

``AudioOutSpec``  what a caller asks for (rate, encoding, speed); host only, validates without a GPU
``AudioOut``      one stream's time-scale + resampler + encoder state on a device
``push_group`` / ``push_group_host`` / ``GroupCopy``  many streams' pushes in one launch per stage (the lock-step batch; section 4.17)
``resample_device``  one-shot form, host array in, host array out"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

# ``flac`` is the s16 encoding followed by the FLAC stage: the output stage itself runs in FQ3_PCM_S16
ENCODINGS = {"f32": _lib.FQ3_PCM_F32, "s16": _lib.FQ3_PCM_S16, "mulaw": _lib.FQ3_PCM_MULAW, "alaw": _lib.FQ3_PCM_ALAW,
             "flac": _lib.FQ3_PCM_S16}
_DTYPES = {"f32": torch.float32, "s16": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8, "flac": torch.uint8}
NUMPY_DTYPES = {"f32": np.float32, "s16": np.dtype("<i2"), "mulaw": np.uint8, "alaw": np.uint8, "flac": np.uint8}
FLAC_HEADER_BYTES = 42
MIN_SPEED, MAX_SPEED = 0.25, 4.0


@dataclass(frozen=True)
class AudioOutSpec:
    """``sample_rate`` None: the model's rate.  ``encoding``: ``f32`` | ``s16`` | ``mulaw`` | ``alaw`` | ``flac`` (the s16 samples, losslessly
    compressed; the output is bytes, not samples).  ``speed`` in [0.25, 4.0], applied in per-mille steps; 1.0: no time-scale stage at
    all."""
    sample_rate: Optional[int] = None
    encoding: str = "f32"
    speed: float = 1.0

    def __post_init__(self):
        sp = self.speed
        if isinstance(sp, bool) or not isinstance(sp, (int, float, np.integer, np.floating)) or not math.isfinite(sp):
            raise ValueError(f"speed must be a number in [{MIN_SPEED}, {MAX_SPEED}], not {sp!r}")
        if not 1000 * MIN_SPEED <= round(float(sp) * 1000) <= 1000 * MAX_SPEED:
            raise ValueError(f"speed {sp!r} is outside [{MIN_SPEED}, {MAX_SPEED}]")
        if self.encoding not in ENCODINGS:
            raise ValueError(f"unknown audio encoding {self.encoding!r}: one of {', '.join(ENCODINGS)}")
        if self.sample_rate is not None and (isinstance(self.sample_rate, bool) or not isinstance(self.sample_rate, (int, np.integer))):
            raise ValueError(f"sample_rate must be an integer number of Hz, not {self.sample_rate!r}")

    def out_rate(self, in_rate: int) -> int:
        return int(in_rate) if self.sample_rate is None else int(self.sample_rate)

    @property
    def permille(self) -> int:
        """``speed`` as the library applies it: quantised once, to per-mille"""
        return int(round(float(self.speed) * 1000))

    def validate(self, in_rate: int) -> "AudioOutSpec":
        """Raises ``ValueError`` with the library's reason when the resampler refuses ``in_rate -> sample_rate`` or the time-scale
        stage refuses ``in_rate``, or the FLAC stage the output rate (host only)."""
        design(int(in_rate), self.out_rate(in_rate), bank=False)
        if self.encoding == "flac":
            flac_design(self.out_rate(in_rate))
        if self.permille != 1000:
            tsm_design(int(in_rate), self.permille, window=False)
        return self


def design(in_rate: int, out_rate: int, zero_crossings: int = 0, bank: bool = True):
    """``(L, M, K, bank float32[L, K] or None)`` of a rate pair (``fq3_audio_out_design``; no GPU needed)."""
    lib = _lib.load()
    L, M, K = C.c_int(), C.c_int(), C.c_int()
    rc = lib.fq3_audio_out_design(in_rate, out_rate, zero_crossings, C.byref(L), C.byref(M), C.byref(K), None, 0)
    if rc != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    if not bank:
        return L.value, M.value, K.value, None
    b = np.empty((L.value, K.value), dtype=np.float32)
    _lib.check(lib.fq3_audio_out_design(in_rate, out_rate, zero_crossings, C.byref(L), C.byref(M), C.byref(K),
                                        b.ctypes.data_as(C.POINTER(C.c_float)), b.size))
    return L.value, M.value, K.value, b


def count(in_rate: int, out_rate: int, n_in: int, final: bool, zero_crossings: int = 0) -> int:
    """Output samples that exist once ``n_in`` samples of a stream were pushed (``fq3_audio_out_count``)."""
    n = _lib.load().fq3_audio_out_count(in_rate, out_rate, zero_crossings, n_in, 1 if final else 0)
    if n < 0:
        _lib.check(int(n))
    return int(n)


def tsm_design(in_rate: int, permille: int, window: bool = True):
    """``(N, Hs, delta, window float32[N] or None)`` of the time-scale stage at ``in_rate`` (``fq3_tsm_design``; no GPU needed)."""
    lib = _lib.load()
    N, Hs, D = C.c_int(), C.c_int(), C.c_int()
    rc = lib.fq3_tsm_design(in_rate, permille, C.byref(N), C.byref(Hs), C.byref(D), None, 0)
    if rc != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    if not window:
        return N.value, Hs.value, D.value, None
    w = np.empty(N.value, dtype=np.float32)
    _lib.check(lib.fq3_tsm_design(in_rate, permille, C.byref(N), C.byref(Hs), C.byref(D), w.ctypes.data_as(C.POINTER(C.c_float)), w.size))
    return N.value, Hs.value, D.value, w


def tsm_count(in_rate: int, permille: int, n_in: int, final: bool) -> int:
    """Time-scaled samples that exist once ``n_in`` samples of a stream were pushed (``fq3_tsm_count``)."""
    n = _lib.load().fq3_tsm_count(in_rate, permille, n_in, 1 if final else 0)
    if n < 0:
        _lib.check(int(n))
    return int(n)


def flac_design(rate: int, block: int = 0):
    """``(block size in force, frame bound 2 * block + 18 bytes)`` of the FLAC stage (``fq3_flac_design``; no GPU needed)."""
    lib = _lib.load()
    b, m = C.c_int(), C.c_int()
    if lib.fq3_flac_design(int(rate), int(block), C.byref(b), C.byref(m)) != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return b.value, m.value


def flac_count(rate: int, block: int, n_in: int, final: bool) -> int:
    """FLAC frames that exist once ``n_in`` samples of a stream were pushed (``fq3_flac_count``)."""
    n = _lib.load().fq3_flac_count(int(rate), int(block), int(n_in), 1 if final else 0)
    if n < 0:
        _lib.check(int(n))
    return int(n)


def flac_header(rate: int, block: int = 0, total: int = 0) -> bytes:
    """The 42 bytes in front of a FLAC stream's frames (``fq3_flac_header``; no GPU needed).  ``total`` 0: length unknown."""
    lib = _lib.load()
    buf = (C.c_uint8 * FLAC_HEADER_BYTES)()
    if lib.fq3_flac_header(int(rate), int(block), int(total), buf, FLAC_HEADER_BYTES) != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return bytes(buf)


class AudioOut:
    """One stream through the stage.  ``push(pcm)`` takes the next float32 samples (a device tensor) and returns the output samples
    they complete as a device tensor (float32 / int16 / uint8); ``push(..., final=True)`` ends the stream and returns the rest.
    Work is enqueued on ``stream`` (default: the current stream at the time of the call); nothing synchronises.

    With a ``speed`` other than 1 the samples first go through the time-scale stage (one launch of its own, one intermediate device
    tensor per push), which holds back about 30 ms of input (N + delta = 3 hops of in_rate / 100 samples) until the final push.
    ``n_in`` counts the vocoder's samples, ``n_out`` what has left the chain.

    With the ``flac`` encoding the s16 samples go into an intermediate device tensor and through the FLAC stage (a launch pair per 64
    frames), which holds back the samples behind the last whole block (up to 48 ms at 24 kHz) until the final push.  ``push`` then
    returns the bytes of the frames this push completes -- without the stream header: ``header()`` -- and ``n_out`` counts bytes
    (``n_samples``, with every encoding, the samples that left the resample + encode launch).  How many bytes that is only the device
    knows: ``push`` reads the 8-byte length (one synchronisation of the stream) and slices; ``push_host`` copies the length and the
    frame buffer to the host in ONE transfer and slices there, so that a caller who wants the bytes on the host pays the one
    synchronisation its copy has anyway."""

    def __init__(self, spec: AudioOutSpec, in_rate: int, device, stream=None, zero_crossings: int = 0, flac_block: int = 0):
        self.spec, self.in_rate, self.out_rate = spec, int(in_rate), spec.out_rate(in_rate)
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        if self.dev.type != "cuda":
            raise ValueError("AudioOut runs on the GPU; there is no CPU fallback")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.stream, self.zero = stream, int(zero_crossings)
        self.dtype = torch.int16 if spec.encoding == "flac" else _DTYPES[spec.encoding]      # what the resample + encode launch writes
        self.permille = spec.permille
        self._lib = _lib.load()
        self._h = self._tsm = self._flac = None
        self.flac = spec.encoding == "flac"
        # speed alone (the model's rate, float32): the time-scale stage writes the output itself, no second launch
        self._encode = self.permille == 1000 or self.out_rate != self.in_rate or spec.encoding != "f32"
        with torch.cuda.device(self.dev):
            if self.permille != 1000:
                self._tsm = self._create(self._lib.fq3_tsm_create, _lib.TsmConfig(self.in_rate, self.permille))
            if self._encode:
                self._h = self._create(self._lib.fq3_audio_out_create,
                                       _lib.AudioOutConfig(self.in_rate, self.out_rate, ENCODINGS[spec.encoding], self.zero))
            if self.flac:
                self.flac_block, self.flac_bound = flac_design(self.out_rate, flac_block)
                self._flac = self._create(self._lib.fq3_flac_create, _lib.FlacConfig(self.out_rate, self.flac_block))
        self.n_in = self.n_mid = self.n_out = self.n_samples = 0
        self.finished = False
        self._empty = torch.empty(0, dtype=torch.float32, device=self.dev)

    def _create(self, fn, cfg):
        h = C.c_void_p()
        rc = fn(C.byref(cfg), C.byref(h))
        if rc == _lib.FQ3_EINVAL:
            raise ValueError(self._lib.fq3_last_error().decode("utf-8", "replace"))
        _lib.check(rc)
        return h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.fq3_audio_out_destroy(h)
        t, self._tsm = getattr(self, "_tsm", None), None
        if t:
            self._lib.fq3_tsm_destroy(t)
        f, self._flac = getattr(self, "_flac", None), None
        if f:
            self._lib.fq3_flac_destroy(f)

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def reset(self) -> None:
        """A new utterance on the same object."""
        s = C.c_void_p(self._stream().cuda_stream)
        if self._tsm:
            _lib.check(self._lib.fq3_tsm_reset(self._tsm, s))
        if self._h:
            _lib.check(self._lib.fq3_audio_out_reset(self._h, s))
        if self._flac:
            _lib.check(self._lib.fq3_flac_reset(self._flac, s))
        self.n_in = self.n_mid = self.n_out = self.n_samples = 0
        self.finished = False

    def push(self, pcm: Optional[torch.Tensor], final: bool = False) -> torch.Tensor:
        if self.flac:
            buf = self._push_flac(pcm, final)
            with torch.cuda.stream(self._stream()):            # (the copy must queue behind the stage's launches, on ITS stream)
                n = int(buf[:8].view(torch.int64).item())      # the one synchronisation: how many bytes the frames took
            self.n_out += n
            return buf[8: 8 + n]
        return self.push_into(pcm, final, None)

    def push_host(self, pcm: Optional[torch.Tensor], final: bool = False) -> np.ndarray:
        """``push`` with the result on the host.  ``flac``: the length and the frames cross in one copy (one synchronisation)."""
        if not self.flac:
            return self.push(pcm, final).cpu().numpy()
        buf = self._push_flac(pcm, final)
        with torch.cuda.stream(self._stream()):
            host = buf.cpu().numpy()
        n = int(host[:8].view(np.int64)[0])
        self.n_out += n
        return host[8: 8 + n]

    def header(self, total: int = 0) -> bytes:
        """``flac``: the stream header (``total`` samples; 0: unknown) that goes in front of everything ``push`` returns."""
        if not self.flac:
            raise ValueError("only the flac encoding has a stream header")
        return flac_header(self.out_rate, self.flac_block, total)

    def _push_flac(self, pcm: Optional[torch.Tensor], final: bool):
        """-> device uint8 buffer: the total length of the frames this push completes as an int64, then the frames back to back"""
        s = self._stream()
        before = self.n_samples
        pcm16 = self.push_into(pcm, final, None)               # the s16 half of the chain, through the code every encoding shares
        n = int(pcm16.numel())
        assert self.n_samples == before + n
        frames = flac_count(self.out_rate, self.flac_block, self.n_samples, final) - flac_count(self.out_rate, self.flac_block, before, False)
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            cap = frames * self.flac_bound
            buf = torch.empty(8 + cap, dtype=torch.uint8, device=self.dev)          # torch aligns allocations far beyond 8 bytes
            got = C.c_int64()
            _lib.check(self._lib.fq3_flac_push(self._flac, C.c_void_p(pcm16.data_ptr() if n else None), n, 1 if final else 0,
                                               C.c_void_p(buf.data_ptr() + 8 if cap else None), cap, C.byref(got),
                                               C.c_void_p(buf.data_ptr()), C.c_void_p(s.cuda_stream)))
            assert got.value == frames
            if n:
                pcm16.record_stream(s)
        return buf

    def _counts(self, n_in: int, final: bool):
        """(time-scaled samples, output samples) that exist once ``n_in`` samples of the stream were pushed"""
        mid = tsm_count(self.in_rate, self.permille, n_in, final) if self._tsm else n_in
        return mid, (count(self.in_rate, self.out_rate, mid, final, self.zero) if self._encode else mid)

    def push_into(self, pcm: Optional[torch.Tensor], final: bool, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``push`` into ``out`` (a device tensor of the stage's dtype with room for the samples this push completes; None: a new
        tensor of exactly that size).  Returns the part of ``out`` that was written.  ``flac``: the s16 half of the chain alone."""
        if self.finished:
            # the library's own answer (FQ3_ESTATE, before any launch): the output count below has no meaning past the end
            if self._h:
                _lib.check(self._lib.fq3_audio_out_push(self._h, None, 0, 0, None, 0, C.byref(C.c_int64()), None))
            else:
                _lib.check(self._lib.fq3_tsm_push(self._tsm, None, 0, 0, None, 0, C.byref(C.c_int64()), None, 0, None))
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            x = self._empty if pcm is None else pcm.reshape(-1)
            if x.dtype != torch.float32 or x.device != self.dev or not x.is_contiguous():
                x = x.to(device=self.dev, dtype=torch.float32).contiguous()
            n = n_pushed = int(x.numel())
            mid_total, out_total = self._counts(self.n_in + n, final)
            n_mid, need = mid_total - self.n_mid, out_total - self.n_samples
            if out is None:
                out = torch.empty(need, dtype=self.dtype, device=self.dev)
            elif out.dtype != self.dtype or out.device != self.dev or not out.is_contiguous() or out.dim() != 1:
                raise ValueError("out must be a contiguous 1-D device tensor of the stage's dtype")
            cap = int(out.numel())
            wrote = C.c_int64()
            sp = C.c_void_p(s.cuda_stream)
            if self._tsm:
                if self._encode and need > cap:
                    raise ValueError(f"out has room for {cap} samples, this push completes {need}")
                mid = torch.empty(n_mid, dtype=torch.float32, device=self.dev) if self._encode else out
                mid_cap = int(mid.numel())
                _lib.check(self._lib.fq3_tsm_push(self._tsm, C.c_void_p(x.data_ptr() if n else None), n, 1 if final else 0,
                                                  C.c_void_p(mid.data_ptr() if mid_cap else None), mid_cap, C.byref(wrote), None, 0, sp))
                assert wrote.value == n_mid
                if n:
                    x.record_stream(s)
                x, n = mid, n_mid
            if self._encode:
                _lib.check(self._lib.fq3_audio_out_push(self._h, C.c_void_p(x.data_ptr() if n else None), n, 1 if final else 0,
                                                        C.c_void_p(out.data_ptr() if cap else None), cap, C.byref(wrote), sp))
                assert wrote.value == need
                if n:
                    x.record_stream(s)
        self.n_in += n_pushed
        self.n_mid, self.n_samples = mid_total, out_total
        if not self.flac:
            self.n_out = out_total
        self.finished = self.finished or bool(final)
        return out[:need]


# ---- a group of streams in one launch set (the lock-step batch) -----------------------------------------
GROUP_MAX = _lib.FQ3_STAGE_GROUP_MAX


class _Row:
    """one stage's share of a group push: its input, the counts its ``push`` would reach, and where its output lies in the buffer"""
    __slots__ = ("st", "x", "n", "final", "n_mid", "need", "mid_total", "out_total", "off", "mid_off", "flac_off", "flac_cap", "frames")


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def _call_group(fn, handles, ptrs, lens, finals, outs, caps, sp) -> list:
    """``fn`` = fq3_audio_out_push_group / fq3_tsm_push_group over up to GROUP_MAX rows per call -> the rows' counts"""
    got = []
    for i in range(0, len(handles), GROUP_MAX):
        j = min(len(handles), i + GROUP_MAX)
        B = j - i
        n_out = (C.c_int64 * B)()
        _lib.check(fn((C.c_void_p * B)(*handles[i:j]), B, (C.c_void_p * B)(*ptrs[i:j]), (C.c_int64 * B)(*lens[i:j]),
                      (C.c_int * B)(*finals[i:j]), (C.c_void_p * B)(*outs[i:j]), (C.c_int64 * B)(*caps[i:j]), n_out, sp))
        got.extend(int(v) for v in n_out)
    return got


def _push_group(stages, pcms, finals):
    """The launches of ``push_group``: -> (the uint8 device buffer every row's output lies in, the rows, the stream)."""
    if not (len(stages) == len(pcms) == len(finals)):
        raise ValueError("push_group: one pcm and one final flag per stage")
    if len(set(map(id, stages))) != len(stages):
        raise ValueError("push_group: the same stage twice in one call")
    if not stages:
        return None, [], None
    lib, dev, s = stages[0]._lib, stages[0].dev, stages[0]._stream()
    rows = []
    for st, pcm, final in zip(stages, pcms, finals):
        if st.dev != dev or st._stream().cuda_stream != s.cuda_stream:
            raise ValueError("push_group: the stages of one call share a device and a stream")
        if st.finished:
            st.push_into(None, False, None)                    # the library's own answer (FQ3_ESTATE), as ``push`` gives it
        r = _Row()
        r.st, r.final, r.x = st, bool(final), (st._empty if pcm is None else pcm.reshape(-1))
        rows.append(r)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        # buckets in order of first appearance: the rows of one resample + encode design, and the rows the time-scale stage writes itself
        buckets: dict = {}
        cursor = mid_cursor = 0
        for r in rows:
            st = r.st
            if r.x.dtype != torch.float32 or r.x.device != dev or not r.x.is_contiguous():
                r.x = r.x.to(device=dev, dtype=torch.float32).contiguous()
            r.n = int(r.x.numel())
            r.mid_total, r.out_total = st._counts(st.n_in + r.n, r.final)
            r.n_mid, r.need = r.mid_total - st.n_mid, r.out_total - st.n_samples
            key = (st.in_rate, st.out_rate, ENCODINGS[st.spec.encoding], st.zero) if st._encode else (st.in_rate,)
            buckets.setdefault(key, []).append(r)
            r.mid_off = None
            if st._tsm and st._encode:
                r.mid_off, mid_cursor = mid_cursor, mid_cursor + r.n_mid
        for members in buckets.values():
            cursor = _align(cursor, 16)
            for r in members:                                  # back to back: a row starts at whatever element offset it falls on
                r.off, cursor = cursor, cursor + r.need * r.st.dtype.itemsize
        for r in rows:
            r.flac_off = None
            if r.st.flac:
                st, before = r.st, r.st.n_samples
                r.frames = flac_count(st.out_rate, st.flac_block, r.out_total, r.final) - flac_count(st.out_rate, st.flac_block, before, False)
                r.flac_cap = r.frames * st.flac_bound
                cursor = _align(cursor, 8)
                r.flac_off, cursor = cursor, cursor + 8 + r.flac_cap
        buf = torch.empty(cursor, dtype=torch.uint8, device=dev)
        mid = torch.empty(mid_cursor, dtype=torch.float32, device=dev)
        base, mid_base, sp = buf.data_ptr(), mid.data_ptr(), C.c_void_p(s.cuda_stream)
        # one time-scale launch per in_rate over the rows with a speed ...
        by_rate: dict = {}
        for r in rows:
            if r.st._tsm:
                by_rate.setdefault(r.st.in_rate, []).append(r)
        for members in by_rate.values():
            outs = [(mid_base + 4 * r.mid_off if r.mid_off is not None else base + r.off) if r.n_mid else None for r in members]
            got = _call_group(lib.fq3_tsm_push_group, [r.st._tsm.value for r in members], [r.x.data_ptr() if r.n else None for r in members],
                              [r.n for r in members], [int(r.final) for r in members], outs, [r.n_mid for r in members], sp)
            assert got == [r.n_mid for r in members]
        # ... then one resample + encode launch per design
        for key, members in buckets.items():
            if len(key) == 1:
                continue
            ins = [((mid_base + 4 * r.mid_off, r.n_mid) if r.mid_off is not None else (r.x.data_ptr(), r.n)) for r in members]
            got = _call_group(lib.fq3_audio_out_push_group, [r.st._h.value for r in members], [p if n else None for p, n in ins],
                              [n for _p, n in ins], [int(r.final) for r in members], [base + r.off if r.need else None for r in members],
                              [r.need for r in members], sp)
            assert got == [r.need for r in members]
        # FLAC: the s16 samples of the flac rows of one (rate, block size) go through ONE launch pair, into this buffer as well: frame
        # sizes depend on the data, so every row has room for its frames at their bound, behind the 8-byte count the device fills in
        flac_buckets: dict = {}
        for r in rows:
            if r.flac_off is not None:
                flac_buckets.setdefault((r.st.out_rate, r.st.flac_block), []).append(r)
        for members in flac_buckets.values():
            for i in range(0, len(members), GROUP_MAX):
                part = members[i: i + GROUP_MAX]
                B = len(part)
                if B == 1:                                     # one row: the single push is the shorter way (3 us)
                    r, one = part[0], C.c_int64()
                    _lib.check(lib.fq3_flac_push(r.st._flac, C.c_void_p(base + r.off if r.need else None), r.need, int(r.final),
                                                 C.c_void_p(base + r.flac_off + 8 if r.flac_cap else None), r.flac_cap, C.byref(one),
                                                 C.c_void_p(base + r.flac_off), sp))
                    assert one.value == r.frames
                    continue
                got = (C.c_int64 * B)()
                _lib.check(lib.fq3_flac_push_group(
                    (C.c_void_p * B)(*[r.st._flac.value for r in part]), B, (C.c_void_p * B)(*[base + r.off if r.need else None for r in part]),
                    (C.c_int64 * B)(*[r.need for r in part]), (C.c_int * B)(*[int(r.final) for r in part]),
                    (C.c_void_p * B)(*[base + r.flac_off + 8 if r.flac_cap else None for r in part]), (C.c_int64 * B)(*[r.flac_cap for r in part]),
                    got, (C.c_void_p * B)(*[base + r.flac_off for r in part]), sp))
                assert list(got) == [r.frames for r in part]
        for r in rows:
            if r.n:
                r.x.record_stream(s)
            st = r.st
            st.n_in += r.n
            st.n_mid, st.n_samples = r.mid_total, r.out_total
            if not st.flac:
                st.n_out = r.out_total
            st.finished = st.finished or r.final
    return buf, rows, s


def push_group(stages, pcms, finals) -> list:
    """``[stages[i].push(pcms[i], finals[i]) for i]`` -- the same device tensors, bit for bit, and the same counters on every stage --
    with ONE time-scale launch for the rows that have a speed and ONE resample + encode launch per distinct (rates, encoding) instead
    of one or two launches per row (``fq3_tsm_push_group`` / ``fq3_audio_out_push_group``, up to 32 rows a call).  The stages share a
    device and a stream; ``pcms[i]`` is a float32 device vector or None.  All outputs lie in one device buffer, the rows of a design
    back to back.  The ``flac`` rows take their s16 half in the group launch and then ONE launch pair per (rate, block size)
    (``fq3_flac_push_group``; section 4.20; a lone row keeps its ``fq3_flac_push``); as in ``push``, reading how many bytes their frames took synchronises the stream (once
    for the call)."""
    buf, rows, s = _push_group(stages, pcms, finals)
    out = []
    lens = None
    if any(r.flac_off is not None for r in rows):
        with torch.cuda.stream(s):
            heads = torch.cat([buf[r.flac_off: r.flac_off + 8] for r in rows if r.flac_off is not None])
            lens = iter(heads.cpu().view(torch.int64).tolist())                                  # the one synchronisation
    for r in rows:
        if r.flac_off is not None:
            n = int(next(lens))
            r.st.n_out += n
            out.append(buf[r.flac_off + 8: r.flac_off + 8 + n])
        else:
            out.append(buf[r.off: r.off + r.need * r.st.dtype.itemsize].view(r.st.dtype))
    return out


class GroupCopy:
    """``push_group`` on its way to the host: every row of the call in ONE pinned buffer behind ONE copy.  ``rows()`` waits for the
    copy (the call's only synchronisation) and returns the rows as host arrays; the stages' byte counts of ``flac`` rows move then."""

    def __init__(self, stages, pcms, finals):
        buf, self._rows, s = _push_group(stages, pcms, finals)
        self.host = self.event = None
        if self._rows:
            with torch.cuda.stream(s):
                self.host = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=True)
                self.host.copy_(buf, non_blocking=True)
                self.event = torch.cuda.Event()
                self.event.record(s)
            self._buf = buf                                    # alive until the copy has run

    def rows(self) -> list:
        if self.event is not None:
            self.event.synchronize()
            self.event = self._buf = None
        out = []
        h = self.host.numpy() if self.host is not None else None
        for r in self._rows:
            if r.flac_off is not None:
                n = int(h[r.flac_off: r.flac_off + 8].view(np.int64)[0])
                if r.frames is not None:
                    r.st.n_out += n
                    r.frames = None                            # counted once, however often the rows are read
                out.append(h[r.flac_off + 8: r.flac_off + 8 + n])
            else:
                out.append(h[r.off: r.off + r.need * r.st.dtype.itemsize].view(NUMPY_DTYPES[r.st.spec.encoding]))
        return out


def push_group_host(stages, pcms, finals) -> list:
    """``push_group`` with the results on the host -- ``[stages[i].push_host(pcms[i], finals[i]) for i]`` -- all rows in one pinned
    copy and one synchronisation (``GroupCopy`` is the form that does not wait)."""
    return GroupCopy(stages, pcms, finals).rows()


def resample_device(audio: np.ndarray, sr: int, target_sr: int, device) -> np.ndarray:
    """``audio`` (host, mono) at ``sr`` -> float32 host array at ``target_sr`` through the device stage, in one shot."""
    a = np.array(audio, dtype=np.float32).reshape(-1)          # a copy: the caller's array may be read-only
    stage = AudioOut(AudioOutSpec(int(target_sr), "f32"), int(sr), device)
    return stage.push(torch.from_numpy(a).to(stage.dev), final=True).cpu().numpy()
