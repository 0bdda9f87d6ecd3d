"""A provenance watermark on the device (``fq3_mark_*``): a keyed spread-spectrum mark in the 516 .. 3469 Hz
band of a float32 stream at 24 kHz, and its detector.  Length-preserving; the marked stream does not depend on how it was cut into
pushes, bit for bit.  Both run as DFT-as-GEMM on the fp32 matrix cores; there is no CPU fallback.

``design``      the constants and the chip rows of a key (``fq3_mark_design``; no GPU needed)
``count``       output samples that exist after ``n_in`` input samples (``fq3_mark_count``; no GPU needed)
``Watermark``   one stream on a device: ``push`` / ``flush`` / ``reset``
``detect``      ``Detection(z, offset, phase, present)`` of a signal at any rate for a key
``scan``        which sliding windows of one or many clips carry the mark (``fq3_mark_scan``, section 4.23): a ``Scan`` per clip"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

RATE = 24000
N, H, PERIOD, N_OFFSETS, OFFSET_STEP = 512, 256, 128, 32, 8
STRENGTH_RANGE = (0.02, 0.3)
THRESHOLD = 6.0          # 4096 hypotheses x Q(6.0): about 4e-6 false positives per clip


def _key(key) -> int:
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 64:
        raise ValueError(f"key must be an integer in [0, 2^64), not {key!r}")
    return int(key)


def _strength(strength) -> float:
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) \
            or not (float(strength) == 0.0 or STRENGTH_RANGE[0] <= float(strength) <= STRENGTH_RANGE[1]):
        raise ValueError(f"strength must be 0 (the identity) or a number in [{STRENGTH_RANGE[0]}, {STRENGTH_RANGE[1]}], not {strength!r}")
    return float(strength)


@dataclass(frozen=True)
class MarkSpec:
    """What ``FasterQwen3TTS.watermark`` keeps: the 64-bit ``key`` and the ``strength`` a (the mark is ``a`` times the band, about
    ``20 log10(a)`` dB below the voice in that band).  0.1 is NOT tuned on real voices."""
    key: int
    strength: float = 0.1

    def __post_init__(self):
        _key(self.key)
        _strength(self.strength)


def design(key: int, strength: float = 0.1):
    """``fq3_mark_design`` (host only): -> (a as the device's float32, the chip rows as int8 [128][64] of -1 / +1)."""
    lib = _lib.load()
    a, words = C.c_float(), (C.c_uint32 * (2 * PERIOD))()
    if lib.fq3_mark_design(_key(key), float(strength), None, None, None, None, None, C.byref(a), words) != 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    w = np.frombuffer(words, dtype=np.uint32).reshape(PERIOD, 2)
    j = np.arange(64)
    return np.float32(a.value), (((w[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(np.int8) * 2 - 1)


def count(n_in: int, final: bool) -> int:
    """``fq3_mark_count``: ``n_in`` when ``final``, else ``max(0, n_in // 256 - 1) * 256``."""
    lib = _lib.load()
    n = lib.fq3_mark_count(int(n_in), 1 if final else 0)
    if n < 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return int(n)


def _device(device) -> torch.device:
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type != "cuda":
        raise ValueError("the watermark runs on the GPU; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


class Watermark:
    """One stream through the mark.  ``push(pcm)`` takes the next float32 samples (a device tensor) and returns the samples that
    became final -- ``count(total so far) - count(before)`` of them, a device tensor, one launch, nothing synchronises;
    ``push(..., final=True)`` or ``flush()`` ends the stream and hands out what was held back (between 256 and 511 samples).
    ``reset()`` starts a new stream on the same object.  Work is enqueued on ``stream`` (default: the current stream)."""

    def __init__(self, key: int, strength: float = 0.1, device="cuda", stream=None):
        self.spec = MarkSpec(_key(key), _strength(strength))
        self.dev = _device(device)
        self.stream = stream
        self._lib = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.MarkConfig(self.spec.key, self.spec.strength)
        with torch.cuda.device(self.dev):
            _lib.check(self._lib.fq3_mark_create(C.byref(cfg), C.byref(self._h)))
        self.n_in, self.n_out, self.finished = 0, 0, False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.fq3_mark_destroy(h)

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def reset(self) -> None:
        _lib.check(self._lib.fq3_mark_reset(self._h, C.c_void_p(self._stream().cuda_stream)))
        self.n_in, self.n_out, self.finished = 0, 0, False

    def push(self, pcm: Optional[torch.Tensor], final: bool = False) -> torch.Tensor:
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            x = None if pcm is None else pcm.reshape(-1)
            if x is not None and (x.dtype != torch.float32 or x.device != self.dev or not x.is_contiguous()):
                x = x.to(device=self.dev, dtype=torch.float32).contiguous()
            n = 0 if x is None else int(x.numel())
            total = self.n_in + n
            room = max((total if final else max(0, total // H - 1) * H) - self.n_out, 0)
            out = torch.empty(room, dtype=torch.float32, device=self.dev)
            got = C.c_int64()
            _lib.check(self._lib.fq3_mark_push(self._h, C.c_void_p(x.data_ptr() if n else None), n, 1 if final else 0,
                                               C.c_void_p(out.data_ptr() if room else None), room, C.byref(got), C.c_void_p(s.cuda_stream)))
            if n:
                x.record_stream(s)
            out.record_stream(s)
        self.n_in = total
        self.n_out += int(got.value)
        self.finished = self.finished or bool(final)
        return out[:got.value]

    def flush(self) -> torch.Tensor:
        """ends the stream: the held-back samples"""
        return self.push(None, final=True)


GROUP_MAX = _lib.FQ3_STAGE_GROUP_MAX


def _push_group(marks, pcms, finals):
    """The launches of ``push_group``: -> (the float32 device buffer every row's output lies in, [(offset, count)] per row)."""
    from .leveller import _float_rows, _group_members
    marks, pcms, finals = list(marks), list(pcms), [bool(f) for f in finals]
    dev, s = _group_members("watermark.push_group", marks, pcms, finals)
    if dev is None:
        return None, []
    lib = marks[0]._lib
    with torch.cuda.device(dev), torch.cuda.stream(s):
        rows = _float_rows(pcms, dev)
        cursor, spans = 0, []
        for m, (x, n), final in zip(marks, rows, finals):
            if m.finished:
                m.push(x, final)                                   # the library's own answer (FQ3_ESTATE), as ``push`` gives it
            room = max(count(m.n_in + n, final) - m.n_out, 0)
            spans.append((cursor, room))                           # back to back: a row starts at whatever float offset it falls on
            cursor += room
        buf = torch.empty(cursor, dtype=torch.float32, device=dev)
        base, sp = buf.data_ptr(), C.c_void_p(s.cuda_stream)
        for a in range(0, len(marks), GROUP_MAX):
            part = range(a, min(a + GROUP_MAX, len(marks)))
            B = len(part)
            n_out = (C.c_int64 * B)()
            _lib.check(lib.fq3_mark_push_group(
                (C.c_void_p * B)(*[marks[i]._h.value for i in part]), B,
                (C.c_void_p * B)(*[rows[i][0].data_ptr() if rows[i][1] else None for i in part]),
                (C.c_int64 * B)(*[rows[i][1] for i in part]), (C.c_int * B)(*[int(finals[i]) for i in part]),
                (C.c_void_p * B)(*[base + 4 * spans[i][0] if spans[i][1] else None for i in part]),
                (C.c_int64 * B)(*[spans[i][1] for i in part]), n_out, sp))
            for i, got in zip(part, n_out):
                assert int(got) == spans[i][1]
                marks[i].n_in += rows[i][1]
                marks[i].n_out += int(got)
                marks[i].finished = marks[i].finished or finals[i]
        for x, n in rows:
            if n:
                x.record_stream(s)
        buf.record_stream(s)
    return buf, spans


def push_group(marks, pcms, finals) -> list:
    """``[marks[i].push(pcms[i], finals[i]) for i]`` -- the same device tensors, bit for bit, and the same counters on every object
    -- with ONE launch per 32 rows instead of one per row (``fq3_mark_push_group``).  Rows may differ in key and strength.  The
    objects share a device and a stream and appear once.  All rows' outputs lie back to back, in row order, in ONE float32 device
    buffer, and the results are views of it (``_push_group`` hands out the buffer and the rows' places in it)."""
    buf, spans = _push_group(marks, pcms, finals)
    return [buf[off:off + cnt] for off, cnt in spans]


@dataclass(frozen=True)
class Detection:
    """``z``: the largest detector statistic over 32 sample offsets and 128 frame phases; ``offset`` (samples, a multiple of 8) and
    ``phase`` where it was found; ``present``: ``z >= 6.0``."""
    z: float
    offset: int
    phase: int
    present: bool


def detect_table(pcm, rate: int, key: int, device="cuda") -> torch.Tensor:
    """The detector's whole table ``z[32][128]`` (a device tensor): two launches on the current stream.  ``pcm``: a mono signal, a
    tensor or an array; at another rate than 24 kHz it goes through ``audio_out.resample_device`` first."""
    dev = _device(pcm.device if isinstance(pcm, torch.Tensor) and pcm.is_cuda else device)
    lib, key = _lib.load(), _key(key)
    with torch.cuda.device(dev):
        if int(rate) != RATE:
            from .audio_out import resample_device
            pcm = resample_device(pcm.detach().cpu().numpy() if isinstance(pcm, torch.Tensor) else pcm, int(rate), RATE, dev)
        x = torch.as_tensor(np.asarray(pcm, dtype=np.float32) if not isinstance(pcm, torch.Tensor) else pcm)
        x = x.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        n = int(x.numel())
        need = lib.fq3_mark_detect_workspace(n)
        if need < 0:
            raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
        work = torch.empty(int(need), dtype=torch.float32, device=dev)
        z = torch.empty((N_OFFSETS, PERIOD), dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream(dev)
        _lib.check(lib.fq3_mark_detect(C.c_void_p(x.data_ptr()), n, key, C.c_void_p(work.data_ptr()), int(need), C.c_void_p(z.data_ptr()),
                                       C.c_void_p(s.cuda_stream)))
        for t in (x, work, z):
            t.record_stream(s)
    return z


def detect(pcm, rate: int, key: int, device="cuda") -> Detection:
    """Is the mark of ``key`` in ``pcm``?  One copy brings the table to the host."""
    z = detect_table(pcm, rate, key, device).cpu().numpy()
    oi, ph = np.unravel_index(int(np.argmax(z)), z.shape)
    return Detection(float(z[oi, ph]), int(oi) * OFFSET_STEP, int(ph), bool(z[oi, ph] >= THRESHOLD))


BLOCK = 16 * H           # samples of a scan block: 16 frames, 171 ms
SCAN_MAX = _lib.FQ3_STAGE_GROUP_MAX
_WINDOW = np.dtype([("z", np.float32), ("offset", np.int32), ("phase", np.int32), ("present", np.int32)])


@dataclass(frozen=True)
class Scan:
    """The windows of one clip: arrays of length ``W``.  ``z`` the largest statistic of window ``w``, ``offset`` / ``phase`` where it
    was found (the phase is the clip's: frames count from the clip's start in every window), ``present``: ``z >= 6.0`` -- per window
    the false-positive estimate of ``THRESHOLD`` holds, so a clip of ``W`` windows has about ``W`` times it; ``start_s`` / ``end_s``
    the window's span in seconds of the 24 kHz signal; ``window_s`` / ``hop_s`` as rounded to whole blocks; ``tables`` the device
    tensor ``[W][32][128]`` when asked for."""
    z: np.ndarray
    offset: np.ndarray
    phase: np.ndarray
    present: np.ndarray
    start_s: np.ndarray
    end_s: np.ndarray
    window_s: float
    hop_s: float
    tables: Optional[torch.Tensor] = None


def scan_blocks(window_s: float, hop_s: float):
    """seconds -> (win_blocks, hop_blocks): rounded to whole blocks of 4096 samples, 1 <= hop <= win <= 4096"""
    win = min(max(int(round(float(window_s) * RATE / BLOCK)), 1), 4096)
    return win, min(max(int(round(float(hop_s) * RATE / BLOCK)), 1), win)


def scan_windows(n: int, win_blocks: int, hop_blocks: int) -> int:
    """``fq3_mark_scan_windows`` (host only): the windows of a clip of ``n`` samples"""
    lib = _lib.load()
    w = lib.fq3_mark_scan_windows(int(n), int(win_blocks), int(hop_blocks))
    if w < 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return int(w)


def _at_rate(pcm, rate: int, dev) -> torch.Tensor:
    if int(rate) != RATE:
        from .audio_out import resample_device
        pcm = resample_device(pcm.detach().cpu().numpy() if isinstance(pcm, torch.Tensor) else pcm, int(rate), RATE, dev)
    x = torch.as_tensor(np.asarray(pcm, dtype=np.float32) if not isinstance(pcm, torch.Tensor) else pcm)
    return x.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()


def scan_blocks_device(xs, keys, win_blocks: int, hop_blocks: int, tables: bool = False):
    """One ``fq3_mark_scan`` call (two launches on the current stream, nothing synchronises) over up to 32 float32 device tensors at
    24 kHz.  -> (the windows' records as a device uint8 tensor ``[sum W * 16]``, the device tables ``[sum W][32][128]`` or None, the
    list of ``W``)."""
    lib, B, dev = _lib.load(), len(xs), xs[0].device
    ns = (C.c_int64 * B)(*[int(x.numel()) for x in xs])
    ks = (C.c_uint64 * B)(*[_key(k) for k in keys])
    ptrs = (C.c_void_p * B)(*[x.data_ptr() for x in xs])
    ws = [scan_windows(int(n), win_blocks, hop_blocks) for n in ns]
    with torch.cuda.device(dev):
        need = lib.fq3_mark_scan_workspace(B, ns)
        if need < 0:
            raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
        work = torch.empty(int(need), dtype=torch.float64, device=dev)
        out = torch.empty(sum(ws) * _WINDOW.itemsize, dtype=torch.uint8, device=dev)
        tab = torch.empty((sum(ws), N_OFFSETS, PERIOD), dtype=torch.float32, device=dev) if tables else None
        s = torch.cuda.current_stream(dev)
        _lib.check(lib.fq3_mark_scan(B, ptrs, ns, ks, int(win_blocks), int(hop_blocks), C.c_void_p(work.data_ptr()), int(need),
                                     C.c_void_p(out.data_ptr()), C.c_void_p(tab.data_ptr() if tables else None), C.c_void_p(s.cuda_stream)))
        for t in list(xs) + [work, out] + ([tab] if tables else []):
            t.record_stream(s)
    return out, tab, ws


def scan(clips, rate, key, window_s: float = 3.0, hop_s: float = 1.0, tables: bool = False, device="cuda"):
    """WHICH PARTS of the clips carry the mark: the detector over sliding windows of ``window_s`` seconds every ``hop_s`` seconds (both
    rounded to whole blocks of 171 ms; a clip shorter than the window is one window), all clips of a call in two launches and one pinned
    copy.  ``clips``: one mono signal or a list of them (tensors or arrays); ``rate`` and ``key``: one for all, or one per clip.  More
    than 32 clips run in consecutive calls of 32.  -> one ``Scan`` for a single signal, else a list of them."""
    single = not isinstance(clips, (list, tuple))
    clips = [clips] if single else list(clips)
    rates = list(rate) if isinstance(rate, (list, tuple)) else [rate] * len(clips)
    keys = list(key) if isinstance(key, (list, tuple)) else [key] * len(clips)
    if not clips or len(rates) != len(clips) or len(keys) != len(clips):
        raise ValueError("scan: one rate and one key for all clips, or one per clip")
    first = clips[0]
    dev = _device(first.device if isinstance(first, torch.Tensor) and first.is_cuda else device)
    win, hop = scan_blocks(window_s, hop_s)
    result = []
    with torch.cuda.device(dev):
        for at in range(0, len(clips), SCAN_MAX):
            xs = [_at_rate(c, r, dev) for c, r in zip(clips[at:at + SCAN_MAX], rates[at:at + SCAN_MAX])]
            out, tab, ws = scan_blocks_device(xs, keys[at:at + SCAN_MAX], win, hop, tables)
            host = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(out, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            rec, w0 = host.numpy().view(_WINDOW), 0
            for x, w in zip(xs, ws):
                nb = -(-(-(-int(x.numel()) // H) - 1) // 16)                   # NB = ceil((T - 2) / 16), T = ceil(n / H) + 1
                start = np.minimum(np.arange(w) * hop, max(nb - win, 0))
                end = np.minimum((start + min(win, nb)) * BLOCK, int(x.numel()))
                r = rec[w0:w0 + w]
                result.append(Scan(r["z"].copy(), r["offset"].copy(), r["phase"].copy(), r["present"] != 0, start * BLOCK / RATE, end / RATE,
                                   win * BLOCK / RATE, hop * BLOCK / RATE, tab[w0:w0 + w] if tables else None))
                w0 += w
    return result[0] if single else result
