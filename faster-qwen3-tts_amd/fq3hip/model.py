"""``FasterQwen3TTS``: the reference's public API (``faster_qwen3_tts/model.py``) over the MI355X HIP path.

Same constructor arguments, method names, argument order, defaults, return types and error
behaviour as the reference wrapper (pinned there by ``tests/test_voice_clone_prompt_api.py`` and
``tests/test_sample_rate.py``; mirrored here by ``tests/test_api_contract.py``), so callers switch by
changing the import.  What changed underneath: ``predictor_graph`` / ``talker_graph`` are HIP-backed
objects sharing one ``libfq3hip`` context, ``speech_tokenizer`` is the HIP codec decoder, and the
decode loop state lives on the GPU.
"""
from __future__ import annotations

import contextlib
import logging
import time
from pathlib import Path
from typing import Any, Dict, Generator, List, Optional, Tuple, Union

import numpy as np
import torch

from .loudness import LoudnessSession
from .stream_groups import StreamGroups, runs_of, window_plan

logger = logging.getLogger(__name__)

_GGML_ONLY = ("ref_spk", "ref_rvq", "ref_spk_emb", "ref_codes")


def expand_seeds(seeds, n: int) -> list:
    """``generate.expand_seeds`` (the ``seeds=`` keyword of the batch entry points), imported when first needed like the decode loops."""
    from .generate import expand_seeds as expand
    return expand(seeds, n)


def _to_numpy(a) -> np.ndarray:
    if hasattr(a, "cpu"):
        return a.flatten().float().cpu().numpy()
    return a.flatten() if hasattr(a, "flatten") else a


class _Encoded:
    """One utterance of a ``_SideVocoder`` group that went through the output stage: row ``index`` of the group's one pinned copy."""

    def __init__(self, copy, index: int, stage, give):
        self.copy, self.index, self.stage, self.give = copy, index, stage, give

    def array(self) -> np.ndarray:
        """the encoded utterance (waits for the copy); ``flac``: the whole file, its header carries the sample count"""
        a, st = self.copy.rows()[self.index], self.stage
        if st.flac:
            a = np.concatenate([np.frombuffer(st.header(st.n_samples), dtype=np.uint8), a])
        else:
            a = a.copy()
        self.give(st)
        return a


class _SideVocoder:
    """Non-streaming vocoding of whole utterances off the decode stream (batched generation): ``submit`` enqueues the codec
    decode + the device-to-pinned-host copy on a side stream after the codes are ready, ``collect`` waits and returns the
    waveforms in submission order.  Tokenizers without ``decode_tensor`` (a foreign ``speech_tokenizer``) are decoded
    synchronously through the upstream call."""

    def __init__(self, tok, device, stream=None):
        self.tok = tok
        self.sample_rate = int(getattr(tok, "sample_rate", 24000))
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        self.async_ok = torch.cuda.is_available() and hasattr(tok, "decode_tensor")
        if self.async_ok and stream is None:
            from .streams import concurrent_stream
            stream = concurrent_stream(self.dev)               # verified to run beside the decode stream (fq3hip/streams.py)
        self.stream = stream if self.async_ok else None
        self.items: list = []
        self.device_only = False          # long form: the waveforms stay on the device (``collect_device``), no pinned-host copies
        self.level = None                 # ``level(key, waveform)``: the model's loudness / fixed-gain step, run between the decode and the copy
        # ``output=`` of the batch entry points: {key: AudioOutSpec} of the utterances whose waveform goes through the output stage
        # behind ``level`` -- the utterances vocoded together in ONE ``audio_out.push_group`` -- and the model's ``(take, give)`` of
        # pooled stages
        self.outputs, self.stages = None, None

    def _spec(self, key):
        return self.outputs.get(key) if self.outputs else None

    def _encode_group(self, keys, pcms) -> list:
        """whole utterances (float32 device vectors) through pooled output stages, one ``push_group`` with ``final`` for all of them
        -> one ``_Encoded`` per key: its host array exists once the group's one pinned copy has landed"""
        from .audio_out import GroupCopy
        take, give = self.stages
        stages = [take(self.outputs[k], self.stream) for k in keys]
        copy = GroupCopy(stages, [p.flatten() for p in pcms], [True] * len(keys))
        return [_Encoded(copy, i, st, give) for i, st in enumerate(stages)]

    def _prefix(self, ref):
        """the tokenizer's cached front-end state of an ICL reference (built on the vocoder stream), or None"""
        if ref is None or not hasattr(self.tok, "prefix_for"):
            return None
        return self.tok.prefix_for(ref, self.stream)

    def submit(self, key, codes: torch.Tensor, ref_len: int = 0, ref=None) -> None:
        """``ref_len`` > 0: the first ``ref_len`` frames are the ICL reference; only the waveform after their share
        (``int(ref_len / T * n_samples)``, model.py:927-930) is produced.  ``ref``: that reference's own tensor (its cached
        front-end state then serves every utterance of the voice)."""
        if not self.async_ok or not hasattr(self.tok, "num_samples_total"):
            lst, _rate = self.tok.decode({"audio_codes": codes.unsqueeze(0)})
            a = _to_numpy(lst[0])
            a = a[int(ref_len / max(codes.shape[0], 1) * len(a)):] if ref_len > 0 else a
            if self.level is not None:
                a = _to_numpy(self.level(key, a))
            if self._spec(key) is not None:
                # synchronous tokenizer: its audio is on the host; the utterance is uploaded for the stage
                a = self._encode_group([key], [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)])[0]
            self.items.append((key, a, None, None))
            return
        cut = int(ref_len / max(codes.shape[0], 1) * self.tok.num_samples_total(codes.shape[0])) if ref_len > 0 else 0
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        codes.record_stream(self.stream)
        pf = self._prefix(ref) if ref_len > 0 else None
        with torch.cuda.stream(self.stream):
            pcm = self.tok.decode_tensor(codes, cut, prefix=pf) if pf is not None else self.tok.decode_tensor(codes, cut)
            if self.level is not None:
                pcm = self.level(key, pcm)
            host = None
            if self._spec(key) is not None:
                host = self._encode_group([key], [pcm])[0]
            elif not self.device_only:
                host = torch.empty(pcm.shape, dtype=torch.float32, pin_memory=True)
                host.copy_(pcm, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.items.append((key, host, ev, pcm))          # pcm kept alive until its copy has completed

    MAX_GROUP = 16          # utterances per batched codec launch set (the workspace grows with it; the gain saturates well before)
    STREAM_GROUP = 32       # streaming CHUNKS per launch set (short inputs: 178-202 frames behind a reference, 33 in phase 2): measured per chunk
                            # 0.42 / 0.35 / 0.31 ms at 16 / 32 / 64 (profiles/r06_codec_time_bf16x2_groups.txt); 32 keeps the workspace at ~17 GB

    def add(self, key, codes: torch.Tensor, ref_len: int = 0, more: int = 0, ref=None) -> None:
        """Grouped form of ``submit``: utterances that finished in the same poll of the lock-step decode (``more`` = how many more of
        that poll follow, ``timing["more_in_poll"]``) are held back and vocoded TOGETHER -- utterances of equal length through one
        batched launch set (``decode_tensor_batch``: the [B, T, 16] form of the vocoder interface, model.py:924)."""
        self._held = getattr(self, "_held", [])
        self._held.append((key, codes, ref_len, ref))
        if more <= 0:
            held, self._held = self._held, []
            self.submit_many(held)

    def add_flush(self) -> None:
        held, self._held = getattr(self, "_held", []), []
        if held:
            self.submit_many(held)

    def submit_many(self, group) -> None:
        if not self.async_ok or not hasattr(self.tok, "decode_tensor_batch") or not hasattr(self.tok, "num_samples_total"):
            for key, codes, ref_len, ref in group:
                self.submit(key, codes, ref_len, ref)
            return
        classes: Dict[Any, list] = {}
        for key, codes, ref_len, ref in group:
            classes.setdefault((int(codes.shape[0]), int(ref_len)), []).append((key, codes, ref))
        for (T, ref_len), members in classes.items():
            for i in range(0, len(members), self.MAX_GROUP):
                part = members[i:i + self.MAX_GROUP]
                if len(part) == 1:
                    self.submit(part[0][0], part[0][1], ref_len, part[0][2])
                    continue
                cut = int(ref_len / max(T, 1) * self.tok.num_samples_total(T)) if ref_len > 0 else 0
                self.stream.wait_stream(torch.cuda.current_stream(self.dev))
                for _k, c, _r in part:
                    c.record_stream(self.stream)
                pfs = [self._prefix(r) for _k, _c, r in part] if ref_len > 0 else None
                if pfs is not None and any(p is None for p in pfs):
                    pfs = None
                with torch.cuda.stream(self.stream):
                    stacked = torch.stack([c for _k, c, _r in part])
                    pcm = self.tok.decode_tensor_batch(stacked, cut, prefixes=pfs) if pfs is not None else self.tok.decode_tensor_batch(stacked, cut)
                    if self.level is not None:
                        pcm = pcm.float().contiguous()
                        for j, (key, _c, _r) in enumerate(part):
                            self.level(key, pcm[j])                 # row by row, in place: every utterance has its own gain
                    host = None
                    staged = [j for j, (key, _c, _r) in enumerate(part) if self._spec(key) is not None]
                    enc = dict(zip(staged, self._encode_group([part[j][0] for j in staged], [pcm[j] for j in staged]))) if staged else {}
                    if not self.device_only and len(staged) < len(part):
                        host = torch.empty(pcm.shape, dtype=torch.float32, pin_memory=True)
                        host.copy_(pcm, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                for j, (key, _c, _r) in enumerate(part):
                    self.items.append((key, enc[j] if j in enc else host[j] if host is not None else None, ev, pcm[j]))

    # ---- incremental (exact) vocoding of utterances that are still decoding ------------------------------------------------
    # The codec decoder is causal: decode(codes[:p]) is bit for bit the prefix of decode(codes), and a tail decode from sample s is
    # the tail of the full decode.  So the waveform of a running utterance can be produced in slices -- every ``inc`` frames the
    # samples that became final, by ``decode_tensor_batch(codes so far, first_sample = samples already produced)`` -- on the side
    # stream, under the lock-step decode of the following frames, and across all lanes that reached the boundary together as ONE
    # batched launch set.  What is left when the utterance ends is the last slice, not the whole waveform.  The concatenation
    # is exactly ``decode_tensor(ref + codes)[cut:]``; the reference's cut of an ICL waveform (``int(ref_len / T * n_samples)``,
    # model.py:927-930) depends on the final length T, so slices start at a lower bound of it and the few samples in front of
    # the real cut are dropped at the end.
    def _cut_floor(self, ref_len: int, max_total: int) -> int:
        if ref_len <= 0:
            return 0
        key = (ref_len, max_total)
        cache = self.__dict__.setdefault("_cut_cache", {})
        if key not in cache:
            cache[key] = min(int(ref_len / T * self.tok.num_samples_total(T)) for T in range(ref_len + 1, max(ref_len + 2, max_total + 1)))
        return cache[key]

    def inc_add(self, key, chunk, ref_codes, ready_event, final: bool, more: int, max_new: int) -> None:
        """``chunk``: the frames of utterance ``key`` that completed since the last call (LongTensor[n, 16] on the device, or None / empty).
        ``final``: the utterance is over.  ``more``: events of the same poll still to come (the slice is decoded when it reaches 0)."""
        inc = self.__dict__.setdefault("_inc", {})
        st = inc.get(key)
        if st is None:
            ref_len = int(ref_codes.shape[0]) if ref_codes is not None else 0
            st = inc[key] = dict(ref=ref_codes, ref_len=ref_len, chunks=[], T=0, done=0, parts=[], final=False,
                                 floor=self._cut_floor(ref_len, ref_len + int(max_new)))
        if chunk is not None and chunk.shape[0] > 0:
            chunk.record_stream(self.stream)
            st["chunks"].append(chunk)
            st["T"] += int(chunk.shape[0])
            self.__dict__.setdefault("_inc_held", []).append((key, ready_event))
        st["final"] = st["final"] or bool(final)
        if more <= 0:
            self.inc_flush()

    def inc_flush(self) -> None:
        held, self._inc_held = self.__dict__.get("_inc_held", []), []
        if not held:
            return
        main = torch.cuda.current_stream(self.dev)
        jobs, seen = {}, set()
        for key, ev in held:
            if ev is not None:
                self.stream.wait_event(ev)
            else:
                self.stream.wait_stream(main)
            if key in seen:
                continue
            seen.add(key)
            st = self._inc[key]
            T = st["ref_len"] + st["T"]
            first = st["floor"] + st["done"]
            n = self.tok.num_samples_total(T)
            if first < n:
                jobs.setdefault((T, first), []).append((key, st, n))
        with torch.cuda.stream(self.stream):
            for (T, first), members in jobs.items():
                for i in range(0, len(members), self.MAX_GROUP):
                    part = members[i:i + self.MAX_GROUP]
                    fulls = [torch.cat(([st["ref"].to(st["chunks"][0].device)] if st["ref"] is not None else []) + st["chunks"], dim=0)
                             for _k, st, _n in part]
                    if len(part) == 1:
                        pcm = self.tok.decode_tensor(fulls[0], first).unsqueeze(0)
                    else:
                        pcm = self.tok.decode_tensor_batch(torch.stack(fulls), first)
                    host = torch.empty(pcm.shape, dtype=torch.float32, pin_memory=True)
                    host.copy_(pcm, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                    for j, (_k, st, n) in enumerate(part):
                        st["parts"].append((host[j], ev, pcm))
                        st["done"] = n - st["floor"]

    def inc_collect(self):
        """-> (key, waveform) of every utterance handed to ``inc_add``, in first-seen order (waits for the side stream)."""
        self.inc_flush()
        inc, self._inc = self.__dict__.get("_inc", {}), {}
        for key, st in inc.items():
            if not st["parts"]:
                yield key, np.zeros(1, dtype=np.float32)
                continue
            rows = []
            for host, ev, _pcm in st["parts"]:
                ev.synchronize()
                rows.append(host.numpy())
            a = np.concatenate(rows) if len(rows) > 1 else rows[0].copy()
            T = st["ref_len"] + st["T"]
            cut = int(st["ref_len"] / max(T, 1) * self.tok.num_samples_total(T)) if st["ref_len"] > 0 else 0
            yield key, a[cut - st["floor"]:]

    def collect(self):
        for key, host, ev, _pcm in self.items:
            if isinstance(host, _Encoded):
                yield key, host.array()
            elif ev is None:
                yield key, host
            else:
                ev.synchronize()
                yield key, host.numpy().copy()
        self.items = []

    def collect_device(self):
        """``device_only``: -> (key, waveform) in submission order, the waveform a float32 tensor still on the device, valid on
        ``self.stream`` without a wait (a host array for a tokenizer that is decoded synchronously)."""
        for key, host, ev, pcm in self.items:
            yield key, (host if ev is None else pcm.flatten().float())
        self.items = []


class StreamingVocoder:
    """The reference's streaming windowing (``faster_qwen3_tts/model.py:1048-1137``) as a state machine over code chunks:
    phase 1 re-decodes everything (reference codes in front) until >= max(25, chunk) frames exist and calibrates samples
    per frame; phase 2 decodes [25 context frames + the new chunk] and drops the context.  With the HIP tokenizer only the
    samples that are kept are produced (``decode_tensor(codes, first_sample)``: bit-identical to slicing the full decode)
    and the codec runs on ``side_stream`` so that it overlaps the next frames' decode kernels.

    ``output`` (an ``AudioOutSpec``; default None: float32 at the model's rate, through the code below unchanged): every chunk's
    waveform goes through the device output stage (``fq3hip/audio_out.py``) on the vocoder's stream before it is copied to the host,
    and the rate handed back with a chunk is the output rate.  The stage holds back its look-ahead (about 16 * max(1, in / out) input
    samples; with a ``speed`` other than 1 the time-scale stage in front of it adds about 30 ms of input, three hops of 10 ms, and
    hands out whole 10 ms segments) until ``push(..., final=True)`` or ``flush()``.  With the ``flac`` encoding the chunks are
    ``uint8`` arrays that concatenate to a complete FLAC stream: the first begins with the 42-byte header, and the samples behind the
    last whole FLAC block (up to 48 ms at 24 kHz) wait for the final push as well.

    ``exact=True`` (opt-in; the default stays the reference's windowing): no windowing at all -- the utterance owns a codec stream
    state and a chunk's audio is that push's samples, so the chunks concatenate to the one-pass decode of all the codes at any chunk
    size (see ``_init_exact``).  ``push`` / ``prepare`` / ``flush`` keep their signatures; the output stage sits behind it unchanged.

    ``gain`` / ``limiter`` (``FasterQwen3TTS.fixed_gain`` / ``limiter``): the chunk is multiplied and then limited on the vocoder's
    stream, in front of the output stage.  The limiter holds back ``A + 6`` samples of the stream; ``push(..., final=True)`` or
    ``flush()`` hands them out, with or without an ``output``.  ``leveller`` (``FasterQwen3TTS.leveller``): the streaming loudness
    leveller (``fq3hip/leveller.py``) between the two; it holds nothing back and does not limit."""

    CONTEXT_FRAMES = 25

    def __init__(self, tok, ref_codes, chunk_size: int, device, side_stream=None, output=None, exact=False, gain=None, limiter=None,
                 limiter_pool=None, leveller=None, leveller_pool=None, leveller_hops: int = 0):
        self.tok, self.ref_codes, self.side = tok, ref_codes, side_stream
        self.output, self.stage, self.header_sent = output, None, False
        self.gain = gain                  # a 1-element float32 device tensor (``FasterQwen3TTS.fixed_gain``) or None
        # a ``LimiterSpec`` (``FasterQwen3TTS.limiter``) or None; the stage, taken at the first chunk and given back at the last;
        # ``limiter_pool``: a list the model keeps per (device, stream, spec) -- idle ``Limiter`` objects of finished utterances
        self.limit_spec, self.limit, self.limit_pool = limiter, None, limiter_pool
        # a ``LevelSpec`` (``FasterQwen3TTS.leveller``) or None; its stage and pool likewise, between the gain and the limiter
        # (the pool holds objects of ``leveller.pooled``: the initial gain is set per stream); ``leveller_hops``: the capacity a new
        # object gets (0: 4096 hops); ``level_stats``: the device report of the utterance's leveller once its stream has ended;
        # ``on_level``: a caller's hook (the server's worker keeps the voice-memory callback of its request here)
        self.level_spec, self.level, self.level_pool, self.level_hops = leveller, None, leveller_pool, int(leveller_hops)
        self.level_stats, self.on_level = None, None
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        self.exact = bool(exact)
        if self.exact:
            self._init_exact()
            return
        self.min_cal = max(self.CONTEXT_FRAMES, int(chunk_size))
        self.all_codes: List[torch.Tensor] = []
        self.prev_len, self.spf = 0, None
        # phase 1 decodes ``ref_codes + everything so far`` for every chunk: with the tokenizer's cached front-end state of the
        # reference (built once per voice, on the vocoder stream) only the rows behind it are computed -- bit-identical
        self.prefix = (tok.prefix_for(ref_codes, side_stream) if side_stream is not None and ref_codes is not None and hasattr(tok, "prefix_for")
                       else None)
        self.last_prefix = None          # the prefix the decode returned by the last ``prepare`` may use (None in phase 2)

    # ---- exact mode (``exact=True``) ------------------------------------------------------------------------------
    # The utterance owns one codec stream state (``tok.stream_open``) that moves forward with every chunk: a chunk's audio is that
    # push's samples, so the chunks concatenate, sample for sample, to the ONE-PASS decode of all the codes -- at any chunk size.  No
    # phase 1 / phase 2, no calibrated samples-per-frame, no concatenation of the codes so far.
    # ICL: the non-streaming cut ``int(ref_len / T * n)`` depends on the final length T, so the stream begins at ``c0``, its lower bound
    # over every total length of a one-pass decode (T <= CHUNK_FRAMES; beyond that the non-streaming output is piecewise anyway), and
    # drops the ``c0 - num_samples(ref_len)`` samples in front of it from its first push: the non-streaming waveform is the stream from
    # sample ``cut - c0`` on.
    def _init_exact(self):
        tok, rc = self.tok, self.ref_codes
        if not hasattr(tok, "stream_open") or not hasattr(tok, "stream_push"):
            raise ValueError("exact streaming needs a speech tokenizer with codec stream states (stream_open / stream_push)")
        self.prefix = self.last_prefix = None
        ref_len = int(rc.shape[0]) if rc is not None else 0
        self.c0 = 0
        if ref_len > 0:
            cache = tok.__dict__.setdefault("_exact_c0", {})
            if ref_len not in cache:
                cache[ref_len] = _SideVocoder._cut_floor(self, ref_len, int(getattr(tok, "CHUNK_FRAMES", 300)))
            self.c0 = cache[ref_len]
        self.cstream = tok.stream_open(rc if ref_len > 0 else None, self.side)
        self.frames = ref_len                                     # frames handed to the stream so far (prepared pushes included)
        self.drop = max(0, self.c0 - self._samples_upto(ref_len)) if ref_len > 0 else 0

    def _samples_upto(self, frames: int) -> int:
        """samples of the one-pass decode that belong to the first ``frames`` frames"""
        if hasattr(self.tok, "stream_samples"):
            return self.tok.stream_samples(0, frames)
        return self.tok.num_samples_total(frames)

    def _prepare_exact(self, chunk):
        """-> (the new frames, samples to drop from the front of their push); the push itself is the caller's (``tok.stream_push`` on
        ``self.cstream``, alone or with other utterances of the same class ``(min(frames_before, ctx_max), n_new)``)"""
        if self.side is not None:
            chunk.record_stream(self.side)
        drop, self.drop = self.drop, 0
        self.frames_before, self.frames = self.frames, self.frames + int(chunk.shape[0])
        return chunk, drop

    def _push_exact(self, chunk, ev, final):
        codes, drop = self._prepare_exact(chunk)
        if self.side is not None:
            if ev is not None:
                self.side.wait_event(ev)
            else:
                self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with (contextlib.nullcontext() if self.side is None else torch.cuda.stream(self.side)):
            wav = self.tok.stream_push([self.cstream], codes.unsqueeze(0))[0]
            wav = wav[drop:]              # (the drop is below one frame's samples: the trims of the transposed convs add up to less)
            wav = self._gained(wav, final)
            if self.output is not None:
                return self._encoded(wav.flatten().float(), final)
            out = _to_numpy(wav)
        return out, int(getattr(self.tok, "sample_rate", 24000))

    def _gained(self, wav, final: bool = False):
        """``wav`` (device tensor, on the vocoder's stream) times the fixed gain, through the leveller and then through the limiter,
        in front of the output stage; without any: ``wav``.  The limiter holds back its look-ahead (``A + 6`` samples) until ``final``
        or ``flush()``."""
        if self.gain is not None:
            from .loudness import apply_gain
            wav = apply_gain(wav.flatten().float().contiguous(), self.gain, self.side)
        if self.level_spec is not None:
            wav = self.level_push(wav.flatten().float().contiguous(), final)
        if self.limit_spec is not None:
            wav = self.limit_push(wav.flatten().float().contiguous(), final)
        return wav

    LIMITER_POOL_MAX = 256

    def limit_take(self):
        """This utterance's limiter, taken at the first chunk: an idle one from the model's pool, reset, or a new one -- on the
        vocoder's stream (without one, the current stream).  ``limit_release`` is the other half."""
        if self.limit is None:
            try:
                lim = self.limit_pool.pop() if self.limit_pool else None        # (another thread may take the last one first)
            except IndexError:
                lim = None
            if lim is not None and lim.stream is self.side and lim.dev == (self.dev if self.dev.index is not None else torch.device("cuda", torch.cuda.current_device())) and lim.spec == self.limit_spec:
                lim.reset()
                self.limit = lim
            else:
                from .limiter import Limiter
                self.limit = Limiter(self.limit_spec, int(getattr(self.tok, "sample_rate", 24000)), self.dev, self.side)
        return self.limit

    def limit_release(self) -> None:
        """the utterance's limiter (if it has one) goes back to the pool behind its final push: its device buffers are then reused by
        a later utterance on the same stream instead of being allocated and freed per reply (a free synchronises the device while
        other lanes run)"""
        lim, self.limit = self.limit, None
        if lim is not None and self.limit_pool is not None and len(self.limit_pool) < self.LIMITER_POOL_MAX:
            self.limit_pool.append(lim)

    def limit_push(self, wav, final: bool):
        """``wav`` (contiguous float32 device vector, or None) through this utterance's limiter (``limit_take``); with the final push
        the object goes back (``limit_release``)."""
        out = self.limit_take().push(wav, final)
        if final:
            self.limit_release()
        return out

    def level_take(self):
        """This utterance's leveller, taken at the first chunk as the limiter is (``limit_take``): a pooled object is reset to this
        stream's initial gain.  ``level_release`` is the other half."""
        if self.level is None:
            try:
                lev = self.level_pool.pop() if self.level_pool else None        # (another thread may take the last one first)
            except IndexError:
                lev = None
            dev = self.dev if self.dev.index is not None else torch.device("cuda", torch.cuda.current_device())
            if (lev is not None and lev.stream is self.side and lev.dev == dev and lev.spec.pooled == self.level_spec.pooled
                    and lev.capacity_hops >= self.level_hops):
                lev.reset(self.level_spec.initial_gain_db)          # one kept object, whatever gain the stream starts from
                self.level = lev
            else:
                from .leveller import Leveller
                self.level = Leveller(self.level_spec, int(getattr(self.tok, "sample_rate", 24000)), self.dev, self.side,
                                      capacity_hops=self.level_hops)
        return self.level

    def level_push(self, wav, final: bool, out=None):
        """``wav`` (contiguous float32 device vector) through this utterance's leveller on the vocoder's stream: as many samples come
        back (into ``out``, if given).  The object is taken and given back as the limiter's is (``limit_push``)."""
        y = self.level_take().push(wav, final, out=out)
        if final:
            self.level_release()
        return y

    def level_release(self) -> None:
        """the utterance's leveller (if it has one) goes back to the pool: its stream has ended, with or without a final push"""
        lev, self.level = self.level, None
        if lev is not None:
            self.level_stats = lev.stats_buffer()                  # the newest gains stay readable (``level_gain_db``), on the device
            if self.level_pool is not None and len(self.level_pool) < self.LIMITER_POOL_MAX:
                self.level_pool.append(lev)

    @property
    def level_gain_db(self):
        """After the utterance: the leveller's last target in dB, None when it never measured one (or there was no leveller); waits
        for the vocoder's stream."""
        if self.level_stats is None:
            return None
        from .leveller import LevelStats
        with (contextlib.nullcontext() if self.side is None else torch.cuda.stream(self.side)):
            st = LevelStats.from_bytes(self.level_stats.cpu().numpy().tobytes())
        return st.target_gain_db if st.valid else None

    def level_report_async(self):
        """After the utterance: ``(pinned host bytes, event)`` of the leveller's report -- the copy is queued on the vocoder's stream
        and the event marks it, so a caller that may not wait (the server's scheduler thread) reads it once ``event.query()`` says so
        (``level_gain_of``); None without a report."""
        if self.level_stats is None:
            return None
        with (contextlib.nullcontext() if self.side is None else torch.cuda.stream(self.side)):
            host = torch.empty(self.level_stats.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(self.level_stats, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.side if self.side is not None else torch.cuda.current_stream(self.dev))
        return host, ev

    @staticmethod
    def level_gain_of(host) -> Optional[float]:
        """the last target in dB of a landed ``level_report_async`` copy, None when it never measured one"""
        from .leveller import LevelStats
        st = LevelStats.from_bytes(host.numpy().tobytes())
        return st.target_gain_db if st.valid else None

    def _stage(self):
        """the output stage of this utterance, made at its first chunk (on the vocoder's stream; without one, on the current stream)"""
        if self.stage is None:
            from .audio_out import AudioOut
            self.stage = AudioOut(self.output, int(getattr(self.tok, "sample_rate", 24000)), self.dev, self.side)
        return self.stage

    def _encoded(self, wav, final: bool):
        """``wav`` (device tensor, or None for the tail alone) through the output stage -> (host array, output rate)"""
        st = self._stage()
        with (contextlib.nullcontext() if self.side is None else torch.cuda.stream(self.side)):
            out = st.push_host(wav, final)
        if st.flac and not self.header_sent:
            # a FLAC stream: the utterance's first chunk starts with the stream header (length unknown); the chunks are bytes
            out, self.header_sent = np.concatenate([np.frombuffer(st.header(), dtype=np.uint8), out]), True
        return out, st.out_rate

    def flush(self):
        """With an ``output``: ends the stage's stream and returns ``(tail, rate)`` -- the samples it held back as look-ahead -- for an
        utterance whose last event carried no codes.  Empty after a ``push(..., final=True)``, and without an ``output``.  With a
        ``limiter``: ends its stream as well; the ``A + 6`` samples it held back come out (through the ``output`` stage, if any)."""
        if self.level is not None:
            with (contextlib.nullcontext() if self.side is None else torch.cuda.stream(self.side)):
                self.level_release()                                # (it held nothing back)
        if self.limit is not None:
            # the limiter's held-back samples: they go out through the output stage, or as they are
            with (contextlib.nullcontext() if self.side is None else torch.cuda.stream(self.side)):
                tail = self.limit_push(None, True)
                if self.output is None:
                    return tail.cpu().numpy(), int(getattr(self.tok, "sample_rate", 24000))
            return self._encoded(tail, True)
        if self.output is None:
            return np.zeros(0, dtype=np.float32), int(getattr(self.tok, "sample_rate", 24000))
        st = self._stage()
        if st.finished:
            from .audio_out import NUMPY_DTYPES
            return np.zeros(0, dtype=NUMPY_DTYPES[self.output.encoding]), st.out_rate
        return self._encoded(None, True)

    def _vocode(self, codes_in, first_sample, ev, prefix=None, final=False):
        """waveform[first_sample:] of codes_in (host array).  On the side stream an ``output`` stage runs here, before the copy."""
        if self.side is None:
            lst, rate = self.tok.decode({"audio_codes": codes_in.unsqueeze(0)})
            return _to_numpy(lst[0])[first_sample:], rate
        if ev is not None:
            self.side.wait_event(ev)
        else:
            self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            # (.cpu() synchronises the side stream only)
            wav = self.tok.decode_tensor(codes_in, first_sample, prefix=prefix) if prefix is not None else self.tok.decode_tensor(codes_in, first_sample)
            wav = self._gained(wav, final)
            if self.output is not None:
                return self._encoded(wav.flatten().float(), final)
            out = _to_numpy(wav)
        return out, self.tok.sample_rate

    def _ref_on(self, device):
        """The reference codes on ``device``.  A host tensor is uploaded ONCE per tensor object and device (noted on the object: the
        streams of one voice share the prompt's tensor), not once per chunk of every stream (a synchronous copy each)."""
        rc = self.ref_codes
        if rc.device == device:
            return rc
        note = getattr(rc, "fq3_on_device", None)
        if not (isinstance(note, tuple) and note[0] == device and (note[2] is None or (not rc.is_inference() and note[2] == rc._version))):
            note = (device, rc.to(device), None if rc.is_inference() else rc._version)
            try:
                rc.fq3_on_device = note
            except Exception:
                pass
        return note[1]

    def _cat(self, parts, ev):
        if self.side is None:
            return torch.cat(parts, dim=0)
        with torch.cuda.stream(self.side):
            if ev is not None:
                self.side.wait_event(ev)
            else:
                self.side.wait_stream(torch.cuda.current_stream(self.dev))
            return torch.cat(parts, dim=0)

    def prepare(self, chunk: torch.Tensor, ready_event=None):
        """Side-stream form of ``push`` in two halves: advances the windowing state by ``chunk`` and returns ``(codes_in,
        first_sample)`` -- the decode whose ``waveform[first_sample:]`` is this chunk's audio -- so that a caller with several
        utterances at the same point (the first chunks of lock-step lanes) can run those decodes as ONE batched launch set."""
        assert self.side is not None
        if self.exact:
            return self._prepare_exact(chunk)
        chunk.record_stream(self.side)
        self.all_codes.append(chunk)
        n_new = chunk.shape[0]
        flat = self._cat(self.all_codes, ready_event)
        n_total = flat.shape[0]
        rc = self.ref_codes
        ref_len = rc.shape[0] if rc is not None else 0
        start, n_in, first, self.prev_len, self.spf = window_plan(n_total, n_new, ref_len, self.prev_len, self.spf, self.min_cal,
                                                                  self.CONTEXT_FRAMES, self.tok.num_samples_total)
        if start is None:
            inp = self._cat([self._ref_on(flat.device), flat], ready_event) if rc is not None else flat
            self.last_prefix = self.prefix if ref_len else None
        else:
            inp = flat[start:]
            self.last_prefix = None
        assert inp.shape[0] == n_in
        return inp, first

    def push(self, chunk: torch.Tensor, ready_event=None, final=False):
        """``chunk`` LongTensor[n_new, 16] (device) -> (new audio as a host array, sample_rate).  ``final`` (only read with an
        ``output`` or a ``limiter``): this is the utterance's last chunk, the tail those stages held back comes with it."""
        if self.exact:
            return self._push_exact(chunk, ready_event, final)
        if self.side is not None:
            inp, first = self.prepare(chunk, ready_event)
            return self._vocode(inp, first, ready_event, self.last_prefix, final)
        self.all_codes.append(chunk)
        n_new = chunk.shape[0]
        flat = self._cat(self.all_codes, ready_event)
        n_total = flat.shape[0]
        if self.spf is None:
            rc = self.ref_codes
            inp = self._cat([self._ref_on(flat.device), flat], ready_event) if rc is not None else flat
            ref_len = rc.shape[0] if rc is not None else 0
            if self.side is not None:
                # model.py:1095-1100 without materialising what is thrown away: audio[cut:][prev_len:]
                n_audio = self.tok.num_samples_total(inp.shape[0])
                cut = int(ref_len / max(inp.shape[0], 1) * n_audio) if ref_len else 0
                new_audio, sr = self._vocode(inp, cut + self.prev_len, ready_event)
                gen_len = n_audio - cut
            else:
                audio, sr = self._vocode(inp, 0, ready_event)
                if ref_len:
                    audio = audio[int(ref_len / max(inp.shape[0], 1) * len(audio)):]
                new_audio = audio[self.prev_len:]
                gen_len = len(audio)
            self.prev_len = gen_len
            if n_total >= self.min_cal:
                self.spf = gen_len / n_total
        else:
            start = max(0, n_total - n_new - self.CONTEXT_FRAMES)
            window = flat[start:]
            n_ctx = window.shape[0] - n_new
            new_audio, sr = self._vocode(window, int(round(n_ctx * self.spf)) if n_ctx > 0 else 0, ready_event)
        if self.gain is not None or self.limit_spec is not None or self.level_spec is not None:
            # synchronous tokenizer: its audio is on the host; the chunk is uploaded for the multiply (and the stages behind it)
            wav = self._gained(torch.from_numpy(np.ascontiguousarray(new_audio, dtype=np.float32)).to(self.dev), final)
            return self._encoded(wav, final) if self.output is not None else (wav.cpu().numpy(), sr)
        if self.output is not None:
            # synchronous tokenizer: its audio is on the host; the chunk is uploaded for the stage
            return self._encoded(torch.from_numpy(np.ascontiguousarray(new_audio, dtype=np.float32)).to(self.dev), final)
        return new_audio, sr


class FasterQwen3TTS:
    """Qwen3-TTS with a hipGraph-captured, hand-written HIP decode path (drop-in for the CUDA-graph wrapper)."""

    def __init__(self, base_model, predictor_graph, talker_graph, device: str = "cuda",
                 dtype: torch.dtype = torch.bfloat16, max_seq_len: int = 2048):
        self.model = base_model
        self.predictor_graph = predictor_graph
        self.talker_graph = talker_graph
        self.device = device
        self.dtype = dtype
        self.max_seq_len = max_seq_len
        self.sample_rate = self._infer_sample_rate(base_model)
        self._warmed_up = False
        self._voice_prompt_cache: Dict[Any, Any] = {}
        self._audio_spec = None          # the AudioOutSpec of an open ``audio_output`` context
        self._loud = None                # the LoudnessSession of an open ``loudness`` context
        self._gain = None                # the factor of an open ``fixed_gain`` context
        self._limit = None               # the LimiterSpec of an open ``limiter`` context
        self._lvl = None                 # the LevelSpec of an open ``leveller`` context
        self._last_levelled = None       # the vocoder / leveller of the last levelled stream (``last_level_gain_db``)
        self._seed = None                # the sampling seed of an open ``seeded`` context

    # ---- small helpers pinned by the reference's unit tests ------------------------------------------------
    @staticmethod
    def _get_speech_tokenizer(base_model):
        return getattr(getattr(base_model, "model", None), "speech_tokenizer", None)

    @property
    def speech_tokenizer(self):
        tok = self._get_speech_tokenizer(self.model)
        if tok is None:
            raise AttributeError("Underlying model does not expose a speech_tokenizer")
        return tok

    @staticmethod
    def _infer_sample_rate(base_model) -> int:
        """speech_tokenizer.sample_rate, then base_model.sample_rate, then 24000 (model.py:59-84)."""
        rate = None
        tok = FasterQwen3TTS._get_speech_tokenizer(base_model)
        if tok is not None:
            rate = getattr(tok, "sample_rate", None)
        if rate is None:
            rate = getattr(base_model, "sample_rate", None)
        if rate is None:
            logger.warning("Could not infer sample rate from base model; defaulting to 24000 Hz.")
            return 24000
        return int(rate)

    @staticmethod
    def _resolve_non_streaming_mode(non_streaming_mode: Optional[bool], *, default: bool) -> bool:
        return default if non_streaming_mode is None else non_streaming_mode

    @staticmethod
    def _reject_ggml_cached_reference_args(ref_spk=None, ref_rvq=None, ref_spk_emb=None, ref_codes=None) -> None:
        if any(v is not None for v in (ref_spk, ref_rvq, ref_spk_emb, ref_codes)):
            raise NotImplementedError(
                "ref_spk/ref_rvq cached qwentts.cpp references require backend='ggml'. "
                "Use voice_clone_prompt for precomputed prompts with the torch backend.")

    # ---- construction ---------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, model_name: str, device: str = "cuda", dtype: Union[str, torch.dtype] = torch.bfloat16,
                        attn_implementation: str = "sdpa", max_seq_len: int = 2048, backend: str = "torch",
                        quant: str = "BF16", gguf_talker_path: Optional[Union[str, Path]] = None,
                        gguf_codec_path: Optional[Union[str, Path]] = None,
                        qwentts_library_path: Optional[Union[str, Path]] = None, qwentts_use_fa: bool = True,
                        qwentts_clamp_fp16: bool = False, qwentts_ref_cache_dir: Optional[Union[str, Path]] = None,
                        cache_dir: Optional[Union[str, Path]] = None, local_files_only: bool = False,
                        codec_precision: Optional[str] = None):
        """Load a local Qwen3-TTS checkpoint directory and build the HIP decode context.

        ``backend`` keeps the reference's vocabulary: ``"torch"`` (the default) selects the graph-captured
        fast path -- here the HIP one; ``"ggml"``/``"qwentts"`` name the external qwentts.cpp runtime, which
        has no ROCm build in this repository.  ``attn_implementation`` is accepted for compatibility (the
        HIP attention kernel is the only implementation)."""
        if backend not in ("torch", "ggml", "qwentts"):
            raise ValueError(f"Unsupported backend {backend!r}. Expected 'torch', 'ggml', or 'qwentts'.")
        if backend in ("ggml", "qwentts"):
            raise NotImplementedError("the qwentts.cpp (GGML) backend is not part of the MI355X build; use backend='torch'")
        if isinstance(dtype, str):
            dtype = getattr(torch, dtype)
        if not device.startswith("cuda") or not torch.cuda.is_available():
            raise ValueError("CUDA graphs require CUDA device")       # same message as the reference (model.py:181-182)
        from .weights import load_hf_checkpoint
        import os
        path = str(model_name)
        if not os.path.isdir(path):
            raise FileNotFoundError(
                f"{model_name!r} is not a local checkpoint directory; this build has no network access "
                "(HF_HUB_OFFLINE) -- download the model and pass its path.")
        cfg, weights = load_hf_checkpoint(path, dtype=dtype, device="cpu")
        tokenizer = None
        try:
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(path, local_files_only=True)
        except Exception as e:      # tokenizer files are optional for code-only workflows
            logger.warning("no text tokenizer loaded from %s (%s)", path, e)
        return cls.from_weights(cfg, weights, device=device, dtype=dtype, max_seq_len=max_seq_len, tokenizer=tokenizer,
                                codec_precision=codec_precision)

    @classmethod
    def from_weights(cls, cfg, weights, device: str = "cuda", dtype: torch.dtype = torch.bfloat16,
                     max_seq_len: int = 2048, tokenizer=None, codec_max_frames: int = 1024, max_frames: int = 2048,
                     share: Optional["FasterQwen3TTS"] = None, codec_precision: Optional[str] = None):
        """Build from an in-memory weight table (real or seeded synthetic, ``fq3hip.weights``).
        ``share``: an existing model on the same GPU whose weight replica this instance borrows -- one
        instance (decode context + codec workspace) per concurrently running utterance.
        ``codec_precision``: ``None`` = model dtype, ``"fp32"`` = high-precision vocoder (see ``NativeQwen3TTS``)."""
        if not str(device).startswith("cuda") or not torch.cuda.is_available():
            raise ValueError("CUDA graphs require CUDA device")
        from .native_model import NativeQwen3TTS
        from .predictor_graph import PredictorGraph
        from .talker_graph import TalkerGraph
        base = NativeQwen3TTS(cfg, weights, device=device, dtype=dtype, max_seq_len=max_seq_len, tokenizer=tokenizer,
                              codec_max_frames=codec_max_frames, max_frames=max_frames,
                              share=share.model if share is not None else None, codec_precision=codec_precision)
        pg = PredictorGraph(base.engine, do_sample=True, top_k=50, temperature=0.9)      # model.py:209-218
        tg = TalkerGraph(base.engine)
        return cls(base_model=base, predictor_graph=pg, talker_graph=tg, device=device, dtype=dtype,
                   max_seq_len=max_seq_len)

    def warmup(self, prefill_len: int = 100) -> None:
        """Capture the decode hipGraph once (idempotent, model.py:239-252)."""
        if self._warmed_up:
            return
        self.predictor_graph.capture(num_warmup=3)
        self.talker_graph.capture(prefill_len=prefill_len, num_warmup=3)
        self._warmed_up = True

    def _warmup(self, prefill_len: int) -> None:
        self.warmup(prefill_len=prefill_len)

    # ---- prefix KV cache (opt-in) -----------------------------------------------------------------------------------
    def enable_prefix_cache(self, capacity_rows: int, min_rows: Optional[int] = None, batch: bool = False):
        """Keep the talker K/V rows of instruct turns (voice design, custom voice with an instruct) on the device, up to
        ``capacity_rows`` rows, and prefill only the rest of a prompt whose instruct is cached (``fq3hip/prefix_cache.py``).
        ``batch=False``: the cache of the single-stream entry points (``generate_*``, ``generate_*_streaming``, ``stream_*``), carried by
        the model's engine.  ``batch=True``: the cache of the ``*_batch`` entry points and the batch scheduler
        (``BatchDecoder(prefix_cache=...)``: packed groups go through ``PrefixCache.prefill_pack``); it is a cache of its own, because
        the scheduler prefills on a stream of its own, and the single-stream entry points never see it.  Both may be on.  Returns the
        :class:`PrefixCache`."""
        from .prefix_cache import DEFAULT_BATCH_MIN_ROWS, PrefixCache
        eng = self.talker_graph.engine
        if batch:
            self.disable_prefix_cache(batch=True)
            self._batch_prefix_cache = PrefixCache(eng, capacity_rows, DEFAULT_BATCH_MIN_ROWS if min_rows is None else min_rows)
            eng.prefix_split = True           # the prompt builder projects the instruct ids on their own (prompt.py)
            cached = getattr(self, "_batch_cache", None)
            if cached is not None:
                cached[1].prefix_cache = self._batch_prefix_cache
            return self._batch_prefix_cache
        self.disable_prefix_cache()
        eng.prefix_cache = PrefixCache(eng, capacity_rows, min_rows)
        return eng.prefix_cache

    def disable_prefix_cache(self, batch: bool = False) -> None:
        eng = self.talker_graph.engine
        if batch:
            cache = getattr(self, "_batch_prefix_cache", None)
            self._batch_prefix_cache = None
            eng.prefix_split = False
            cached = getattr(self, "_batch_cache", None)
            if cached is not None:
                cached[1].prefix_cache = None
            if cache is not None:
                if torch.cuda.is_available():
                    torch.cuda.synchronize(eng.device)                    # the scheduler's prefill stream has run the last copies
                cache.close()
            return
        cache = getattr(eng, "prefix_cache", None)
        eng.prefix_cache = None
        if cache is not None:
            torch.cuda.current_stream(eng.device).synchronize()      # the last request's copies out of the entries have run
            cache.close()

    def generate(self, text: str, language: str = "English", max_new_tokens: int = 2048, temperature: float = 0.9,
                 top_k: int = 50, do_sample: bool = True, repetition_penalty: float = 1.05) -> Tuple[list, int]:
        raise NotImplementedError("Default voice generation not yet implemented. "
                                  "Use generate_voice_clone() with reference audio.")

    # ---- voice-clone prompt resolution (model.py:295-463) -------------------------------------------------------
    def _resolve_voice_clone_prompt(self, input_ids, ref_audio, ref_text: str, xvec_only: bool, append_silence: bool,
                                    voice_clone_prompt):
        if voice_clone_prompt is not None:
            return self._resolve_precomputed_voice_clone_prompt(input_ids=input_ids, ref_text=ref_text,
                                                                voice_clone_prompt=voice_clone_prompt)
        if ref_audio is None:
            raise ValueError("ref_audio is required when voice_clone_prompt is not provided")
        return self._resolve_voice_clone_prompt_from_reference(input_ids=input_ids, ref_audio=ref_audio,
                                                               ref_text=ref_text, xvec_only=xvec_only,
                                                               append_silence=append_silence)

    def _ref_ids(self, text: str):
        return self.model._tokenize_texts([self.model._build_ref_text(text)])[0]

    def _resolve_precomputed_voice_clone_prompt(self, input_ids, ref_text: str, voice_clone_prompt):
        n = len(input_ids)
        if isinstance(voice_clone_prompt, list):
            if len(voice_clone_prompt) != n:
                raise ValueError(f"voice_clone_prompt must have length {n}, got {len(voice_clone_prompt)}")
            vcp = self.model._prompt_items_to_voice_clone_prompt(voice_clone_prompt)
            ref_ids = []
            for item in voice_clone_prompt:
                if bool(item.icl_mode):
                    text = item.ref_text if item.ref_text else ref_text
                    if not text:
                        raise ValueError("ref_text is required when voice_clone_prompt uses ICL mode.")
                    ref_ids.append(self._ref_ids(text))
                else:
                    ref_ids.append(None)
            return vcp, ref_ids, any(vcp["icl_mode"])
        missing = [k for k in ("ref_spk_embedding",) if k not in voice_clone_prompt]
        if missing:
            raise ValueError(f"voice_clone_prompt missing required keys: {missing}. Expected keys: ['ref_spk_embedding']")
        for key in ("ref_spk_embedding", "x_vector_only_mode", "icl_mode", "ref_code"):
            if key in voice_clone_prompt:
                v = voice_clone_prompt[key]
                if not isinstance(v, list) or len(v) != n:
                    raise ValueError(f"voice_clone_prompt[{key!r}] must be a list with length {n}")
        xvec = voice_clone_prompt.get("x_vector_only_mode", [True] * n)
        if "icl_mode" in voice_clone_prompt:
            icl = [bool(v) for v in voice_clone_prompt["icl_mode"]]
            for i, (a, b) in enumerate(zip(xvec, icl)):
                if bool(a) == bool(b):
                    raise ValueError(f"voice_clone_prompt has inconsistent mode flags at index {i}: "
                                     "x_vector_only_mode and icl_mode must be opposites")
        else:
            icl = [not bool(v) for v in xvec]
        codes = voice_clone_prompt.get("ref_code", [None] * n)
        for i, (a, b, c) in enumerate(zip(xvec, icl, codes)):
            if bool(a) and c is not None:
                raise ValueError(f"voice_clone_prompt index {i}: ref_code must be None in x_vector_only mode")
            if bool(b) and c is None:
                raise ValueError(f"voice_clone_prompt index {i}: ref_code is required in ICL mode")
        vcp = dict(ref_code=codes, ref_spk_embedding=voice_clone_prompt["ref_spk_embedding"],
                   x_vector_only_mode=[bool(v) for v in xvec], icl_mode=[bool(v) for v in icl])
        using_icl = any(vcp["icl_mode"])
        if using_icl:
            if not ref_text:
                raise ValueError("ref_text is required when voice_clone_prompt uses ICL mode.")
            rid = self._ref_ids(ref_text)
            ref_ids = [rid if f else None for f in vcp["icl_mode"]]
        else:
            ref_ids = [None] * n
        return vcp, ref_ids, using_icl

    def _load_ref_audio_with_silence(self, ref_audio, silence_secs: float = 0.5):
        """model.py:278-293.  ``soundfile`` when it is installed, otherwise the standard-library WAV reader."""
        from .audio_io import load_audio
        audio, sr = load_audio(ref_audio)
        if silence_secs > 0:
            audio = np.concatenate([audio, np.zeros(int(silence_secs * sr), dtype=np.float32)])
        return audio, sr

    def set_voice_ref_cache(self, directory) -> None:
        """Serve ``ref_audio=...`` calls from an on-disk cache of precomputed voice-clone prompts (``fq3hip/voice_cache.py``;
        the role the reference's ``qwentts_ref_cache_dir`` plays for its GGML backend, ``ggml_backend.py:403-471``)."""
        from .voice_cache import VoiceRefCache
        self._voice_ref_cache = VoiceRefCache(directory) if directory else None

    def _voice_cache_entry(self, ref_audio, xvec_only: bool, append_silence: bool):
        """(audio at 24 kHz, key, metadata) of a reference clip: ONE construction for lookups and stores (same loader, same
        resampler, the request's mode in the metadata), so that what is written is what is found."""
        from .audio_io import resample
        from .voice_cache import cache_key
        silence = 0.5 if (append_silence and not xvec_only) else 0.0
        audio, sr = self._load_ref_audio_with_silence(ref_audio, silence_secs=silence)
        audio = resample(audio, sr, 24000)
        ident = f"{getattr(self.model.model, 'tts_model_type', 'base')}-{getattr(self.model.model, 'tts_model_size', '')}"
        key, meta = cache_key(audio, append_silence=silence > 0, model_identity=ident, mode="xvec" if xvec_only else "icl")
        return audio, key, meta, silence > 0, ident

    def _cached_voice_prompt(self, ref_audio, ref_text: str, xvec_only: bool, append_silence: bool):
        cache = getattr(self, "_voice_ref_cache", None)
        if cache is None:
            return None
        _audio, key, meta, _sil, _ident = self._voice_cache_entry(ref_audio, xvec_only, append_silence)
        hit = cache.load(key, meta)
        if hit is None or (not xvec_only and hit["ref_code"] is None):      # an entry without codes cannot serve an ICL request
            return None
        spk = torch.from_numpy(hit["ref_spk_embedding"])
        if xvec_only:
            return dict(ref_code=[None], ref_spk_embedding=[spk], x_vector_only_mode=[True], icl_mode=[False]), None
        return (dict(ref_code=[torch.from_numpy(hit["ref_code"])], ref_spk_embedding=[spk], x_vector_only_mode=[False],
                     icl_mode=[True]), hit["ref_text"] or ref_text)

    def _store_voice_prompt(self, ref_audio, item, xvec_only: bool, append_silence: bool) -> None:
        """Write a freshly analysed reference through to the on-disk cache (when one is set), so that the next process
        serves it without running the analysers (the reference's GGML backend does the same, ggml_backend.py:448-465)."""
        cache = getattr(self, "_voice_ref_cache", None)
        if cache is None:
            return
        from .voice_cache import export_voice_clone_prompt
        audio, _key, _meta, sil, ident = self._voice_cache_entry(ref_audio, xvec_only, append_silence)
        export_voice_clone_prompt(cache, audio, item, append_silence=sil, model_identity=ident,
                                  ref_text=getattr(item, "ref_text", None) or "")

    def _resolve_voice_clone_prompt_from_reference(self, input_ids, ref_audio, ref_text: str, xvec_only: bool,
                                                   append_silence: bool):
        using_icl = not xvec_only
        key = (str(ref_audio), ref_text, xvec_only, append_silence)
        if key in self._voice_prompt_cache:
            vcp, ref_ids = self._voice_prompt_cache[key]
            return vcp, ref_ids, using_icl
        cached = self._cached_voice_prompt(ref_audio, ref_text, xvec_only, append_silence)
        if cached is not None:
            vcp, rt = cached
            using_icl = bool(vcp["icl_mode"][0])
            if using_icl and not rt:
                raise ValueError("ref_text is required when voice_clone_prompt uses ICL mode.")
            ref_ids = [self._ref_ids(rt) if using_icl else None]
        elif xvec_only:
            items = self.model.create_voice_clone_prompt(ref_audio=str(ref_audio), ref_text="", x_vector_only_mode=True)
            vcp = dict(ref_code=[None], ref_spk_embedding=[items[0].ref_spk_embedding], x_vector_only_mode=[True],
                       icl_mode=[False])
            ref_ids = [None] * len(input_ids)
            self._store_voice_prompt(ref_audio, items[0], xvec_only, append_silence)
        else:
            audio = self._load_ref_audio_with_silence(ref_audio, silence_secs=0.5 if append_silence else 0.0)
            items = self.model.create_voice_clone_prompt(ref_audio=audio, ref_text=ref_text)
            vcp = self.model._prompt_items_to_voice_clone_prompt(items)
            rt = items[0].ref_text
            ref_ids = [self._ref_ids(rt) if rt else None]
            self._store_voice_prompt(ref_audio, items[0], xvec_only, append_silence)
        self._voice_prompt_cache[key] = (vcp, ref_ids)
        return vcp, ref_ids, using_icl

    # ---- prompt assembly (host glue; layout = SURVEY.md Appendix B / model.py:583-805) --------------------------
    def _build_talker_inputs_local(self, m, input_ids, ref_ids, voice_clone_prompt, languages, speakers,
                                   non_streaming_mode: bool, instruct_ids=None):
        tk, tc, mc = m.talker, m.config.talker_config, m.config
        if len(input_ids) == 1 and getattr(tk, "hip_prompt_ready", False):
            # native model: the whole prompt is three launches of HIP arithmetic (fq3hip/prompt.py); the tensor-op
            # version below is kept for foreign `m` objects (an upstream qwen-tts model) and for batches
            from .prompt import build_talker_inputs_hip
            vcp = voice_clone_prompt
            return build_talker_inputs_hip(m, input_ids[0], ref_ids[0] if ref_ids else None, vcp, 0, languages[0],
                                           speakers[0] if speakers is not None else None, non_streaming_mode,
                                           instruct_ids[0] if instruct_ids is not None else None)
        dev = tk.device
        emb_c = tk.get_input_embeddings()
        text = lambda ids: tk.text_projection(tk.get_text_embeddings()(ids))
        ids_t = lambda rows: torch.tensor(rows, device=dev, dtype=torch.long)
        spk_embeds = m.generate_speaker_prompt(voice_clone_prompt) if voice_clone_prompt is not None else None
        speakers = speakers if speakers is not None else [None] * len(input_ids)
        seqs, trailing, pad = [], [], None
        for i, (iid, lang, spk) in enumerate(zip(input_ids, languages, speakers)):
            parts = []
            if instruct_ids is not None and instruct_ids[i] is not None:
                parts.append(text(instruct_ids[i]))
            if spk_embeds is not None:
                use = voice_clone_prompt["x_vector_only_mode"][i] or voice_clone_prompt["icl_mode"][i]
                spk_e = spk_embeds[i] if use else None
            elif spk in ("", None):
                spk_e = None
            else:
                if spk.lower() not in tc.spk_id:
                    raise NotImplementedError(f"Speaker {spk} not implemented")
                spk_e = emb_c(ids_t(tc.spk_id[spk.lower()]))
            assert lang is not None
            if lang.lower() == "auto":
                lang_id = None
            else:
                if lang.lower() not in tc.codec_language_id:
                    raise NotImplementedError(f"Language {lang} not implemented")
                lang_id = tc.codec_language_id[lang.lower()]
            if lang.lower() in ("chinese", "auto") and spk not in ("", None) and tc.spk_is_dialect.get(spk.lower()):
                lang_id = tc.codec_language_id[tc.spk_is_dialect[spk.lower()]]
            bos, eos, pad = text(ids_t([[mc.tts_bos_token_id, mc.tts_eos_token_id, mc.tts_pad_token_id]])).chunk(3, dim=1)
            prefix = ([tc.codec_nothink_id, tc.codec_think_bos_id, tc.codec_think_eos_id] if lang_id is None else
                      [tc.codec_think_id, tc.codec_think_bos_id, lang_id, tc.codec_think_eos_id])
            cod = [emb_c(ids_t([prefix]))]
            if spk_e is not None:
                cod.append(spk_e.view(1, 1, -1))
            cod.append(emb_c(ids_t([[tc.codec_pad_id, tc.codec_bos_id]])))
            cod = torch.cat(cod, dim=1)                                   # [..., codec_pad, codec_bos]
            role = text(iid[:, :3])
            head = torch.cat((pad.expand(-1, cod.shape[1] - 2, -1), bos), dim=1) + cod[:, :-1]
            parts += [role, head]
            icl = (voice_clone_prompt is not None and voice_clone_prompt.get("ref_code", None) is not None
                   and voice_clone_prompt["icl_mode"][i])
            if icl:
                icl_embed, trail = m.generate_icl_prompt(
                    text_id=iid[:, 3:-5], ref_id=ref_ids[i][:, 3:-2],
                    ref_code=torch.as_tensor(voice_clone_prompt["ref_code"][i]).to(dev).clone(),
                    tts_pad_embed=pad, tts_eos_embed=eos, non_streaming_mode=non_streaming_mode)
                parts.append(icl_embed)
            elif non_streaming_mode:
                body = iid[:, 3:-5]
                parts.append(torch.cat((text(body), eos), dim=1) + emb_c(ids_t([[tc.codec_pad_id] * (body.shape[1] + 1)])))
                parts.append(pad + emb_c(ids_t([[tc.codec_bos_id]])))
                trail = pad
            else:
                parts.append(text(iid[:, 3:4]) + cod[:, -1:])
                trail = torch.cat((text(iid[:, 4:-5]), eos), dim=1)
            seqs.append(torch.cat(parts, dim=1).squeeze(0))
            trailing.append(trail.squeeze(0))
        # left-pad the batch (B is always 1 through the public API)
        L = max(s.shape[0] for s in seqs)
        H = seqs[0].shape[1]
        embeds = torch.zeros(len(seqs), L, H, dtype=seqs[0].dtype, device=dev)
        mask = torch.zeros(len(seqs), L, dtype=torch.long, device=dev)
        for b, s in enumerate(seqs):
            embeds[b, L - s.shape[0]:] = s
            mask[b, L - s.shape[0]:] = 1
        Tt = max(t.shape[0] for t in trailing)
        tth = pad.squeeze(0).expand(len(seqs), Tt, H).clone()
        for b, t in enumerate(trailing):
            tth[b, : t.shape[0]] = t
        if len(seqs) == 1 and instruct_ids is not None and instruct_ids[0] is not None:
            # a single prompt is not padded: its instruct rows come first and depend on the instruct ids alone (fq3hip/prefix_cache.py)
            from .prompt import host_ids
            key = tuple(host_ids(instruct_ids[0]))
            if key:
                embeds.fq3_prefix = (len(key), key)
        return embeds, mask, tth, pad

    def _after_prepare(self, m, tie):
        if not self._warmed_up:
            self.warmup(tie.shape[1])
        m.talker.rope_deltas = None
        return m.talker, m.config.talker_config

    def _prepare_generation(self, text: str, ref_audio=None, ref_text: str = "", language: str = "English",
                            xvec_only: bool = False, non_streaming_mode: bool = False, append_silence: bool = True,
                            voice_clone_prompt=None, instruct: Optional[str] = None, input_ids=None):
        if input_ids is None:
            input_ids = self.model._tokenize_texts([self.model._build_assistant_text(text)])
        instruct_ids = [None]
        if instruct:
            instruct_ids = [self.model._tokenize_texts([self.model._build_instruct_text(instruct)])[0]]
        vcp, ref_ids, using_icl = self._resolve_voice_clone_prompt(
            input_ids=input_ids, ref_audio=ref_audio, ref_text=ref_text, xvec_only=xvec_only,
            append_silence=append_silence, voice_clone_prompt=voice_clone_prompt)
        if instruct and not using_icl:
            logger.warning("Base-model instruct with x-vector-only voice cloning is experimental; prefer xvec_only=False.")
        m = self.model.model
        tie, tam, tth, tpe = self._build_talker_inputs_local(
            m=m, input_ids=input_ids, ref_ids=ref_ids, voice_clone_prompt=vcp,
            languages=[language] if language is not None else ["Auto"], speakers=None,
            non_streaming_mode=non_streaming_mode, instruct_ids=instruct_ids)
        talker, config = self._after_prepare(m, tie)
        ref_codes = None
        if using_icl and vcp.get("ref_code") and vcp["ref_code"][0] is not None:
            ref_codes = torch.as_tensor(vcp["ref_code"][0])
        return m, talker, config, tie, tam, tth, tpe, ref_codes

    def _prepare_generation_custom(self, text: str, language: str, speaker: Optional[str],
                                   instruct: Optional[str] = None, non_streaming_mode: bool = True, input_ids=None):
        if input_ids is None:
            input_ids = self.model._tokenize_texts([self.model._build_assistant_text(text)])
        instruct_ids = [None if not instruct else
                        self.model._tokenize_texts([self.model._build_instruct_text(instruct)])[0]]
        m = self.model.model
        tie, tam, tth, tpe = self._build_talker_inputs_local(
            m=m, input_ids=input_ids, ref_ids=[None], voice_clone_prompt=None,
            languages=[language] if language is not None else ["Auto"], speakers=[speaker],
            non_streaming_mode=non_streaming_mode, instruct_ids=instruct_ids)
        talker, config = self._after_prepare(m, tie)
        return m, talker, config, tie, tam, tth, tpe

    # ---- audio output stage (opt-in) ---------------------------------------------------------------------------------
    @contextlib.contextmanager
    def audio_output(self, sample_rate: Optional[int] = None, encoding: str = "f32", speed: float = 1.0):
        """Context manager: inside it the single-stream entry points (``generate_*``, ``generate_*_streaming``, ``stream_*``) hand out
        audio at ``sample_rate`` (None: the model's) in ``encoding`` (``f32`` | ``s16`` | ``mulaw`` | ``alaw`` | ``flac``), resampled and
        encoded on the device before the copy to the host (``fq3hip/audio_out.py``); ``sr`` in what they yield or return is the output
        rate.  ``flac``: the s16 samples compressed losslessly on the device; the streaming entry points yield ``uint8`` chunks that
        concatenate to a FLAC stream (the first one starts with the header), the one-shot ones return one ``uint8`` array, a FLAC file.
        ``speed`` in [0.25, 4.0] (1.0: off) time-scales the audio on the device first: an utterance of n samples becomes
        ceil(n / speed) samples at the same pitch.  The ``*_batch`` entry points raise ``ValueError`` inside it.  Outside it nothing
        changes."""
        from .audio_out import AudioOutSpec
        spec = AudioOutSpec(sample_rate, encoding, speed).validate(self.sample_rate)
        prev, self._audio_spec = getattr(self, "_audio_spec", None), spec
        try:
            yield spec
        finally:
            self._audio_spec = prev

    # ---- reproducible sampling (opt-in) ------------------------------------------------------------------------------
    @contextlib.contextmanager
    def seeded(self, seed: Optional[int]):
        """Context manager: inside it the single-stream entry points (``generate_*``, ``generate_*_streaming``, ``stream_*``) sample
        with ``seed`` (an integer in [0, 2^64); ``ValueError`` otherwise): the sampling noise is a pure function of (seed, frame)
        generated on the device, so the same request gives the same codes -- streaming or not, at any chunk size, whole or incremental
        text.  Iterate a streaming generator inside the context.  With ``do_sample=False`` the talker's greedy choice ignores the seed; a
        code predictor that still samples (``predictor_graph.do_sample``) draws its codebooks from it.  The ``*_batch`` entry points
        take ``seeds=`` instead.  Not re-entrant across threads, like the rest of the model.  Outside it nothing changes."""
        from .generate import validate_seed
        seed = validate_seed(seed)
        prev, self._seed = getattr(self, "_seed", None), seed
        try:
            yield seed
        finally:
            self._seed = prev

    # ---- exact streaming (opt-in) --------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def exact_streaming(self):
        """Context manager: inside it every streaming vocoder this model hands out (``streaming_vocoder``: the ``generate_*_streaming``,
        ``stream_*``, ``generate_long_*_streaming``, ``*_batch_streaming`` / ``stream_*_batch`` entry points and the server's workers)
        is exact: the streamed audio is, sample for sample, the one-pass decode of the utterance's codes, whatever the chunk size and
        whichever lanes share a launch.  Behind an ICL reference the stream begins at ``StreamingVocoder.c0``, a few samples before
        the non-streaming cut, and up to ``CHUNK_FRAMES`` total frames ``generate_voice_clone``'s waveform is the stream from sample
        ``cut - c0`` on.  Iterate a streaming generator inside the context.  Outside it nothing changes: the reference's windowing."""
        prev, self._exact_stream = getattr(self, "_exact_stream", False), True
        try:
            yield
        finally:
            self._exact_stream = prev

    # ---- loudness (opt-in; fq3hip/loudness.py) ------------------------------------------------------
    @contextlib.contextmanager
    def loudness(self, target_lufs: float = -16.0, ceiling_db: float = -1.0, max_gain_db: float = 20.0):
        """Context manager: inside it the one-shot entry points (``generate``, ``generate_voice_clone``, ``generate_custom_voice``,
        ``generate_voice_design``), the non-streaming ``*_batch`` ones and the non-streaming ``generate_long_*`` return every utterance
        measured (ITU-R BS.1770-4, integrated, gated) and scaled to ``target_lufs`` on the device, on the vocoder's stream and in front
        of the copy to the host and of an open ``audio_output`` stage.  The gain is bounded by ``max_gain_db`` and by what keeps the
        sample peak at or below ``ceiling_db`` dBFS -- a bound on the gain, there is no limiter -- and an utterance that cannot be
        measured (shorter than 0.4 s, silent, not finite) is left as it is.  Long form: each segment is measured on its raw waveform
        and its gain applied to what the join stage emits for it, so the segments leave at one level; the join's silence decisions
        see the unscaled samples.  Yields a ``LoudnessSession``: ``.stats`` holds the ``LoudnessStats`` of the last call, one per
        utterance (per segment for long form).  Every STREAMING entry point raises ``ValueError`` inside it: a stream's gain cannot be
        known before it ends -- measure the voice once (``measure_loudness``) and stream inside ``fixed_gain``.  The defaults are not
        tuned on real voices.  Outside it nothing changes."""
        from .loudness import LoudnessSpec, design
        spec = LoudnessSpec(target_lufs, ceiling_db, max_gain_db)
        design(self.sample_rate, spec)                       # the library's own range checks (host only)
        if getattr(self, "_gain", None) is not None:
            raise ValueError("loudness() inside fixed_gain(): one of the two sets the level")
        if getattr(self, "_lvl", None) is not None:
            raise ValueError("loudness() inside leveller(): the two answer the same question")
        prev, self._loud = getattr(self, "_loud", None), LoudnessSession(spec)
        try:
            yield self._loud
        finally:
            self._loud = prev

    @contextlib.contextmanager
    def fixed_gain(self, gain_db: float):
        """Context manager: inside it every vocoder this model hands out (``streaming_vocoder``, hence every streaming entry point and
        the server's workers) and every one-shot, batch and long-form path multiplies its audio by ``10^(gain_db / 20)`` on the device
        (``fq3_loud_apply``, the factor read from a 1-element device tensor), in front of the time-scale and output stages.
        ``gain_db`` in [-60, 40].  The gain itself does not limit -- float32 output may exceed 1.0, the s16 / G.711 encoders clamp --
        so stream inside ``limiter()`` as well when the level of what comes is not known.  Iterate a
        streaming generator inside the context.  Outside it nothing changes."""
        from .loudness import gain_factor
        factor = gain_factor(gain_db)
        if getattr(self, "_loud", None) is not None:
            raise ValueError("fixed_gain() inside loudness(): one of the two sets the level")
        prev, self._gain = getattr(self, "_gain", None), dict(gain_db=float(gain_db), factor=factor, tensors={})
        try:
            yield float(np.float32(factor))
        finally:
            self._gain = prev

    @contextlib.contextmanager
    def limiter(self, ceiling_db: float = -1.0, lookahead_ms: float = 5.0, hold_ms: float = 20.0):
        """Context manager: inside it every vocoder this model hands out (``streaming_vocoder``, hence the single-stream streaming
        entry points and the server's workers) and every one-shot, ``*_batch`` and long-form path runs a true-peak look-ahead
        limiter on the device (``fq3hip/limiter.py``) directly behind the gain of ``fixed_gain`` / ``loudness``
        and in front of the time-scale and output stages: no sample leaves above ``ceiling_db`` dBFS (by more than one part in 2^22),
        whatever the stream does later.  The audio keeps its length and is delayed by ``lookahead_ms`` plus 6 samples inside a stream:
        a chunk comes out that much shorter, and the samples held back come with the final chunk (or one more, final, chunk).  A
        stream's output does not depend on the chunk size beyond what the vocoder's windowing does (``exact_streaming``: not at all).
        The ``*_batch_streaming`` / ``stream_*_batch`` entry points give every utterance its own limiter; long form limits the ONE
        joined stream, behind the join and the per-segment gains.  Yields the ``LimiterSpec``.  The defaults are not tuned on real
        voices.  Iterate a streaming generator inside the context.  Outside it nothing changes."""
        from .limiter import LimiterSpec, design
        spec = LimiterSpec(ceiling_db, lookahead_ms, hold_ms)
        design(self.sample_rate, spec)                       # the library's own range checks (host only)
        prev, self._limit = getattr(self, "_limit", None), spec
        try:
            yield spec
        finally:
            self._limit = prev

    @contextlib.contextmanager
    def leveller(self, target_lufs: float = -16.0, ceiling_db: float = -1.0, max_gain_db: float = 20.0, initial_gain_db: float = 0.0,
                 smooth_hops: int = 10, min_blocks: int = 8):
        """Context manager: inside it every vocoder this model hands out (``streaming_vocoder``, hence every streaming entry point and
        the server's workers) and every one-shot, ``*_batch`` and long-form path runs the streaming loudness leveller on the device
        (``fq3hip/leveller.py``) behind the gain of ``fixed_gain`` and in front of the limiter, the time-scale
        and the output stages.  It is causal and holds nothing back: a chunk keeps its length, and a sample's gain comes from the
        BS.1770 measure of the 100 ms hops that ended before its own began -- ``initial_gain_db`` until ``min_blocks`` blocks of 400 ms
        passed the absolute gate, then the mean of the last ``smooth_hops`` targets -- so the stream converges to the level
        ``loudness()`` would have given the whole utterance.  It does NOT limit: a hop louder than everything before it can pass
        ``ceiling_db``, so stream inside ``limiter()`` as well.  A stream's output does not depend on the chunk size beyond what the
        vocoder's windowing does (``exact_streaming``: not at all).  The batch entry points give every utterance its own leveller;
        long form levels the ONE joined stream, behind the join and the gains.  Together with ``loudness()`` it raises ``ValueError``:
        the two answer the same question.  Yields the ``LevelSpec``.  The defaults are NOT tuned on real voices.  Iterate a streaming
        generator inside the context.  Outside it nothing changes."""
        from .leveller import LevelSpec
        from .loudness import design
        spec = LevelSpec(target_lufs, ceiling_db, max_gain_db, initial_gain_db, smooth_hops, min_blocks)
        design(self.sample_rate, spec.loudness)              # the library's own range checks (host only)
        if getattr(self, "_loud", None) is not None:
            raise ValueError("leveller() inside loudness(): the two answer the same question")
        prev, self._lvl = getattr(self, "_lvl", None), spec
        try:
            yield spec
        finally:
            self._lvl = prev

    def _stream_level_hops(self) -> int:
        """The capacity of an utterance's leveller: the hops of the longest stream the model can decode -- ``max_seq_len`` frames, the
        bound of every frame limit (``max_new_tokens``, a text session) -- and at least the default 4096."""
        from .leveller import MAX_HOPS
        tok = getattr(getattr(getattr(self, "model", None), "model", None), "speech_tokenizer", None)
        frames = int(getattr(self, "max_seq_len", 2048) or 2048)
        per_frame = int(getattr(getattr(tok, "cfg", None), "total_upsample", 0) or (self.sample_rate * 2 // 25))
        return min(MAX_HOPS, max(4096, frames * per_frame // (self.sample_rate // 10) + 2))

    def _levelled(self, x, stream=None, inplace: bool = False):
        """A whole utterance (contiguous float32 device vector) through the open ``leveller`` context's stage on ``stream`` (None: the
        current one): one object per (device, stream), kept, reset for every utterance, replaced by a larger one when an utterance
        needs more hops."""
        from .leveller import Leveller, capacity_for
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        levs = self.__dict__.setdefault("_levellers", {})
        key = (str(x.device), s.cuda_stream)
        need = capacity_for(int(x.numel()), self.sample_rate)
        if key not in levs or levs[key].spec.pooled != self._lvl.pooled or levs[key].capacity_hops < need:
            levs[key] = Leveller(self._lvl, self.sample_rate, x.device, s, capacity_hops=max(need, 4096))
        levs[key].reset(self._lvl.initial_gain_db)
        return levs[key].push(x, final=True, out=x if inplace else None)

    def _limited(self, x, stream=None):
        """A whole utterance (contiguous float32 device vector) through the open ``limiter`` context's stage on ``stream`` (None: the
        current one): one object per (device, stream), kept, reset for every utterance."""
        from .limiter import Limiter
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        lims = self.__dict__.setdefault("_limiters", {})
        key = (str(x.device), s.cuda_stream)
        if key not in lims or lims[key].spec != self._limit:
            lims[key] = Limiter(self._limit, self.sample_rate, x.device, s)
        lims[key].reset()
        return lims[key].push(x, final=True)

    def _gain_tensor(self, device=None):
        """the open ``fixed_gain`` context's factor as a 1-element float32 tensor on ``device`` (made once per device), or None"""
        g = getattr(self, "_gain", None)
        if g is None:
            return None
        dev = torch.device(self.device if device is None else device)
        if dev.index is None and dev.type == "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in g["tensors"]:
            g["tensors"][dev] = torch.tensor([g["factor"]], dtype=torch.float32, device=dev)
        return g["tensors"][dev]

    def _levelling(self) -> bool:
        return (getattr(self, "_loud", None) is not None or getattr(self, "_gain", None) is not None or getattr(self, "_limit", None) is not None
                or getattr(self, "_lvl", None) is not None)

    def _refuse_streaming_loudness(self) -> None:
        if getattr(self, "_loud", None) is not None:
            raise ValueError("a stream's gain cannot be known before the stream ends, so the streaming entry points do not run inside "
                             "loudness(): measure the voice once (measure_loudness) and stream inside fixed_gain(stats.gain_db)")

    def _meter(self, spec, device, stream):
        """One ``LoudnessMeter`` per (device, stream), kept: its buffers are reused by the utterances that follow on that stream.  A
        meter is made for one spec (the gain constants live in it): another spec on the same stream replaces it, so the cache does not
        grow with the targets a caller asks for."""
        from .loudness import LoudnessMeter
        meters = self.__dict__.setdefault("_meters", {})
        key = (str(device), None if stream is None else stream.cuda_stream)
        if key not in meters or meters[key].spec != spec:
            meters[key] = LoudnessMeter(spec, self.sample_rate, device, stream)
        return meters[key]

    def _measure(self, x, key=None, stream=None):
        """``x`` (contiguous float32 device vector) through the open ``loudness`` context's meter on ``stream`` (None: the current
        one) -> the device stats buffer, also noted in the session under ``key``"""
        sess = self._loud
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        meter = self._meter(sess.spec, x.device, s)
        meter.reset()
        meter.push(x, final=True)
        buf = meter.finish()
        sess.put(key, buf)
        return buf

    def _level(self, wav, key=None, stream=None, inplace: bool = False):
        """A whole utterance's waveform (device tensor or host array) as the open ``loudness`` / ``fixed_gain`` / ``limiter`` contexts
        want it: a float32 device vector, measured and scaled, or multiplied by the fixed factor, and then limited.  Outside all of
        them: ``wav`` itself."""
        if not self._levelling():
            return wav
        from .loudness import apply_gain, gain_of
        dev = torch.device(self.device) if not isinstance(self.device, torch.device) else self.device
        if torch.is_tensor(wav) and wav.is_cuda:
            x = wav.reshape(-1)
            if x.dtype != torch.float32 or not x.is_contiguous():
                x, inplace = x.float().contiguous(), False
        else:
            x, inplace = torch.from_numpy(np.ascontiguousarray(_to_numpy(wav), dtype=np.float32).reshape(-1)).to(dev), True
        if self._gain is not None or self._loud is not None:
            gain = self._gain_tensor(x.device) if self._gain is not None else gain_of(self._measure(x, key, stream))
            x = apply_gain(x, gain, stream, out=x if inplace else None)
        if getattr(self, "_lvl", None) is not None:
            x = self._levelled(x, stream, inplace)
        if getattr(self, "_limit", None) is None:
            return x
        y = self._limited(x, stream)
        if not inplace:
            return y
        # (the limiter reads its tiles' halos while other tiles write: it cannot run in place, so a row levelled in place is copied back)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(x.device)):
            x.copy_(y)
        return x

    def measure_loudness(self, audio, spec=None):
        """``audio`` (a device tensor or a host array, mono, at the model's rate) -> ``LoudnessStats``: its integrated loudness, sample
        peak and the gain ``spec`` (a ``LoudnessSpec``; None: the defaults) would give it, measured on the device.  How a caller
        calibrates a voice once -- synthesise a sentence, measure it -- and then streams inside ``fixed_gain(stats.gain_db)``."""
        from .loudness import LoudnessSpec
        spec = LoudnessSpec() if spec is None else spec
        if not isinstance(spec, LoudnessSpec):
            raise ValueError(f"spec must be a LoudnessSpec or None, not {type(spec).__name__}")
        dev = torch.device(self.device) if not isinstance(self.device, torch.device) else self.device
        if torch.is_tensor(audio) and audio.is_cuda:
            x = audio.reshape(-1).float().contiguous()
        else:
            x = torch.from_numpy(np.ascontiguousarray(_to_numpy(audio), dtype=np.float32).reshape(-1)).to(dev)
        meter = self._meter(spec, x.device, torch.cuda.current_stream(x.device))
        meter.reset()
        meter.push(x, final=True)
        return meter.stats()

    def _exact_kw(self) -> dict:
        """``exact=True`` for the vocoders built inside ``exact_streaming`` -- nothing at all outside it (the calls stay what they were)."""
        return dict(exact=True) if getattr(self, "_exact_stream", False) else {}

    def _gain_kw(self) -> dict:
        """``gain=`` for the vocoders built inside ``fixed_gain`` -- nothing at all outside it (the calls stay what they were)."""
        kw = dict(gain=self._gain_tensor()) if getattr(self, "_gain", None) is not None else {}
        if getattr(self, "_limit", None) is not None:
            # (the vocoders of one model share the vocoder stream; the pool is per spec, so a change of context starts another)
            kw["limiter"] = self._limit
            kw["limiter_pool"] = self.__dict__.setdefault("_limiter_pools", {}).setdefault(self._limit, [])
        if getattr(self, "_lvl", None) is not None:
            # (the pool is keyed WITHOUT the initial gain, which is set per stream: contexts that differ in it alone share objects)
            kw["leveller"] = self._lvl
            kw["leveller_pool"] = self.__dict__.setdefault("_leveller_pools", {}).setdefault(self._lvl.pooled, [])
            kw["leveller_hops"] = self._stream_level_hops()
        return kw

    def _seed_kw(self) -> dict:
        """``seed=`` for the decode loops inside ``seeded`` -- nothing at all outside it (the calls stay what they were)."""
        seed = getattr(self, "_seed", None)
        return {} if seed is None else dict(seed=seed)

    def _refuse_batch_audio_output(self) -> None:
        if getattr(self, "_audio_spec", None) is not None:
            raise ValueError("the batch entry points decode their audio in groups and do not run the audio output stage: call them outside "
                             "audio_output(), or use the single-stream entry points (the server builds one vocoder per request instead)")

    def _batch_outputs(self, output, n: int) -> Optional[list]:
        """``output=`` of the batch entry points -> None, or one validated ``AudioOutSpec`` or None per text.  Every argument error
        surfaces here, before anything is prepared or decoded."""
        if output is None:
            return None
        from .audio_out import AudioOutSpec
        if getattr(self, "_audio_spec", None) is not None:
            raise ValueError("output= inside audio_output(): the batch entry points take their output specs as output= alone; call them "
                             "outside the context")
        specs = self._per_text(output, n, "output")
        for sp in specs:
            if sp is not None and not isinstance(sp, AudioOutSpec):
                raise ValueError(f"output must be an AudioOutSpec, or a list with one AudioOutSpec or None per text, not {type(sp).__name__}")
        specs = [None if sp is None else sp.validate(self.sample_rate) for sp in specs]
        return specs if any(sp is not None for sp in specs) else None

    STAGE_POOL_MAX = 256

    def _take_stage(self, spec, stream):
        """An output stage for one utterance of a batched run: an idle one of the same spec and stream from the model's pool, reset,
        or a new one -- its device buffers are not allocated and freed per reply (a free synchronises the device while other lanes run)."""
        from .audio_out import AudioOut
        pool = self.__dict__.setdefault("_stage_pools", {}).setdefault((spec, str(self.device), stream), [])
        try:
            st = pool.pop()
        except IndexError:
            st = AudioOut(spec, self.sample_rate, self.device, stream)
            st.pool = pool
            return st
        st.reset()
        return st

    def _give_stage(self, st) -> None:
        pool = getattr(st, "pool", None)
        if pool is not None and len(pool) < self.STAGE_POOL_MAX and not any(st is other for other in pool):
            pool.append(st)

    def _one_shot_output(self, wav, spec=None) -> Tuple[np.ndarray, int]:
        """A whole utterance's waveform (device tensor or host array) through the output stage of the open context (or of ``spec``)."""
        from .audio_out import AudioOut
        dev = torch.device(self.device) if not isinstance(self.device, torch.device) else self.device
        stage = AudioOut(self._audio_spec if spec is None else spec, self.sample_rate, wav.device if hasattr(wav, "is_cuda") and wav.is_cuda else dev)
        x = wav.flatten().float() if hasattr(wav, "cpu") else torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32).reshape(-1))
        out = stage.push_host(x.to(stage.dev), final=True)
        if stage.flac:                 # a whole FLAC file: its header carries the sample count
            out = np.concatenate([np.frombuffer(stage.header(stage.n_samples), dtype=np.uint8), out])
        return out, stage.out_rate

    @staticmethod
    def _tail_event(voc, timing: Optional[dict]):
        """After a streaming loop with an output stage: the stage's tail as one more chunk, when the last chunk was not marked final
        (an utterance that ends on a full chunk) -- with that event's timing, no codes, ``is_final``."""
        if voc.output is None and getattr(voc, "limit_spec", None) is None:
            return None
        tail, sr = voc.flush()
        if len(tail) == 0:
            return None
        t = dict(timing or {})
        t.update(chunk_index=t.get("chunk_index", -1) + 1, chunk_steps=0, prefill_ms=0, decode_ms=0.0, is_final=True)
        t.pop("first_text_ms", None)
        return tail, sr, t

    # ---- shared back halves -------------------------------------------------------------------------------------
    def _run_full(self, m, talker, config, tie, tam, tth, tpe, ref_codes, gen_kwargs) -> Tuple[list, int]:
        from .generate import fast_generate
        codec_ids, timing = fast_generate(talker=talker, talker_input_embeds=tie, attention_mask=tam,
                                          trailing_text_hiddens=tth, tts_pad_embed=tpe, config=config,
                                          predictor_graph=self.predictor_graph, talker_graph=self.talker_graph,
                                          **gen_kwargs, **self._seed_kw())
        if self._loud is not None:
            self._loud.begin()
        if codec_ids is None:
            logger.warning("Generation returned no tokens")
            if self._audio_spec is not None:
                a, sr = self._one_shot_output(np.zeros(1, dtype=np.float32))
                return [a], sr
            return [np.zeros(1, dtype=np.float32)], self.sample_rate
        # ICL: the reference codes go in front so the decoder has acoustic context (model.py:919-937)
        codes = torch.cat([ref_codes.to(codec_ids.device), codec_ids], dim=0) if ref_codes is not None else codec_ids
        ref_len = ref_codes.shape[0] if ref_codes is not None else 0
        tok = m.speech_tokenizer
        if ref_len > 0 and hasattr(tok, "decode_tensor") and hasattr(tok, "num_samples_total"):
            # the reference decodes ref + generated frames and cuts the reference's share (model.py:927-930); the HIP
            # decoder produces only that tail (bit-identical to the slice, fq3_codec_decode_tail)
            cut = int(ref_len / max(codes.shape[0], 1) * tok.num_samples_total(codes.shape[0]))
            pf = tok.prefix_for(ref_codes) if hasattr(tok, "prefix_for") else None          # the voice's cached front-end state
            wav = self._level(tok.decode_tensor(codes, cut, prefix=pf) if pf is not None else tok.decode_tensor(codes, cut))
            if self._audio_spec is not None:
                a, sr = self._one_shot_output(wav)
                out = [a]
            else:
                out, sr = [_to_numpy(wav)], tok.sample_rate
        elif self._audio_spec is not None and ref_len == 0 and hasattr(tok, "decode_tensor"):
            a, sr = self._one_shot_output(self._level(tok.decode_tensor(codes, 0)))
            out = [a]
        elif self._levelling() and ref_len == 0 and hasattr(tok, "decode_tensor"):
            # (``tok.decode`` of one utterance IS decode_tensor: the waveform stays on the device for the meter and the multiply)
            out, sr = [_to_numpy(self._level(tok.decode_tensor(codes, 0)))], tok.sample_rate
        else:
            audio_list, sr = tok.decode({"audio_codes": codes.unsqueeze(0)})
            out = []
            for a in audio_list:
                a = _to_numpy(a)
                if ref_len > 0:
                    a = a[int(ref_len / max(codes.shape[0], 1) * len(a)):]
                if self._levelling():
                    a = self._level(a)                             # a foreign tokenizer's host waveform: uploaded for the stage
                    a = a if self._audio_spec is not None else _to_numpy(a)
                if self._audio_spec is not None:
                    a, sr = self._one_shot_output(a)
                out.append(a)
        n = timing["steps"]
        total = timing["prefill_ms"] / 1000 + timing["decode_s"]
        logger.info("Generated %.2fs audio in %.2fs (%.1fms/step, RTF: %.2f)", n / 12.5, total, timing["ms_per_step"],
                    (n / 12.5) / total if total > 0 else 0)
        return out, sr

    def _vocoder_stream(self, tok):
        """The HIP stream every streaming vocoder of this model runs on (one codec workspace -> one stream), or None for a
        foreign tokenizer that is decoded synchronously."""
        use_side = torch.cuda.is_available() and hasattr(tok, "decode_tensor") and hasattr(tok, "num_samples_total")
        if not use_side:
            return None
        if getattr(self, "_voc_stream", None) is None:
            dev = torch.device(self.device) if not isinstance(self.device, torch.device) else self.device
            # vocoder_stream_priority (attribute, default None = the device default): HIP stream priority of the vocoder
            # stream, larger = lower.  Set it before the first streaming call.
            prio = getattr(self, "vocoder_stream_priority", None)
            share = getattr(self, "vocoder_cu_share", None)
            if share:
                # measurement switch (attribute, default None): the vocoder confined to a share of the CUs (fq3hip/streams.py::cu_masked_stream)
                from .streams import cu_masked_stream
                self._voc_stream = cu_masked_stream(dev, float(share))
                return self._voc_stream
            from .streams import concurrent_stream
            # a stream VERIFIED to execute beside the decode stream: one that shares its hardware queue would hold the first audio chunk
            # back until the next chunk's frames -- queued before it -- have run (fq3hip/streams.py)
            self._voc_stream = concurrent_stream(dev, prio)
        return self._voc_stream

    def streaming_vocoder(self, ref_codes, chunk_size: int, output=None) -> "StreamingVocoder":
        """A fresh windowing state for one utterance (used by the streaming entry points and by the batch server).  ``output``: an
        ``AudioOutSpec`` for this utterance's audio (default: that of the open ``audio_output`` context, if any)."""
        self._refuse_streaming_loudness()
        tok = self.model.model.speech_tokenizer
        return StreamingVocoder(tok, ref_codes, chunk_size, self.device, self._vocoder_stream(tok),
                                output=output if output is not None else getattr(self, "_audio_spec", None), **self._exact_kw(),
                                **self._gain_kw())

    def _run_streaming(self, m, talker, config, tie, tam, tth, tpe, ref_codes, gen_kwargs, chunk_size: int,
                       parity_mode: bool = False):
        """model.py:1048-1137: the decode loop yields code chunks, ``StreamingVocoder`` turns each into the audio the
        reference's windowing would emit for it."""
        from .streaming import fast_generate_streaming, parity_generate_streaming
        self._refuse_streaming_loudness()
        self._last_levelled = None       # (``last_level_gain_db`` speaks of THIS stream once it has ended, never of an earlier one)
        tok = m.speech_tokenizer
        voc = StreamingVocoder(tok, ref_codes, chunk_size, self.device, self._vocoder_stream(tok), output=self._audio_spec, **self._exact_kw(),
                               **self._gain_kw())
        fn = parity_generate_streaming if parity_mode else fast_generate_streaming
        stream = fn(talker=talker, talker_input_embeds=tie, attention_mask=tam, trailing_text_hiddens=tth,
                    tts_pad_embed=tpe, config=config, predictor_graph=self.predictor_graph,
                    talker_graph=self.talker_graph, chunk_size=chunk_size, **gen_kwargs, **self._seed_kw())
        timing = None
        for chunk, timing in stream:
            ev = timing.pop("codes_ready_event", None)
            new_audio, sr = voc.push(chunk, ev, final=bool(timing.get("is_final")))
            yield new_audio, sr, timing
        tail = self._tail_event(voc, timing)
        if voc.level_spec is not None:
            with (contextlib.nullcontext() if voc.side is None else torch.cuda.stream(voc.side)):
                voc.level_release()                                 # (a stream that ended without a final chunk)
            self._last_levelled = voc
        if tail is not None:
            yield tail

    @property
    def last_level_gain_db(self) -> Optional[float]:
        """Inside or after ``leveller()``: the last target gain in dB of the single-stream or long-form stream that ended last -- what
        the same voice's next stream may start from as ``initial_gain_db`` -- or None when it never reached a valid measure (or nothing
        was levelled yet).  Waits for the vocoder's stream."""
        last = getattr(self, "_last_levelled", None)
        if last is None:
            return None
        return last.level_gain_db if hasattr(last, "level_gain_db") else last.final_gain_db

    @staticmethod
    def _gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample, repetition_penalty):
        return dict(max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens, temperature=temperature,
                    top_k=top_k, top_p=top_p, do_sample=do_sample, repetition_penalty=repetition_penalty)

    @staticmethod
    def _frame_limit(gen_kwargs) -> int:
        """the largest ``max_new_tokens`` of a batch's entries (one value, or one per text: ``_batch_feed``)"""
        n = gen_kwargs.get("max_new_tokens", 2048)
        return max(int(v) for v in n) if isinstance(n, (list, tuple)) else int(n)

    # ---- public generation entry points ----------------------------------------------------------------------------
    @torch.inference_mode()
    def generate_voice_clone(self, text: str, language: str, ref_audio: Optional[Union[str, Path]] = None,
                             ref_text: str = "", max_new_tokens: int = 2048, min_new_tokens: int = 2,
                             temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                             repetition_penalty: float = 1.05, xvec_only: bool = False,
                             non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                             instruct: Optional[str] = None, ref_spk: Optional[Union[str, Path]] = None,
                             ref_rvq: Optional[Union[str, Path]] = None, ref_spk_emb: Optional[np.ndarray] = None,
                             ref_codes: Optional[np.ndarray] = None,
                             voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None) -> Tuple[list, int]:
        """Voice cloning; returns ``([np.float32 waveform], sample_rate)``."""
        self._reject_ggml_cached_reference_args(ref_spk=ref_spk, ref_rvq=ref_rvq, ref_spk_emb=ref_spk_emb,
                                                ref_codes=ref_codes)
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        m, talker, config, tie, tam, tth, tpe, rc = self._prepare_generation(
            text=text, language=language, ref_audio=ref_audio, ref_text=ref_text, xvec_only=xvec_only,
            non_streaming_mode=nsm, append_silence=append_silence, voice_clone_prompt=voice_clone_prompt,
            instruct=instruct)
        return self._run_full(m, talker, config, tie, tam, tth, tpe, rc,
                              self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                               repetition_penalty))

    # ---- batched generation (extension: the reference has no multi-utterance entry point) ---------------------------------
    def _batch_decoder(self, lanes: int, staging: Optional[int] = None):
        """Lazily builds ``lanes`` decode contexts over this model's single weight replica, ``staging`` spare contexts
        (default: as many as lanes) that the next requests are prefilled into while the batch decodes, the KV block pool they
        all draw from, and the scheduler on top.

        ``self.batch_kv_blocks`` (attribute, default ``None``): size of that pool in 64-key blocks.  ``None`` = enough for every
        lane AND every spare context at ``max_seq_len`` (what static caches would reserve; the pool then never runs short).  A
        server that knows its traffic sets less -- e.g. ``(lanes + staging) * ceil((prompt + max_new_tokens + 1) / 64)`` --
        and a request the pool cannot hold yet waits until finished lanes give blocks back.  NOTE: a request reserves its WORST case up
        front (``prompt + max_new_tokens + 1`` key slots, capped at ``max_seq_len``: a short pool must show before any work is queued),
        so with the default ``max_new_tokens=2048`` at ``max_seq_len=2048`` every request takes a whole context's blocks and a reduced pool
        merely serialises requests -- size ``batch_kv_blocks`` from the ``max_new_tokens`` the callers really pass."""
        from .batching import BatchDecoder
        from .engine import Fq3Engine, Fq3KvPool
        from .batching import MAX_LANES
        lanes = max(1, min(int(lanes), MAX_LANES))
        staging = lanes if staging is None else max(0, int(staging))
        first = self.talker_graph.engine
        full = (lanes + staging) * Fq3KvPool.blocks_for(first.max_seq_len)
        want = getattr(self, "batch_kv_blocks", None)
        blocks = full if want is None else max(Fq3KvPool.blocks_for(first.max_seq_len), min(int(want), full))
        # batch_groups (attribute, default None = the library's choice: one chain): fq3_batch_set_option("groups"), a measurement switch
        groups = getattr(self, "batch_groups", None)
        cached = getattr(self, "_batch_cache", None)
        if cached is not None and cached[0] == (lanes, staging, blocks, groups):
            la = getattr(self, "batch_lookahead", None)
            cached[1].lookahead = (int(la) if la is not None else 1) if hasattr(cached[1].batch, "poll_async") else 0
            # the lanes follow this model's CURRENT predictor policy (it is copied into the loop state when a lane is armed)
            pg = self.predictor_graph
            cached[1].set_predictor_policy(do_sample=pg.do_sample, top_k=pg.top_k, top_p=pg.top_p, temperature=pg.temperature)
            cached[1].prefix_cache = getattr(self, "_batch_prefix_cache", None)
            return cached[1]
        self._batch_cache = None                    # a differently shaped scheduler: its contexts and pool go first
        pool = Fq3KvPool(first.cfg, blocks, device=str(first.device), dtype=first.dtype)
        mk = lambda: Fq3Engine(first.cfg, first.weights, device=str(first.device), dtype=first.dtype,
                               max_seq_len=first.max_seq_len, max_frames=first.max_frames, share=first, pool=pool)
        engines = [mk() for _ in range(lanes)]
        pg = self.predictor_graph
        dec = BatchDecoder(engines, predictor_policy=dict(do_sample=pg.do_sample, top_k=pg.top_k, top_p=pg.top_p,
                                                          temperature=pg.temperature),
                           staging=[mk() for _ in range(staging)], prefix_cache=getattr(self, "_batch_prefix_cache", None))
        dec.kv_pool = pool
        # batch_lookahead (attribute, default None = the scheduler's default, 1: the next batch of frames is queued before the previous
        # batch's poll is read; 0 = wait for every batch right after queuing it) -- see BatchDecoder.lookahead
        la = getattr(self, "batch_lookahead", None)
        if la is not None:
            dec.lookahead = int(la) if hasattr(dec.batch, "poll_async") else 0
        if groups is not None and hasattr(dec.batch, "set_option"):
            dec.batch.set_option("groups", int(groups))
            dec.n_groups = int(groups)
        if torch.cuda.is_available():
            tok = self.model.model.speech_tokenizer
            dec.beside = [st for st in (self._vocoder_stream(tok),) if st is not None]
        self._batch_cache = ((lanes, staging, blocks, groups), dec)
        return dec

    def _side_vocoder(self):
        """Vocoder for finished utterances of a batched run: decodes on its own HIP stream (the lock-step decode of the
        remaining / next utterances goes on meanwhile) and copies the waveform to pinned host memory asynchronously."""
        tok = self.model.model.speech_tokenizer
        if getattr(self, "_side_voc_stream", None) is None and torch.cuda.is_available() and hasattr(tok, "decode_tensor"):
            from .streams import concurrent_stream
            # ONE vocoder stream per model (probed once, fq3hip/streams.py): hardware queues are few, and the scheduler's prefill
            # stream and the lane groups' stream have to stay clear of it
            self._side_voc_stream = self._vocoder_stream(tok) or concurrent_stream(self.device)
        return _SideVocoder(tok, self.device, getattr(self, "_side_voc_stream", None))

    def _batch_feed(self, prepared, gen_kwargs, lanes: int, meta: dict, first_wave: Optional[int] = None, seeds=None):
        """``prepared``: an iterable (usually a generator: the prompt of utterance i is built when the scheduler asks for it) of
        ``(talker, config, tie, tam, tth, tpe, ref_codes | None)``.  Returns ``(head, source)`` for ``BatchDecoder.run``: the first
        ``lanes`` requests up front -- the first wave starts decoding before the later prompts exist -- and a ``source`` callback
        that prepares the rest one at a time at frame boundaries.  ``meta[i]`` receives the entry's ``ref_codes``.  ``seeds``: one
        sampling seed or None per entry (``generate.expand_seeds``).  ``gen_kwargs["max_new_tokens"]`` may be a list: entry i's own
        frame limit (the ``max_new_tokens`` of the batch entry points: one value, or one per text)."""
        from .batching import BatchRequest
        it = enumerate(prepared)

        def pull():
            nxt = next(it, None)
            if nxt is None:
                return None
            i, (talker, config, tie, tam, tth, tpe, rc) = nxt
            meta[i] = rc
            kw = dict(gen_kwargs)
            if isinstance(kw.get("max_new_tokens"), (list, tuple)):
                # one frame limit per entry (lanes then finish, and are re-used, at staggered frames)
                if i >= len(kw["max_new_tokens"]):
                    raise ValueError("max_new_tokens must be one value or one per text")
                kw["max_new_tokens"] = int(kw["max_new_tokens"][i])
            return BatchRequest(i, talker, tie, tam, tth, tpe, config, kw, seed=None if seeds is None else seeds[i])

        # (only the first SLICE of the first wave is built here: the scheduler pulls the rest from `source` in slices and queues every
        # slice's packed prefill behind the one before, so prompt builds and prefills overlap -- BatchDecoder.run, "first wave, pipelined")
        head = []
        wave = max(1, int(lanes) if first_wave is None else min(int(lanes), int(first_wave)))
        for _ in range(min(wave, 16)):
            r = pull()
            if r is None:
                break
            head.append(r)
        return head, pull

    def _run_batch_full(self, prepared, gen_kwargs, lanes: int, count: int, seeds=None, device_audio: bool = False,
                        outputs=None) -> List[Tuple[list, int]]:
        """The lock-step decode of ``count`` prepared utterances (see :meth:`_batch_feed`) through ``lanes`` lanes, every finished
        utterance vocoded on the side stream (the reference's share of an ICL waveform is cut by not producing it,
        model.py:927-930).  One ``([waveform], sample_rate)`` per entry, in input order.  ``device_audio`` (internal, long form): the
        waveforms are handed out as device tensors valid on the side vocoder's stream -- ``(out, voc)`` is returned -- and the caller
        runs the output chain itself.  ``outputs`` (:meth:`_batch_outputs`): utterance i with a spec comes back as
        ``([encoded array], output rate)`` -- the utterances vocoded together go through the output stage together, behind the levelling
        step (``_SideVocoder._encode_group``)."""
        if not device_audio:
            self._refuse_batch_audio_output()
        seeds = expand_seeds(seeds, count)
        meta: dict = {}
        dec = self._batch_decoder(lanes)
        # batch_first_wave (attribute): requests prepared + prefilled + armed before the first frame is queued (BatchDecoder.first_wave);
        # None = one per lane
        dec.first_wave = getattr(self, "batch_first_wave", None)
        head, source = self._batch_feed(prepared, gen_kwargs, len(dec.lanes), meta, dec.first_wave, seeds)
        out: List[Optional[Tuple[list, int]]] = [None] * count
        voc = self._side_vocoder()
        voc.device_only = bool(device_audio)
        if outputs is not None:
            voc.outputs, voc.stages = {i: sp for i, sp in enumerate(outputs) if sp is not None}, (self._take_stage, self._give_stage)
        rate_of = lambda rid: self.sample_rate if outputs is None or outputs[rid] is None else outputs[rid].out_rate(self.sample_rate)  # noqa: E731

        def nothing(rid):
            """an utterance without a single frame: one zero sample, through its stage if it has one"""
            if outputs is None or outputs[rid] is None:
                return [np.zeros(1, dtype=np.float32)], self.sample_rate
            z = torch.zeros(1, dtype=torch.float32, device=voc.dev)
            if voc.stream is not None:
                voc.stream.wait_stream(torch.cuda.current_stream(voc.dev))
            a = voc._encode_group([rid], [z])[0].array()
            return [a], rate_of(rid)
        if self._loud is not None:
            self._loud.begin(count)
        if self._levelling() and not device_audio:
            # between the decode and the pinned copy, on the vocoder's stream (long form levels behind the join instead)
            voc.level = lambda key, wav: self._level(wav, key, voc.stream, inplace=True)
        # batch_vocode_every (attribute; default 0 = vocode an utterance when it has ended; N > 0 = produce the waveform in slices every N
        # frames while the utterance still decodes -- exact, see _SideVocoder.inc_add -- so that what is left at the end is the last slice
        # only).  Measured on MI355X (profiles/r04_batch_e2e_vocode_every_*.txt): the slices contend with the latency-bound lock-step
        # frames for more than they save at the end -- 64 lanes x 128 utterances, 0.6B: 561x at 0, 537x at 64, 552x at 100; 1.7B: 458x vs
        # 443x -- so it is OFF by default; a server whose lanes finish at different times has nothing to gain from it either.
        inc = int(getattr(self, "batch_vocode_every", 0) or 0)
        if inc > 0 and not device_audio and outputs is None and not self._levelling() and voc.async_ok and hasattr(voc.tok, "decode_tensor_batch") and hasattr(voc.tok, "num_samples_total"):
            max_new = min(self._frame_limit(gen_kwargs), int(self.talker_graph.engine.max_frames))
            for rid, codes, info in dec.run(head, source=source, chunk_frames=inc):
                more = int(getattr(dec, "more_in_poll", 0))
                voc.inc_add(rid, codes, meta.get(rid), info.pop("codes_ready_event", None), bool(info.get("is_final")), more, max_new)
            for rid, a in voc.inc_collect():
                out[rid] = ([a], voc.sample_rate)
            return [o if o is not None else ([np.zeros(1, dtype=np.float32)], self.sample_rate) for o in out]
        for rid, codec_ids, timing in dec.run(head, source=source):
            more = int(getattr(dec, "more_in_poll", 0))
            if codec_ids is None:
                out[rid] = nothing(rid)
                if more <= 0:
                    voc.add_flush()
                continue
            rc = meta[rid]
            codes = torch.cat([rc.to(codec_ids.device), codec_ids], dim=0) if rc is not None else codec_ids
            # side stream; the next frames of the other lanes are not held up.  Utterances that finished in the same poll are vocoded
            # together (equal lengths: one batched launch set)
            voc.add(rid, codes, ref_len=rc.shape[0] if rc is not None else 0, more=more, ref=rc)
        voc.add_flush()
        if device_audio:
            for rid, a in voc.collect_device():
                out[rid] = ([a], voc.sample_rate)
            return out, voc
        for rid, a in voc.collect():
            out[rid] = ([a], voc.sample_rate if outputs is None else rate_of(rid))
        return out

    def _run_batch_streaming(self, prepared, gen_kwargs, chunk_size: int, lanes: int, rounds=None, stamp=None, seeds=None,
                             count: Optional[int] = None, device_audio: bool = False, outputs=None, group_marks: bool = False):
        """Streaming form of :meth:`_run_batch_full`: yields ``(index, audio_chunk, sample_rate, timing)`` for every
        ``chunk_size`` frames of any utterance -- per utterance exactly the chunks the single-utterance streaming entry point
        would produce (same windowing state machine).  ``timing``: ``chunk_index``, ``total_steps_so_far``, ``is_final``.
        ``rounds`` (incremental text, :meth:`_run_text_batch_streaming`): ``rounds(dec, meta)`` yields the ``(head, source)`` pairs of
        successive scheduler runs instead of the one pair :meth:`_batch_feed` makes of ``prepared``; ``stamp(index, timing)`` may add
        keys to a chunk's timing before it goes out.  ``device_audio`` (internal, long form; what is yielded by default does not
        change): a chunk vocoded on the vocoder stream is handed out as the group's device waveform row -- a float32 tensor valid on
        that stream, no copy to the host, no wait -- and the utterances' vocoders carry no output stage of their own.
        ``outputs`` (:meth:`_batch_outputs`): utterance i with a spec owns a pooled output stage; behind the gain and the limiter the
        rows of a launch group that have one go through ONE ``audio_out.push_group`` on the vocoder stream and reach pinned memory in
        one copy, and what is yielded for them is the encoded array and the output rate (``flac``: bytes, the stream header in the
        utterance's first chunk).  What the stage held back leaves with the utterance's final event (``StreamingVocoder.flush``).
        ``group_marks`` (internal, long form over many texts): the events a poll hands out together carry ``group_end`` in their
        timing, True on the last of them, so that the caller can take them through its own stages as one group."""
        self._refuse_streaming_loudness()
        if not device_audio:
            self._refuse_batch_audio_output()
        gain = None if device_audio else self._gain_tensor()       # (long form multiplies behind the join)
        limit = None if device_audio else getattr(self, "_limit", None)      # (and limits there, as one stream)
        lvl = None if device_audio else getattr(self, "_lvl", None)         # (and levels there, likewise)
        if seeds is not None:
            # the ``seeds=`` keyword of the public entry points is expanded HERE and in _run_batch_full, nowhere else; a caller that
            # builds its own requests (``rounds``) seeds them itself
            if rounds is not None or count is None:
                raise ValueError("seeds= goes with `prepared` and its `count`; requests made by `rounds` carry their own seed")
            seeds = expand_seeds(seeds, count)
        meta: dict = {}
        vocs, n_chunks = {}, {}
        dec = self._batch_decoder(lanes)
        # ``batch_first_wave_streaming`` (attribute, default None = one request per lane): requests prepared and prefilled in front of the
        # first frame, the others joining at the following frame boundaries.  MEASURED (profiles/r05_ttfa_first_wave.txt): a smaller
        # first wave does not buy its members a lower latency -- the prefills of the followers run beside their first frames and
        # stretch them (128 lanes: p25 305 ms / p50 395 ms at a wave of 32 against 340 ms for everybody at once) -- so the default stays.
        dec.first_wave = getattr(self, "batch_first_wave_streaming", None)
        pairs = rounds(dec, meta) if rounds is not None else [self._batch_feed(prepared, gen_kwargs, len(dec.lanes), meta, dec.first_wave, seeds)]
        tok = self.model.model.speech_tokenizer
        side = self._vocoder_stream(tok)
        batched = side is not None and hasattr(tok, "decode_tensor_batch")
        # chunks of different utterances that need the SAME decode shape (the first chunks of lanes that started together: reference + 8
        # frames in, the last 8 frames' samples out) go through one batched launch set on the vocoder stream, STREAM_GROUP at a time.
        # Round 6: a group is LAUNCHED as soon as it is full -- while the host still prepares the next group's inputs -- every group's
        # waveform goes to pinned host memory behind its launch set, and the groups are handed out one by one as their copies land: a
        # wave of 128 first chunks (four groups of 32) used to be prepared as a whole, launched group by group with a host wait after
        # each, and reached the caller all at once after the last group.  The bookkeeping -- the jobs of a poll ``[rid, meta, audio |
        # None, (codes_in, first, ev, ...) | None]``, their classes, the launches made -- is ``stream_groups.StreamGroups``; ``launch`` and
        # ``collect`` below are the device work it calls.  Per utterance the order of the events is kept BY THE LAUNCHES, in both modes: a
        # launch pushes its members' own stages and stream states, so a chunk never joins a class that would launch in front of an
        # earlier chunk of its utterance that still waits (lanes re-used at staggered frames produce that; the classes up to that
        # chunk's are launched first).  Groups are handed out in launch order, markers without audio come last.

        def launch(key, part):
            _T, first, pf_len = key
            for j in part:
                if j[3][2] is not None:
                    side.wait_event(j[3][2])
                else:
                    side.wait_stream(torch.cuda.current_stream(torch.device(self.device)))
            with torch.cuda.stream(side):
                exact = pf_len == "exact"
                pfs = [j[3][3] for j in part] if not exact and pf_len > 0 else None      # (phase 1 behind ICL references: the voices' cached front-end states)
                if exact:
                    # exact mode: the group's stream states take their new frames in one push; `first` = samples in front of an ICL cut's floor
                    wav = tok.stream_push([j[3][4] for j in part], torch.stack([j[3][0] for j in part]))[:, first:]
                elif len(part) == 1:
                    wav = (tok.decode_tensor(part[0][3][0], first, prefix=pfs[0]) if pfs else tok.decode_tensor(part[0][3][0], first)).reshape(1, -1)
                else:
                    stacked = torch.stack([j[3][0] for j in part])
                    wav = tok.decode_tensor_batch(stacked, first, prefixes=pfs) if pfs else tok.decode_tensor_batch(stacked, first)
                wav = wav.float()
                if gain is not None:
                    from .loudness import apply_gain
                    wav = apply_gain(wav.contiguous(), gain, side)
                finals = [bool(j[1].get("is_final")) for j in part]
                # a poll that completes two chunks of one shape puts an utterance into a part twice; a stage is pushed once per group
                # call, so such a part is cut into consecutive runs in which every utterance appears once (nearly always: one run)
                runs = runs_of(part)
                if lvl is not None:
                    # every utterance's own leveller takes its row and writes a row of the same length: the group stays one tensor,
                    # and the rows of a run go through ONE meter launch, ONE target launch and ONE multiply
                    from .leveller import push_group as level_group
                    rows, wav = wav, torch.empty(wav.shape, dtype=torch.float32, device=wav.device)
                    for run in runs:
                        level_group([vocs[part[k][0]].level_take() for k in run], [rows[k] for k in run], [finals[k] for k in run],
                                    outs=[wav[k] for k in run])
                        for k in run:
                            if finals[k]:
                                vocs[part[k][0]].level_release()
                host = landed = encoded = None
                staged = [k for k, j in enumerate(part) if vocs[j[0]].output is not None]
                if limit is not None:
                    # every utterance's own limiter takes its row: the rows come back shorter by what it holds back, or longer at the
                    # end.  ONE launch per run; the rows lie back to back in the run's device buffer
                    from .limiter import _push_group as limit_group
                    src, wav, bufs, place = wav, [None] * len(part), [], [None] * len(part)
                    for run in runs:
                        buf, spans, _s = limit_group([vocs[part[k][0]].limit_take() for k in run], [src[k] for k in run],
                                                     [finals[k] for k in run])
                        for k, (off, cnt) in zip(run, spans):
                            wav[k], place[k] = buf[off:off + cnt], (sum(int(b.numel()) for b in bufs) + off, cnt)
                            if finals[k]:
                                vocs[part[k][0]].limit_release()
                        bufs.append(buf)
                if staged:
                    # the rows with an output spec: one time-scale launch, one resample + encode launch per design, one pinned copy --
                    # per run, as the stages in front: a stage is pushed once per group call
                    from .audio_out import GroupCopy
                    encoded = []
                    for run in runs:
                        rows = [k for k in run if k in staged]
                        if rows:
                            encoded.append((rows, GroupCopy([vocs[part[k][0]]._stage() for k in rows], [wav[k] for k in rows],
                                                            [finals[k] for k in rows])))
                if limit is not None:
                    # the rows without an output spec: ONE pinned buffer behind one copy per run, and ONE event
                    host = [None] * len(part)
                    if len(staged) < len(part):
                        pinned, at = torch.empty(sum(int(b.numel()) for b in bufs), dtype=torch.float32, pin_memory=True), 0
                        for buf in bufs:
                            pinned[at:at + int(buf.numel())].copy_(buf, non_blocking=True)
                            at += int(buf.numel())
                        host = [None if k in staged else pinned[place[k][0]:place[k][0] + place[k][1]] for k in range(len(part))]
                    landed = torch.cuda.Event()
                    landed.record(side)
                elif not device_audio and len(staged) < len(part):
                    host = torch.empty(wav.shape, dtype=wav.dtype, pin_memory=True)
                    host.copy_(wav, non_blocking=True)
                    landed = torch.cuda.Event()
                    landed.record(side)
                elif staged:
                    landed = encoded[-1][1].event              # (one stream: the last run's copy lands last)
            return host, landed, wav, encoded

        def collect(part, handle):
            host, landed, wav, encoded = handle
            if landed is None:
                arr = wav                                      # device rows: whoever takes them works on the vocoder stream
            else:
                landed.synchronize()
                arr = ([None if h is None else h.numpy() for h in host] if isinstance(host, list) else
                       host.numpy() if host is not None else [None] * len(part))
            for k, j in enumerate(part):
                j[2] = arr[k]
            for rows, copy in encoded or ():
                for k, a in zip(rows, copy.rows()):
                    v = vocs[part[k][0]]
                    if v.stage.flac and not v.header_sent:
                        # a FLAC stream: the utterance's first chunk starts with the stream header (length unknown)
                        a, v.header_sent = np.concatenate([np.frombuffer(v.stage.header(), dtype=np.uint8), a]), True
                    part[k][2] = a
                    if part[k][1].get("is_final"):
                        self._give_stage(v.stage)

        # exact mode: (new codes, drop, ev, None, stream state, frames before the push) -- the class is (min(F, ctx_max), n_new) and the
        # drop, so every steady-state chunk of every lane falls into one class; a state is pushed once per call, so the k-th chunk an
        # utterance adds in a poll goes into the k-th generation of the class (``StreamGroups.key_of``)
        groups = StreamGroups(launch, collect, _SideVocoder.STREAM_GROUP, getattr(tok, "stream_ctx_max", None))
        self._stream_group_stats = groups.stats         # the counters of the newest run (jobs, launches, order_launches), nothing else kept
        add_job, launch_open, flush = groups.add, groups.launch_open, groups.flush

        def out(r, m):
            if stamp is not None:
                stamp(r, m)
            return m

        rate_of = lambda r: self.sample_rate if outputs is None or outputs[r] is None else outputs[r].out_rate(self.sample_rate)  # noqa: E731

        def marked(events):
            if not group_marks:
                return events
            # the whole poll is collected before its first event goes out: with ``device_audio`` nothing is copied, so nothing is
            # waited for; a caller that lands copies (``flush`` hands groups out as they land) would wait for the last of them here
            events = list(events)
            for i, ev in enumerate(events):
                ev[1]["group_end"] = i == len(events) - 1
            return events

        for head, source in pairs:
          for rid, codes, info in dec.run(head, source=source, chunk_frames=chunk_size):
            if rid not in vocs:
                vocs[rid] = (StreamingVocoder(tok, meta[rid], chunk_size, self.device, side, **self._exact_kw()) if device_audio
                             else self.streaming_vocoder(meta[rid], chunk_size))
                if outputs is not None and outputs[rid] is not None:
                    vocs[rid].output, vocs[rid].stage = outputs[rid], self._take_stage(outputs[rid], side)
                n_chunks[rid] = 0
            ev = info.pop("codes_ready_event", None)
            final = bool(info.get("is_final"))
            more = int(getattr(dec, "more_in_poll", 0))
            out_meta = dict(chunk_index=n_chunks[rid], total_steps_so_far=int(info.get("total_steps_so_far", 0)),
                            is_final=final, chunk_steps=0 if codes is None else int(codes.shape[0]))
            if codes is not None and codes.shape[0] > 0:
                if batched:
                    inp, first = vocs[rid].prepare(codes, ev)
                    if vocs[rid].exact:
                        add_job([rid, out_meta, None, (inp, first, ev, None, vocs[rid].cstream, vocs[rid].frames_before)])
                    else:
                        add_job([rid, out_meta, None, (inp, first, ev, vocs[rid].last_prefix)])
                else:
                    staged = limit is not None or lvl is not None or vocs[rid].output is not None
                    audio, _sr = vocs[rid].push(codes, ev, final=final) if staged else vocs[rid].push(codes, ev)
                    if final and vocs[rid].output is not None:
                        self._give_stage(vocs[rid].stage)
                    add_job([rid, out_meta, audio, None])
                n_chunks[rid] += 1
            elif final:
                tail = np.zeros(1 if codes is None else 0, dtype=np.float32)
                if lvl is not None and vocs[rid].level is not None:
                    launch_open()                                  # the utterance's chunks that still wait end its leveller's stream
                    with (contextlib.nullcontext() if side is None else torch.cuda.stream(side)):
                        vocs[rid].level_release()
                if vocs[rid].output is not None:
                    # what the output stage (and a limiter in front of it) held back leaves as this event's audio
                    launch_open()
                    tail, _sr = vocs[rid].flush()
                    if vocs[rid].stage.flac and not vocs[rid].header_sent:
                        tail, vocs[rid].header_sent = np.concatenate([np.frombuffer(vocs[rid].stage.header(), dtype=np.uint8), tail]), True
                    self._give_stage(vocs[rid].stage)
                elif limit is not None and vocs[rid].limit is not None:
                    launch_open()                                  # the utterance's chunks that still wait go in front of its tail
                    held, _sr = vocs[rid].flush()
                    tail = held if len(held) else tail
                add_job([rid, out_meta, tail, None])
                n_chunks[rid] += 1
            if more <= 0:
                for r, m, audio, _job in marked(flush()):
                    yield r, audio, rate_of(r), out(r, m)
          for r, m, audio, _job in marked(flush()):
            yield r, audio, rate_of(r), out(r, m)

    @staticmethod
    def _per_text(value, n: int, what: str) -> list:
        """One value for all texts, or one per text."""
        if isinstance(value, (list, tuple)):
            if len(value) != n:
                raise ValueError(f"{what} must be one value or one per text")
            return list(value)
        return [value] * n

    def _prepare_clone_batch(self, texts, language, ref_audio, ref_text, xvec_only, nsm, append_silence, instruct, voice_clone_prompt):
        langs = self._per_text(language, len(texts), "language")            # argument errors surface before anything is decoded

        def gen():
            for text, lang in zip(texts, langs):
                _m, talker, config, tie, tam, tth, tpe, rc = self._prepare_generation(
                    text=text, language=lang, ref_audio=ref_audio, ref_text=ref_text, xvec_only=xvec_only,
                    non_streaming_mode=nsm, append_silence=append_silence, voice_clone_prompt=voice_clone_prompt,
                    instruct=instruct)
                yield talker, config, tie, tam, tth, tpe, rc
        return gen()

    @torch.inference_mode()
    def generate_voice_clone_batch(self, texts: List[str], language: Union[str, List[str]] = "English",
                                   ref_audio: Optional[Union[str, Path]] = None, ref_text: str = "",
                                   max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9,
                                   top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                   repetition_penalty: float = 1.05, xvec_only: bool = False,
                                   non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                                   instruct: Optional[str] = None,
                                   voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                   lanes: int = 8, seeds=None, output=None) -> List[Tuple[list, int]]:
        """Voice cloning of several texts with one voice: up to ``lanes`` (<= 128) utterances decode in lock-step over
        one pass of the weights per frame (``fq3_batch_*``), finished lanes are refilled from the queue.  Returns one
        ``([np.float32 waveform], sample_rate)`` per text, in input order; each utterance follows exactly the
        single-utterance semantics of :meth:`generate_voice_clone`, nucleus sampling (``top_p < 1``) included."""
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        prepared = self._prepare_clone_batch(texts, language, ref_audio, ref_text, xvec_only, nsm, append_silence, instruct,
                                             voice_clone_prompt)
        return self._run_batch_full(prepared, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                               repetition_penalty), lanes, len(texts), seeds=seeds,
                                    outputs=self._batch_outputs(output, len(texts)))

    @torch.inference_mode()
    def generate_voice_clone_batch_streaming(self, texts: List[str], language: Union[str, List[str]] = "English",
                                             ref_audio: Optional[Union[str, Path]] = None, ref_text: str = "",
                                             max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9,
                                             top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                             repetition_penalty: float = 1.05, chunk_size: int = 12, xvec_only: bool = False,
                                             non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                                             instruct: Optional[str] = None,
                                             voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                             lanes: int = 8, seeds=None, output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """Streaming AND batched: the texts decode in lock-step lanes (as :meth:`generate_voice_clone_batch`) and every
        ``chunk_size`` frames of any utterance yield ``(text_index, audio_chunk, sample_rate, timing)`` -- per utterance
        exactly the chunks :meth:`generate_voice_clone_streaming` would produce for it (same windowing state machine).
        ``timing``: ``chunk_index``, ``total_steps_so_far``, ``is_final``.  ``max_new_tokens``: one value, or a list with one per
        text (all batch entry points)."""
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        prepared = self._prepare_clone_batch(texts, language, ref_audio, ref_text, xvec_only, nsm, append_silence, instruct,
                                             voice_clone_prompt)
        yield from self._run_batch_streaming(prepared, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                         do_sample, repetition_penalty), chunk_size, lanes,
                                             seeds=seeds, count=len(texts), outputs=self._batch_outputs(output, len(texts)))

    def _prepare_custom_batch(self, texts, speaker, language, instruct, non_streaming_mode):
        n = len(texts)
        spks, langs, inss = self._per_text(speaker, n, "speaker"), self._per_text(language, n, "language"), self._per_text(instruct, n, "instruct")
        if self.model.model.tts_model_type != "custom_voice":
            raise ValueError("Loaded model does not support custom voice generation")
        self.model._validate_languages(langs)                                # every argument error before anything is decoded
        self.model._validate_speakers(spks)

        def gen():
            for text, spk, lang, ins in zip(texts, spks, langs, inss):
                _m, talker, config, tie, tam, tth, tpe = self._custom_prepare(text, spk, lang, ins, non_streaming_mode)
                yield talker, config, tie, tam, tth, tpe, None
        return gen()

    @torch.inference_mode()
    def generate_custom_voice_batch(self, texts: List[str], speaker: Union[str, List[str]], language: Union[str, List[str]] = "English",
                                    instruct: Optional[Union[str, List[Optional[str]]]] = None,
                                    non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                    temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                    repetition_penalty: float = 1.05, lanes: int = 16, seeds=None, output=None) -> List[Tuple[list, int]]:
        """CustomVoice for several texts (BASELINE configs[3]: many concurrent utterances of a CustomVoice model): every
        utterance is prepared exactly like :meth:`generate_custom_voice` (speaker-id prompt, model.py:1139-1326; ``speaker`` /
        ``language`` / ``instruct`` may be one value or one per text) and up to ``lanes`` of them decode in lock-step over one pass of
        the weights per frame.  Returns one ``([waveform], sample_rate)`` per text, in input order."""
        prepared = self._prepare_custom_batch(texts, speaker, language, instruct, non_streaming_mode)
        return self._run_batch_full(prepared, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                               repetition_penalty), lanes, len(texts), seeds=seeds,
                                    outputs=self._batch_outputs(output, len(texts)))

    @torch.inference_mode()
    def generate_custom_voice_batch_streaming(self, texts: List[str], speaker: Union[str, List[str]],
                                              language: Union[str, List[str]] = "English",
                                              instruct: Optional[Union[str, List[Optional[str]]]] = None,
                                              non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                              min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                                              do_sample: bool = True, repetition_penalty: float = 1.05, chunk_size: int = 12,
                                              lanes: int = 16, seeds=None, output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """Streaming form of :meth:`generate_custom_voice_batch`: ``(text_index, audio_chunk, sample_rate, timing)`` per chunk."""
        prepared = self._prepare_custom_batch(texts, speaker, language, instruct, non_streaming_mode)
        yield from self._run_batch_streaming(prepared, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                         do_sample, repetition_penalty), chunk_size, lanes,
                                             seeds=seeds, count=len(texts), outputs=self._batch_outputs(output, len(texts)))

    @torch.inference_mode()
    def generate_voice_design_batch(self, texts: List[str], instruct: Union[str, List[str]], language: Union[str, List[str]] = "English",
                                    non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                    temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                    repetition_penalty: float = 1.05, lanes: int = 16, seeds=None, output=None) -> List[Tuple[list, int]]:
        """VoiceDesign for several texts in lock-step lanes; every utterance prepared like :meth:`generate_voice_design`."""
        return self._run_batch_full(self._prepare_design_batch(texts, instruct, language, non_streaming_mode),
                                    self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample, repetition_penalty),
                                    lanes, len(texts), seeds=seeds,
                                    outputs=self._batch_outputs(output, len(texts)))

    def _prepare_design_batch(self, texts, instruct, language, non_streaming_mode):
        n = len(texts)
        inss, langs = self._per_text(instruct, n, "instruct"), self._per_text(language, n, "language")
        if self.model.model.tts_model_type != "voice_design":
            raise ValueError("Loaded model does not support voice design generation")
        self.model._validate_languages(langs)

        def gen():
            for text, ins, lang in zip(texts, inss, langs):
                _m, talker, config, tie, tam, tth, tpe = self._design_prepare(text, ins, lang, non_streaming_mode)
                yield talker, config, tie, tam, tth, tpe, None
        return gen()

    @torch.inference_mode()
    def generate_voice_design_batch_streaming(self, texts: List[str], instruct: Union[str, List[str]],
                                              language: Union[str, List[str]] = "English", non_streaming_mode: Optional[bool] = None,
                                              max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9,
                                              top_k: int = 50, top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                              chunk_size: int = 12, lanes: int = 16, seeds=None, output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """Streaming form of :meth:`generate_voice_design_batch`: ``(text_index, audio_chunk, sample_rate, timing)`` per chunk."""
        prepared = self._prepare_design_batch(texts, instruct, language, non_streaming_mode)
        yield from self._run_batch_streaming(prepared, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                         do_sample, repetition_penalty), chunk_size, lanes,
                                             seeds=seeds, count=len(texts), outputs=self._batch_outputs(output, len(texts)))

    @torch.inference_mode()
    def generate_voice_clone_streaming(self, text: str, language: str, ref_audio: Optional[Union[str, Path]] = None,
                                       ref_text: str = "", max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                       temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                                       do_sample: bool = True, repetition_penalty: float = 1.05, chunk_size: int = 12,
                                       xvec_only: bool = False, non_streaming_mode: Optional[bool] = None,
                                       append_silence: bool = True, parity_mode: bool = False,
                                       instruct: Optional[str] = None, ref_spk: Optional[Union[str, Path]] = None,
                                       ref_rvq: Optional[Union[str, Path]] = None,
                                       ref_spk_emb: Optional[np.ndarray] = None, ref_codes: Optional[np.ndarray] = None,
                                       voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                       ) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        """Yields ``(audio_chunk, sample_rate, timing)`` every ``chunk_size`` codec frames."""
        self._reject_ggml_cached_reference_args(ref_spk=ref_spk, ref_rvq=ref_rvq, ref_spk_emb=ref_spk_emb,
                                                ref_codes=ref_codes)
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        m, talker, config, tie, tam, tth, tpe, rc = self._prepare_generation(
            text=text, language=language, ref_audio=ref_audio, ref_text=ref_text, xvec_only=xvec_only,
            non_streaming_mode=nsm, append_silence=append_silence, voice_clone_prompt=voice_clone_prompt,
            instruct=instruct)
        yield from self._run_streaming(m, talker, config, tie, tam, tth, tpe, rc,
                                       self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                        do_sample, repetition_penalty), chunk_size, parity_mode)

    def _custom_prepare(self, text, speaker, language, instruct, non_streaming_mode, input_ids=None):
        if self.model.model.tts_model_type != "custom_voice":
            raise ValueError("Loaded model does not support custom voice generation")
        self.model._validate_languages([language])
        self.model._validate_speakers([speaker])
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=True)
        if self.model.model.tts_model_size in "0b6":        # 0.6B CustomVoice ignores instruct (model.py:1166-1167)
            instruct = None
        return self._prepare_generation_custom(text=text, language=language, speaker=speaker, instruct=instruct,
                                               non_streaming_mode=nsm, input_ids=input_ids)

    @torch.inference_mode()
    def generate_custom_voice(self, text: str, speaker: str, language: str, instruct: Optional[str] = None,
                              non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                              min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                              do_sample: bool = True, repetition_penalty: float = 1.05) -> Tuple[list, int]:
        m, talker, config, tie, tam, tth, tpe = self._custom_prepare(text, speaker, language, instruct, non_streaming_mode)
        return self._run_full(m, talker, config, tie, tam, tth, tpe, None,
                              self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                               repetition_penalty))

    @torch.inference_mode()
    def generate_custom_voice_streaming(self, text: str, speaker: str, language: str, instruct: Optional[str] = None,
                                        non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                        min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                                        top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                        chunk_size: int = 12) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        m, talker, config, tie, tam, tth, tpe = self._custom_prepare(text, speaker, language, instruct, non_streaming_mode)
        yield from self._run_streaming(m, talker, config, tie, tam, tth, tpe, None,
                                       self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                        do_sample, repetition_penalty), chunk_size)

    def _design_prepare(self, text, instruct, language, non_streaming_mode, input_ids=None):
        if self.model.model.tts_model_type != "voice_design":
            raise ValueError("Loaded model does not support voice design generation")
        self.model._validate_languages([language])
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=True)
        return self._prepare_generation_custom(text=text, language=language, speaker=None, instruct=instruct,
                                               non_streaming_mode=nsm, input_ids=input_ids)

    @torch.inference_mode()
    def generate_voice_design(self, text: str, instruct: str, language: str, non_streaming_mode: Optional[bool] = None,
                              max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9,
                              top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                              repetition_penalty: float = 1.05) -> Tuple[list, int]:
        m, talker, config, tie, tam, tth, tpe = self._design_prepare(text, instruct, language, non_streaming_mode)
        return self._run_full(m, talker, config, tie, tam, tth, tpe, None,
                              self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                               repetition_penalty))

    @torch.inference_mode()
    def generate_voice_design_streaming(self, text: str, instruct: str, language: str,
                                        non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                        min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                                        top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                        chunk_size: int = 12) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        m, talker, config, tie, tam, tth, tpe = self._design_prepare(text, instruct, language, non_streaming_mode)
        yield from self._run_streaming(m, talker, config, tie, tam, tth, tpe, None,
                                       self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                        do_sample, repetition_penalty), chunk_size)

    # ---- long form (extension: a text of any length; fq3hip/long_form.py) --------------------------------
    def _long_setup(self, text, long_form):
        """-> (LongFormSpec, segments): every argument error before anything is prepared or decoded"""
        from .long_form import LongFormSpec
        spec = LongFormSpec() if long_form is None else long_form
        if not isinstance(spec, LongFormSpec):
            raise ValueError(f"long_form must be a LongFormSpec or None, not {type(long_form).__name__}")
        if getattr(self.model.model, "tts_model_type", None) == "voice_design":
            raise ValueError("long form is not offered for voice-design models: every segment would sample its own voice from the "
                             "description, so the voice would change between segments (use a clone or a custom voice)")
        if not isinstance(text, str) or not text.strip():
            raise ValueError("long form needs a text that is not empty")
        segs = spec.split(text)
        # the join stage's own range checks (host only), so that they too surface before the decode
        from .long_form import join_bound
        join_bound(self.sample_rate, spec.threshold, spec.lead_hops, spec.tail_hops, spec.hold_hops, 0, 0)
        return spec, segs

    def _long_chain(self, spec, segs, stream, level_hops: Optional[int] = None, output=None):
        """The request's ONE output stream: the join stage and, inside ``audio_output`` (or with ``output``, a text's spec in the
        many-text form), the chain behind it, all on ``stream``."""
        from .long_form import OrderedJoin, SegmentJoin
        dev = torch.device(self.device) if not isinstance(self.device, torch.device) else self.device
        join = SegmentJoin.from_spec(spec, self.sample_rate, dev, stream=stream)
        chain = None
        output = self._audio_spec if output is None else output
        if output is not None:
            from .audio_out import AudioOut
            chain = AudioOut(output, self.sample_rate, join.dev, stream)
        pauses = [spec.pause_samples(s.pause, self.sample_rate) for s in segs]
        oj = OrderedJoin(join, pauses, chain)
        oj.gains = self._gain_tensor(join.dev)                     # fixed_gain: every joined piece times the one factor
        if getattr(self, "_limit", None) is not None:
            from .limiter import Limiter
            oj.limiter = Limiter(self._limit, self.sample_rate, join.dev, stream)      # behind the join and the gains, one stream
        if getattr(self, "_lvl", None) is not None:
            from .leveller import Leveller
            # behind the join and the gains, in front of the limiter: ONE leveller for the joined stream
            oj.leveller = Leveller(self._lvl, self.sample_rate, join.dev, stream, capacity_hops=max(level_hops or 0, 4096))
        self._last_levelled = oj.leveller
        return oj, chain

    def _long_level_hops(self, spec, segs, gen_kwargs) -> Optional[int]:
        """Inside ``leveller()``: the hops the joined stream of a long-form request can have -- every segment at its frame limit plus
        its pause -- so that the one leveller is made large enough; ``ValueError`` beyond 2^20 hops, before anything decodes."""
        if getattr(self, "_lvl", None) is None:
            return None
        from .leveller import capacity_for
        tok = self.model.model.speech_tokenizer
        frames = self._frame_limit(gen_kwargs)
        per_seg = int(tok.num_samples_total(frames)) if hasattr(tok, "num_samples_total") else frames * (self.sample_rate * 2 // 25)
        total = sum(per_seg + spec.pause_samples(s.pause, self.sample_rate) for s in segs)
        return capacity_for(total, self.sample_rate)

    def _run_long_full(self, prepared, segs, spec, gen_kwargs, lanes: int) -> Tuple[list, int]:
        """The segments as the requests of one lock-step run, whole waveforms kept on the device, joined in text order on the side
        vocoder's stream, then (inside ``audio_output``) through the one-shot output stage as ONE utterance."""
        n = len(segs)
        level_hops = self._long_level_hops(spec, segs, gen_kwargs)
        outs, voc = self._run_batch_full(prepared, gen_kwargs, lanes, n, seeds=getattr(self, "_seed", None), device_audio=True)
        oj, _chain = self._long_chain(spec, segs, voc.stream, level_hops)
        oj.audio_out = None                                         # the whole stream goes through _one_shot_output below
        parts = []
        with (torch.cuda.stream(voc.stream) if voc.stream is not None else contextlib.nullcontext()):
            if self._loud is not None:
                oj.gains = [None] * n
            for k, (wavs, _sr) in enumerate(outs):
                w = wavs[0]
                w = w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(oj.join.dev)
                if self._loud is not None:
                    # the segment's RAW waveform is measured; its gain scales what the join emits for it (the join sees raw samples)
                    from .loudness import gain_of
                    oj.gains[k] = gain_of(self._measure(w.reshape(-1).contiguous(), k, voc.stream))
                parts.extend(y for _k, y, _e in oj.feed(k, w, True))
            pcm = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=oj.join.dev)
            if self._audio_spec is not None:
                a, sr = self._one_shot_output(pcm)
                return [a], sr
            return [pcm.cpu().numpy()], self.sample_rate

    def _run_long_streaming(self, prepared, segs, spec, gen_kwargs, chunk_size: int, lanes: int):
        """Streaming form: the chunks of the lanes' utterances stay device tensors on the vocoder stream; the chunks of segment k + 1
        wait until segment k has ended; what leaves is one stream in text order.  Segment 0 streams as it decodes."""
        n = len(segs)
        self._refuse_streaming_loudness()
        tok = self.model.model.speech_tokenizer
        side = self._vocoder_stream(tok)
        oj, chain = self._long_chain(spec, segs, side, self._long_level_hops(spec, segs, gen_kwargs))
        sr = chain.out_rate if chain is not None else self.sample_rate
        header = chain is not None and chain.flac
        index = 0
        ctx = (lambda: torch.cuda.stream(side)) if side is not None else contextlib.nullcontext
        for rid, audio, _sr, tm in self._run_batch_streaming(prepared, gen_kwargs, chunk_size, lanes,
                                                             seeds=getattr(self, "_seed", None), count=n, device_audio=True):
            with ctx():
                pcm = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(oj.join.dev)
                pieces = [(k, y.cpu().numpy(), ended) for k, y, ended in oj.feed(rid, pcm, bool(tm.get("is_final")))]
            for k, host, ended in pieces:
                if host.size == 0 and not ended:
                    continue                                       # a chunk the join stage removed whole (or holds back)
                if header:
                    host, header = np.concatenate([np.frombuffer(chain.header(), dtype=np.uint8), host]), False
                yield host, sr, dict(segment_index=k, n_segments=n, chunk_index=index, is_final=ended,
                                     total_steps_so_far=int(tm.get("total_steps_so_far", 0)))
                index += 1

    @torch.inference_mode()
    def generate_long_voice_clone(self, text: str, language: str, ref_audio: Optional[Union[str, Path]] = None,
                                  ref_text: str = "", max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                  temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                  repetition_penalty: float = 1.05, xvec_only: bool = False,
                                  non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                                  instruct: Optional[str] = None, ref_spk: Optional[Union[str, Path]] = None,
                                  ref_rvq: Optional[Union[str, Path]] = None, ref_spk_emb: Optional[np.ndarray] = None,
                                  ref_codes: Optional[np.ndarray] = None,
                                  voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                  lanes: int = 16, long_form=None) -> Tuple[list, int]:
        """Voice cloning of a text of any length: ``long_form`` (a ``LongFormSpec``; None: the defaults) cuts it into segments, up to
        ``lanes`` of them decode side by side (``max_new_tokens`` is per segment), and their waveforms are joined on the device --
        leading and trailing silence removed, a pause per boundary -- into one ``([waveform], sample_rate)``.  Works inside
        ``audio_output`` (one stream: join -> time-scale -> resample / encode -> FLAC; pauses scale with ``speed``) and ``seeded``
        (segment i samples with seed + i)."""
        self._reject_ggml_cached_reference_args(ref_spk=ref_spk, ref_rvq=ref_rvq, ref_spk_emb=ref_spk_emb, ref_codes=ref_codes)
        spec, segs = self._long_setup(text, long_form)
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        prepared = self._prepare_clone_batch([s.text for s in segs], language, ref_audio, ref_text, xvec_only, nsm, append_silence,
                                             instruct, voice_clone_prompt)
        return self._run_long_full(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                          do_sample, repetition_penalty), lanes)

    @torch.inference_mode()
    def generate_long_voice_clone_streaming(self, text: str, language: str, ref_audio: Optional[Union[str, Path]] = None,
                                            ref_text: str = "", max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                            temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                            repetition_penalty: float = 1.05, chunk_size: int = 12, xvec_only: bool = False,
                                            non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                                            instruct: Optional[str] = None, ref_spk: Optional[Union[str, Path]] = None,
                                            ref_rvq: Optional[Union[str, Path]] = None, ref_spk_emb: Optional[np.ndarray] = None,
                                            ref_codes: Optional[np.ndarray] = None,
                                            voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                            lanes: int = 16, long_form=None) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        """Streaming form of :meth:`generate_long_voice_clone`: yields ``(audio_chunk, sample_rate, timing)`` strictly in text order;
        ``timing``: ``segment_index``, ``n_segments``, ``chunk_index``, ``is_final``."""
        self._reject_ggml_cached_reference_args(ref_spk=ref_spk, ref_rvq=ref_rvq, ref_spk_emb=ref_spk_emb, ref_codes=ref_codes)
        spec, segs = self._long_setup(text, long_form)
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        prepared = self._prepare_clone_batch([s.text for s in segs], language, ref_audio, ref_text, xvec_only, nsm, append_silence,
                                             instruct, voice_clone_prompt)
        yield from self._run_long_streaming(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k,
                                                                                   top_p, do_sample, repetition_penalty), chunk_size, lanes)

    @torch.inference_mode()
    def generate_long_custom_voice(self, text: str, speaker: str, language: str, instruct: Optional[str] = None,
                                   non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                   min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                                   do_sample: bool = True, repetition_penalty: float = 1.05, lanes: int = 16,
                                   long_form=None) -> Tuple[list, int]:
        """CustomVoice for a text of any length; see :meth:`generate_long_voice_clone`."""
        spec, segs = self._long_setup(text, long_form)
        prepared = self._prepare_custom_batch([s.text for s in segs], speaker, language, instruct, non_streaming_mode)
        return self._run_long_full(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                          do_sample, repetition_penalty), lanes)

    @torch.inference_mode()
    def generate_long_custom_voice_streaming(self, text: str, speaker: str, language: str, instruct: Optional[str] = None,
                                             non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                             min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                                             top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                             chunk_size: int = 12, lanes: int = 16,
                                             long_form=None) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        """Streaming form of :meth:`generate_long_custom_voice`."""
        spec, segs = self._long_setup(text, long_form)
        prepared = self._prepare_custom_batch([s.text for s in segs], speaker, language, instruct, non_streaming_mode)
        yield from self._run_long_streaming(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k,
                                                                                   top_p, do_sample, repetition_penalty), chunk_size, lanes)

    # ---- long form for many texts: the segments of all texts share the lanes of ONE lock-step run ------
    def _long_batch_setup(self, texts, long_form, seeds, output):
        """-> (spec, [segments per text], the requests' seeds, the texts' output specs or None): every argument error, each text's
        ``_long_setup`` included, before anything is prepared or decoded.  The requests are queued text by text; segment ``k`` of a
        text with seed ``s`` samples with ``s + k``, as ``seeded(s)`` gives the single-text call."""
        if isinstance(texts, str) or not isinstance(texts, (list, tuple)) or not texts:
            raise ValueError("texts must be a list of texts that is not empty")
        self._refuse_batch_audio_output()
        outputs = self._batch_outputs(output, len(texts))
        spec, segs = None, []
        for text in texts:
            spec, s = self._long_setup(text, long_form)
            segs.append(s)
        per_text = expand_seeds(seeds, len(texts))
        req_seeds = [None if s is None else (s + k) % 2 ** 64 for s, sg in zip(per_text, segs) for k in range(len(sg))]
        return spec, segs, (req_seeds if seeds is not None else None), outputs

    def _long_batch_chains(self, spec, segs, stream, gen_kwargs, outputs):
        """one ordered join and chain per text, all on ``stream`` -> (``OrderedJoinSet``, the chains)"""
        from .long_form import OrderedJoinSet
        pairs = [self._long_chain(spec, sg, stream, self._long_level_hops(spec, sg, gen_kwargs), None if outputs is None else outputs[t])
                 for t, sg in enumerate(segs)]
        return OrderedJoinSet([oj for oj, _c in pairs]), [c for _oj, c in pairs]

    def _run_long_batch_full(self, prepared, segs, spec, gen_kwargs, lanes: int, seeds, outputs) -> List[Tuple[list, int]]:
        """``_run_long_full`` over many texts: one lock-step run over every segment of every text; round ``k`` joins segment ``k`` of
        every text that has one in ONE group call on the side vocoder's stream."""
        counts = [len(sg) for sg in segs]
        base = [sum(counts[:t]) for t in range(len(segs))]
        outs, voc = self._run_batch_full(prepared, gen_kwargs, lanes, sum(counts), seeds=seeds, device_audio=True)
        ojs, _chains = self._long_batch_chains(spec, segs, voc.stream, gen_kwargs, outputs)
        parts: List[list] = [[] for _ in segs]
        with (torch.cuda.stream(voc.stream) if voc.stream is not None else contextlib.nullcontext()):
            for oj in ojs.ordered:
                oj.audio_out = None                                 # every text's whole stream goes through a one-shot stage below
                if self._loud is not None:
                    oj.gains = [None] * oj.n
            for k in range(max(counts)):
                rows = []
                for t, oj in enumerate(ojs.ordered):
                    if k >= counts[t]:
                        continue
                    w = outs[base[t] + k][0][0]
                    w = w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(oj.join.dev)
                    if self._loud is not None:
                        from .loudness import gain_of
                        oj.gains[k] = gain_of(self._measure(w.reshape(-1).contiguous(), base[t] + k, voc.stream))
                    rows.append((t, k, w, True))
                for t, _k, y, _ended in ojs.feed_group(rows):
                    parts[t].append(y)
            result = []
            for t, oj in enumerate(ojs.ordered):
                pcm = torch.cat(parts[t]) if parts[t] else torch.zeros(0, dtype=torch.float32, device=oj.join.dev)
                if outputs is not None and outputs[t] is not None:
                    a, sr = self._one_shot_output(pcm, outputs[t])
                    result.append(([a], sr))
                else:
                    result.append(([pcm.cpu().numpy()], self.sample_rate))
            return result

    def _run_long_batch_streaming(self, prepared, segs, spec, gen_kwargs, chunk_size: int, lanes: int, seeds, outputs):
        """``_run_long_streaming`` over many texts: the chunks a poll of the lock-step run hands out together go through ONE
        ``feed_group``; every text's audio leaves in text order, the texts interleave as they become ready."""
        self._refuse_streaming_loudness()
        counts = [len(sg) for sg in segs]
        where = [(t, k) for t, n in enumerate(counts) for k in range(n)]
        tok = self.model.model.speech_tokenizer
        side = self._vocoder_stream(tok)
        ojs, chains = self._long_batch_chains(spec, segs, side, gen_kwargs, outputs)
        rates = [c.out_rate if c is not None else self.sample_rate for c in chains]
        header = [c is not None and c.flac for c in chains]
        index = [0] * len(segs)
        dev = ojs.ordered[0].join.dev
        ctx = (lambda: torch.cuda.stream(side)) if side is not None else contextlib.nullcontext

        def settle(group, steps):
            with ctx():
                rows = [(t, k, a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev), last)
                        for t, k, a, last in group]
                got = ojs.feed_group(rows)
                # every piece of the group in ONE device buffer (16-byte aligned, whatever each text's encoding) and ONE copy
                offs, total = [], 0
                for _t, _k, y, _e in got:
                    offs.append(total)
                    total += (int(y.numel()) * y.element_size() + 15) // 16 * 16
                buf = torch.empty(total, dtype=torch.uint8, device=dev)
                for o, (_t, _k, y, _e) in zip(offs, got):
                    if y.numel():
                        buf[o: o + int(y.numel()) * y.element_size()] = y.contiguous().reshape(-1).view(torch.uint8)
                host_all = buf.cpu().numpy()
                pieces = [(t, k, host_all[o: o + int(y.numel()) * y.element_size()].view(torch.empty(0, dtype=y.dtype).numpy().dtype), ended)
                          for o, (t, k, y, ended) in zip(offs, got)]
            for t, k, host, ended in pieces:
                if host.size == 0 and not ended:
                    continue                                       # a chunk the join stage removed whole (or holds back)
                if header[t]:
                    host, header[t] = np.concatenate([np.frombuffer(chains[t].header(), dtype=np.uint8), host]), False
                yield t, host, rates[t], dict(segment_index=k, n_segments=counts[t], chunk_index=index[t], is_final=ended,
                                              total_steps_so_far=steps)
                index[t] += 1

        group, steps = [], 0
        for rid, audio, _sr, tm in self._run_batch_streaming(prepared, gen_kwargs, chunk_size, lanes, seeds=seeds, count=len(where),
                                                             device_audio=True, group_marks=True):
            t, k = where[rid]
            group.append((t, k, audio, bool(tm.get("is_final"))))
            steps = int(tm.get("total_steps_so_far", 0))
            if tm.get("group_end"):
                yield from settle(group, steps)
                group = []
        if group:
            yield from settle(group, steps)

    def _prepare_long_batch(self, segs, prepare_text):
        """the requests of every text's segments, text by text; ``prepare_text(t, [segment texts])`` -> that text's prepared requests"""
        import itertools
        return itertools.chain.from_iterable([prepare_text(t, [s.text for s in sg]) for t, sg in enumerate(segs)])

    @torch.inference_mode()
    def generate_long_voice_clone_batch(self, texts: List[str], language: Union[str, List[str]],
                                        ref_audio: Optional[Union[str, Path]] = None,
                                        ref_text: str = "", max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                        temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                        repetition_penalty: float = 1.05, xvec_only: bool = False,
                                        non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                                        instruct: Optional[str] = None, ref_spk: Optional[Union[str, Path]] = None,
                                        ref_rvq: Optional[Union[str, Path]] = None, ref_spk_emb: Optional[np.ndarray] = None,
                                        ref_codes: Optional[np.ndarray] = None,
                                        voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                        lanes: int = 16, long_form=None, seeds=None, output=None) -> List[Tuple[list, int]]:
        """:meth:`generate_long_voice_clone` for many texts in ONE lock-step run: every segment of every text is a request, queued
        text by text, and a lane that finishes one takes the next, whichever text it belongs to.  One ``([waveform], sample_rate)``
        per text, in input order; text ``t`` equals the single-text call inside ``seeded(seeds[t])``.  ``seeds`` (a list, or an int
        ``s``: text ``t`` gets ``s + t``) and ``output`` (an ``AudioOutSpec``, or one or None per text) as on the ``*_batch`` entry
        points, per TEXT; ``language`` may be one per text."""
        self._reject_ggml_cached_reference_args(ref_spk=ref_spk, ref_rvq=ref_rvq, ref_spk_emb=ref_spk_emb, ref_codes=ref_codes)
        spec, segs, req_seeds, outputs = self._long_batch_setup(texts, long_form, seeds, output)
        langs = self._per_text(language, len(texts), "language")
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        prepared = self._prepare_long_batch(segs, lambda t, ts: self._prepare_clone_batch(
            ts, langs[t], ref_audio, ref_text, xvec_only, nsm, append_silence, instruct, voice_clone_prompt))
        return self._run_long_batch_full(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                                do_sample, repetition_penalty), lanes, req_seeds, outputs)

    @torch.inference_mode()
    def generate_long_voice_clone_batch_streaming(self, texts: List[str], language: Union[str, List[str]],
                                                  ref_audio: Optional[Union[str, Path]] = None,
                                                  ref_text: str = "", max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                                  temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                                  repetition_penalty: float = 1.05, chunk_size: int = 12, xvec_only: bool = False,
                                                  non_streaming_mode: Optional[bool] = None, append_silence: bool = True,
                                                  instruct: Optional[str] = None, ref_spk: Optional[Union[str, Path]] = None,
                                                  ref_rvq: Optional[Union[str, Path]] = None, ref_spk_emb: Optional[np.ndarray] = None,
                                                  ref_codes: Optional[np.ndarray] = None,
                                                  voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                                  lanes: int = 16, long_form=None, seeds=None,
                                                  output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """Streaming form of :meth:`generate_long_voice_clone_batch`: yields ``(text_index, audio_chunk, sample_rate, info)``;
        ``info``: ``segment_index``, ``n_segments``, ``chunk_index``, ``is_final`` (all per text) and ``total_steps_so_far``.  The
        audio of one text leaves strictly in text order; the texts interleave as they become ready.  ``flac``: the stream header
        comes in front of a text's first piece."""
        self._reject_ggml_cached_reference_args(ref_spk=ref_spk, ref_rvq=ref_rvq, ref_spk_emb=ref_spk_emb, ref_codes=ref_codes)
        self._refuse_streaming_loudness()
        spec, segs, req_seeds, outputs = self._long_batch_setup(texts, long_form, seeds, output)
        langs = self._per_text(language, len(texts), "language")
        nsm = self._resolve_non_streaming_mode(non_streaming_mode, default=False)
        prepared = self._prepare_long_batch(segs, lambda t, ts: self._prepare_clone_batch(
            ts, langs[t], ref_audio, ref_text, xvec_only, nsm, append_silence, instruct, voice_clone_prompt))
        yield from self._run_long_batch_streaming(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k,
                                                                                         top_p, do_sample, repetition_penalty),
                                                  chunk_size, lanes, req_seeds, outputs)

    @torch.inference_mode()
    def generate_long_custom_voice_batch(self, texts: List[str], speaker: Union[str, List[str]], language: Union[str, List[str]],
                                         instruct: Optional[str] = None,
                                         non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                         min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                                         do_sample: bool = True, repetition_penalty: float = 1.05, lanes: int = 16,
                                         long_form=None, seeds=None, output=None) -> List[Tuple[list, int]]:
        """CustomVoice for many texts of any length; see :meth:`generate_long_voice_clone_batch`.  ``speaker`` and ``language`` may
        be one per text."""
        spec, segs, req_seeds, outputs = self._long_batch_setup(texts, long_form, seeds, output)
        spk, langs = self._per_text(speaker, len(texts), "speaker"), self._per_text(language, len(texts), "language")
        prepared = self._prepare_long_batch(segs, lambda t, ts: self._prepare_custom_batch(ts, spk[t], langs[t], instruct, non_streaming_mode))
        return self._run_long_batch_full(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p,
                                                                                do_sample, repetition_penalty), lanes, req_seeds, outputs)

    @torch.inference_mode()
    def generate_long_custom_voice_batch_streaming(self, texts: List[str], speaker: Union[str, List[str]],
                                                   language: Union[str, List[str]], instruct: Optional[str] = None,
                                                   non_streaming_mode: Optional[bool] = None, max_new_tokens: int = 2048,
                                                   min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                                                   top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                                   chunk_size: int = 12, lanes: int = 16, long_form=None, seeds=None,
                                                   output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """Streaming form of :meth:`generate_long_custom_voice_batch`."""
        self._refuse_streaming_loudness()
        spec, segs, req_seeds, outputs = self._long_batch_setup(texts, long_form, seeds, output)
        spk, langs = self._per_text(speaker, len(texts), "speaker"), self._per_text(language, len(texts), "language")
        prepared = self._prepare_long_batch(segs, lambda t, ts: self._prepare_custom_batch(ts, spk[t], langs[t], instruct, non_streaming_mode))
        yield from self._run_long_batch_streaming(prepared, segs, spec, self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k,
                                                                                         top_p, do_sample, repetition_penalty),
                                                  chunk_size, lanes, req_seeds, outputs)

    # ---- incremental text (extension: the reference takes the whole text before it starts; fq3hip/text_stream.py) ---------
    @staticmethod
    def _refuse_icl_text_stream(xvec_only, voice_clone_prompt) -> str:
        """Raises for a voice that can only be served as an ICL clone; returns the message for the checks that follow the prompt build."""
        why = ("incremental text needs an x-vector-only voice: an ICL clone lays the text against the reference frames inside the "
               "prompt, so the prefill needs the whole text (use generate_voice_clone_streaming)")
        if not xvec_only and voice_clone_prompt is None:
            raise ValueError(why)
        if isinstance(voice_clone_prompt, list) and any(bool(it.icl_mode) for it in voice_clone_prompt):
            raise ValueError(why)
        if isinstance(voice_clone_prompt, dict):
            icl = voice_clone_prompt.get("icl_mode", [not bool(v) for v in voice_clone_prompt.get("x_vector_only_mode", [True])])
            if any(bool(v) for v in icl):
                raise ValueError(why)
        return why

    def _text_tokenize(self):
        """str -> token ids of a piece of the text BODY (no chat template around it)."""
        from .native_model import ByteTokenizer
        tok = self.model.tokenizer
        if isinstance(tok, ByteTokenizer):
            return lambda s: tok(s)[3:-5]
        if callable(getattr(tok, "encode", None)):
            return lambda s: list(tok.encode(s))
        return lambda s: list(tok(s)["input_ids"])

    def _text_session_ids(self, feeder):
        """Waits for the first text token; returns the ``input_ids`` of the step-by-step prompt: the chat template around that one
        token (``prompt.py`` puts token 3 into the prompt and needs nothing else of the body)."""
        first, closed = feeder.take(block=True, limit=1)
        while not first and not closed:
            first, closed = feeder.take(block=True, limit=1)
        if not first:
            raise ValueError("the text stream ended before its first token")
        shell = self.model._tokenize_texts([self.model._build_assistant_text("")])[0]
        from .prompt import host_ids
        ids = host_ids(shell)
        if len(ids) != 8:
            raise ValueError(f"the chat template around an empty text must be 3 + 5 tokens, got {len(ids)}")
        ids = ids[:3] + [int(first[0])] + ids[3:]
        tt = torch.tensor([ids], dtype=torch.long, device=self.model.device)
        tt.fq3_host_ids = (list(ids), None if tt.is_inference() else tt._version)
        return [tt]

    def _run_text_streaming(self, text_iter, prepare, gen_kwargs, chunk_size: int):
        """Shared back half of the ``stream_*`` entry points: ``prepare(input_ids)`` builds the step-by-step prompt from the first
        token; the decode loop runs behind the text as it arrives and ``StreamingVocoder`` turns each code chunk into audio."""
        from .text_stream import TextFeeder, fast_generate_text_streaming, pump_text
        self._refuse_streaming_loudness()
        if isinstance(text_iter, TextFeeder):
            feeder = text_iter
        else:
            if isinstance(text_iter, str):
                text_iter = [text_iter]
            feeder = TextFeeder(self._text_tokenize())
            pump_text(feeder, text_iter)
        try:
            m, talker, config, tie, tam, _tth, tpe = prepare(self._text_session_ids(feeder))
            tok = m.speech_tokenizer
            voc = StreamingVocoder(tok, None, chunk_size, self.device, self._vocoder_stream(tok), output=self._audio_spec, **self._exact_kw(),
                                   **self._gain_kw())
            stream = fast_generate_text_streaming(
                talker=talker, talker_input_embeds=tie, attention_mask=tam, tts_pad_embed=tpe, config=config,
                predictor_graph=self.predictor_graph, talker_graph=self.talker_graph, feeder=feeder,
                tts_eos_id=int(m.config.tts_eos_token_id), chunk_size=chunk_size, **gen_kwargs, **self._seed_kw())
            timing = None
            for chunk, timing in stream:
                ev = timing.pop("codes_ready_event", None)
                new_audio, sr = voc.push(chunk, ev, final=bool(timing.get("is_final")))
                if "first_text_ms" in timing:
                    timing["first_text_ms"] = (time.time() - feeder.t_first) * 1000      # first piece received -> first audio
                yield new_audio, sr, timing
            tail = self._tail_event(voc, timing)
            if tail is not None:
                yield tail
        finally:
            # a consumer that went away: stop the loop at the next frame boundary (frames of the look-ahead may be queued)
            eng = self.talker_graph.engine
            if torch.cuda.is_available() and getattr(eng, "ctx", None):
                eng.decode_cancel()

    @torch.inference_mode()
    def stream_custom_voice(self, text_iter, speaker: str, language: str, instruct: Optional[str] = None, chunk_size: int = 12,
                            max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                            top_p: float = 1.0, do_sample: bool = True,
                            repetition_penalty: float = 1.05) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        """``generate_custom_voice_streaming(..., non_streaming_mode=False)`` for a text that is still arriving: ``text_iter`` is any
        iterable of ``str`` pieces (a generator driven by an LLM client, a queue reader) or a ``TextFeeder``.  Decoding starts at
        the first complete word; codes and audio are those of the whole text, whatever the cuts.  The first chunk's timing has
        ``first_text_ms`` (first piece received -> first audio)."""
        def prepare(input_ids):
            m, talker, config, tie, tam, tth, tpe = self._custom_prepare(None, speaker, language, instruct, False, input_ids=input_ids)
            return m, talker, config, tie, tam, tth, tpe
        yield from self._run_text_streaming(text_iter, prepare,
                                            self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                             repetition_penalty), chunk_size)

    @torch.inference_mode()
    def stream_voice_design(self, text_iter, instruct: str, language: str, chunk_size: int = 12, max_new_tokens: int = 2048,
                            min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                            do_sample: bool = True,
                            repetition_penalty: float = 1.05) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        """``generate_voice_design_streaming(..., non_streaming_mode=False)`` for a text that is still arriving (see
        ``stream_custom_voice``)."""
        def prepare(input_ids):
            return self._design_prepare(None, instruct, language, False, input_ids=input_ids)
        yield from self._run_text_streaming(text_iter, prepare,
                                            self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                             repetition_penalty), chunk_size)

    @torch.inference_mode()
    def stream_voice_clone(self, text_iter, language: str, ref_audio: Optional[Union[str, Path]] = None, chunk_size: int = 12,
                           max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                           top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05, xvec_only: bool = True,
                           append_silence: bool = True, instruct: Optional[str] = None,
                           voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                           ) -> Generator[Tuple[np.ndarray, int, dict], None, None]:
        """``generate_voice_clone_streaming(..., non_streaming_mode=False)`` for a text that is still arriving, for x-vector-only
        voices.  An ICL voice (reference codes + reference text) is refused: there the text is laid against the reference frames
        inside the prompt, so the prefill itself needs the whole text."""
        why = self._refuse_icl_text_stream(xvec_only, voice_clone_prompt)

        def prepare(input_ids):
            m, talker, config, tie, tam, tth, tpe, rc = self._prepare_generation(
                text=None, language=language, ref_audio=ref_audio, ref_text="", xvec_only=True, non_streaming_mode=False,
                append_silence=append_silence, voice_clone_prompt=voice_clone_prompt, instruct=instruct, input_ids=input_ids)
            if rc is not None:
                raise ValueError(why)
            return m, talker, config, tie, tam, tth, tpe
        yield from self._run_text_streaming(text_iter, prepare,
                                            self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                             repetition_penalty), chunk_size)

    # ---- incremental text in the lock-step batch: many text streams, one decoder ------------------------------------------
    def _text_feeders(self, text_iters):
        from .text_stream import TextFeeder, pump_text
        feeders = []
        for it in text_iters:
            if isinstance(it, TextFeeder):
                feeders.append(it)
                continue
            f = TextFeeder(self._text_tokenize())
            pump_text(f, [it] if isinstance(it, str) else it)
            feeders.append(f)
        return feeders

    def _bind_lane_prompt_weights(self, dec):
        """The lanes of the batch scheduler project text themselves (``fq3_batch_text_append``): they borrow the text embedding and
        ``text_projection`` this model's own context is bound to."""
        keep = getattr(self.talker_graph.engine, "_prompt_keep", None)
        if keep is None:
            raise RuntimeError("incremental text needs the HIP prompt builder (this model's context has no prompt weights bound)")
        for ln in dec.lanes:
            if getattr(ln.engine, "_prompt_keep", None) is None:
                ln.engine.bind_prompt_weights(*keep)

    def text_batch_request(self, rid, feeder, prepare, gen_kwargs, seed=None):
        """The scheduler's request for a text stream whose first token exists: the step-by-step prompt around that token, an empty
        trailing table, the feeder for every later token.  ``prepare(input_ids)`` is the voice's prompt builder."""
        from .batching import BatchRequest
        m, talker, config, tie, tam, _tth, tpe = prepare(self._text_session_ids(feeder))
        return BatchRequest(rid, talker, tie, tam, tie.new_zeros(1, 0, tie.shape[-1]), tpe, config, dict(gen_kwargs),
                            text_feeder=feeder, tts_eos_id=int(m.config.tts_eos_token_id), seed=seed)

    def _run_text_batch_streaming(self, text_iters, prepares, gen_kwargs, chunk_size: int, lanes: int, seeds=None, outputs=None):
        """Shared back half of the ``stream_*_batch`` entry points.  A request enters the scheduler when its first token exists;
        streams whose first token has not arrived wait beside it and do not block the others."""
        import threading
        from collections import deque
        seeds = expand_seeds(seeds, len(text_iters))
        feeders = self._text_feeders(text_iters)
        arrived = threading.Event()
        for f in feeders:
            f.waker = arrived                                   # (the scheduler puts its own event here when it arms the lane)
        waiting = deque(range(len(feeders)))

        def rounds(dec, meta):
            self._bind_lane_prompt_weights(dec)

            def pull():
                for _ in range(len(waiting)):
                    i = waiting.popleft()
                    n, closed = feeders[i].pending()
                    if n or closed:                             # (closed and empty: _text_session_ids raises, as the single stream does)
                        meta[i] = None
                        return self.text_batch_request(i, feeders[i], prepares[i], gen_kwargs, seed=seeds[i])
                    waiting.append(i)
                return None

            while waiting:
                arrived.clear()
                if not any(sum(feeders[i].pending()) for i in waiting):
                    arrived.wait(0.05)                          # nothing decodes and no first token yet: sleep until a feeder has one
                    continue
                yield [], pull

        def stamp(i, timing):
            if timing.get("chunk_index") == 0 and feeders[i].t_first is not None:
                timing["first_text_ms"] = (time.time() - feeders[i].t_first) * 1000      # first piece received -> first audio

        yield from self._run_batch_streaming(None, gen_kwargs, chunk_size, lanes, rounds=rounds, stamp=stamp, outputs=outputs)

    @torch.inference_mode()
    def stream_custom_voice_batch(self, text_iters, speaker: Union[str, List[str]], language: Union[str, List[str]] = "English",
                                  instruct: Optional[Union[str, List[Optional[str]]]] = None, chunk_size: int = 12,
                                  max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50,
                                  top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                  lanes: int = 16, seeds=None, output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """``generate_custom_voice_batch_streaming(..., non_streaming_mode=False)`` for texts that are still arriving: every element of
        ``text_iters`` is an iterable of ``str`` pieces or a ``TextFeeder`` (an LLM's token stream per utterance), and up to ``lanes``
        of them decode in lock-step while their text comes in.  Yields ``(index, audio_chunk, sample_rate, timing)``; per utterance the
        chunks are those of the whole text, whatever the cuts and their timing.  The first chunk's timing has ``first_text_ms``."""
        n = len(text_iters)
        spks, langs, inss = self._per_text(speaker, n, "speaker"), self._per_text(language, n, "language"), self._per_text(instruct, n, "instruct")
        if self.model.model.tts_model_type != "custom_voice":
            raise ValueError("Loaded model does not support custom voice generation")
        self.model._validate_languages(langs)
        self.model._validate_speakers(spks)

        def prep(spk, lang, ins):
            return lambda input_ids: self._custom_prepare(None, spk, lang, ins, False, input_ids=input_ids)
        yield from self._run_text_batch_streaming(text_iters, [prep(*a) for a in zip(spks, langs, inss)],
                                                  self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                                   repetition_penalty), chunk_size, lanes, seeds=seeds,
                                                  outputs=self._batch_outputs(output, len(text_iters)))

    @torch.inference_mode()
    def stream_voice_design_batch(self, text_iters, instruct: Union[str, List[str]], language: Union[str, List[str]] = "English",
                                  chunk_size: int = 12, max_new_tokens: int = 2048, min_new_tokens: int = 2, temperature: float = 0.9,
                                  top_k: int = 50, top_p: float = 1.0, do_sample: bool = True, repetition_penalty: float = 1.05,
                                  lanes: int = 16, seeds=None, output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """``generate_voice_design_batch_streaming(..., non_streaming_mode=False)`` for texts that are still arriving (see
        :meth:`stream_custom_voice_batch`)."""
        n = len(text_iters)
        inss, langs = self._per_text(instruct, n, "instruct"), self._per_text(language, n, "language")
        if self.model.model.tts_model_type != "voice_design":
            raise ValueError("Loaded model does not support voice design generation")
        self.model._validate_languages(langs)

        def prep(ins, lang):
            return lambda input_ids: self._design_prepare(None, ins, lang, False, input_ids=input_ids)
        yield from self._run_text_batch_streaming(text_iters, [prep(*a) for a in zip(inss, langs)],
                                                  self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                                   repetition_penalty), chunk_size, lanes, seeds=seeds,
                                                  outputs=self._batch_outputs(output, len(text_iters)))

    @torch.inference_mode()
    def stream_voice_clone_batch(self, text_iters, language: Union[str, List[str]] = "English",
                                 ref_audio: Optional[Union[str, Path]] = None, chunk_size: int = 12, max_new_tokens: int = 2048,
                                 min_new_tokens: int = 2, temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                                 do_sample: bool = True, repetition_penalty: float = 1.05, xvec_only: bool = True,
                                 append_silence: bool = True, instruct: Optional[str] = None,
                                 voice_clone_prompt: Optional[Union[Dict[str, Any], List[Any]]] = None,
                                 lanes: int = 16, seeds=None, output=None) -> Generator[Tuple[int, np.ndarray, int, dict], None, None]:
        """``generate_voice_clone_batch_streaming(..., non_streaming_mode=False)`` for texts that are still arriving, one x-vector-only
        voice for all of them.  An ICL voice is refused with the message of :meth:`stream_voice_clone`."""
        why = self._refuse_icl_text_stream(xvec_only, voice_clone_prompt)
        langs = self._per_text(language, len(text_iters), "language")

        def prep(lang):
            def prepare(input_ids):
                m, talker, config, tie, tam, tth, tpe, rc = self._prepare_generation(
                    text=None, language=lang, ref_audio=ref_audio, ref_text="", xvec_only=True, non_streaming_mode=False,
                    append_silence=append_silence, voice_clone_prompt=voice_clone_prompt, instruct=instruct, input_ids=input_ids)
                if rc is not None:
                    raise ValueError(why)
                return m, talker, config, tie, tam, tth, tpe
            return prepare
        yield from self._run_text_batch_streaming(text_iters, [prep(l) for l in langs],
                                                  self._gen_kwargs(max_new_tokens, min_new_tokens, temperature, top_k, top_p, do_sample,
                                                                   repetition_penalty), chunk_size, lanes, seeds=seeds,
                                                  outputs=self._batch_outputs(output, len(text_iters)))
