#!/usr/bin/env python3
"""OpenAI-compatible speech endpoint over the MI355X path: ``POST /v1/audio/speech`` with the request schema, formats,
voice registry and streaming-WAV behaviour of the reference's ``examples/openai_server.py`` (:77-265).

What differs is the scheduling.  The reference serialises requests with one lock (``openai_server.py:71``) because its graph
objects hold a single static context.  Here there are two schedulers:

* ``lock``   one request at a time, audio streamed chunk by chunk as it is generated (the reference's behaviour);
* ``batch``  a worker thread owns the model and runs the continuous-batching decoder (``fq3hip/batching.py`` over
             ``fq3_batch_*``): requests that arrive while others are decoding join at the next frame boundary, up to
             ``lanes`` (<= 128) utterances advance in lock-step over ONE pass of the weights per frame; each response is
             sent when its utterance finishes.

With the ``batch`` scheduler a client may also send its text in pieces while the audio is already coming (an LLM's token stream
into speech): ``POST /v1/audio/speech/sessions`` -> ``{"id"}``, ``POST /v1/audio/speech/sessions/{id}/text`` with
``{"text", "final"}``, ``GET /v1/audio/speech/sessions/{id}/audio`` -> the streaming wav / pcm body of ``/v1/audio/speech``.  A
session decodes in a lane like any other request (``BatchWorker.submit_text``); it uses the voice's x-vector only.

``create_app(model, voices, ...)`` is the testable core; ``main()`` is the command line (same flags as the reference plus
``--scheduler/--lanes/--voice-cache/--synthetic``)."""
from __future__ import annotations

import argparse
import asyncio
import contextlib
import json
import logging
import math
import os
import queue
import sys
import threading
import time
import uuid
from typing import Any, AsyncGenerator, Dict, Optional

import numpy as np
from pydantic import BaseModel

from .audio_io import to_pcm16, to_wav_bytes, wav_header, wav_header_for

logger = logging.getLogger(__name__)
CONTENT_TYPES = {"wav": "audio/wav", "pcm": "audio/pcm", "mp3": "audio/mpeg", "flac": "audio/flac"}


class SpeechRequest(BaseModel):
    """examples/openai_server.py:77-82."""
    model: str = "tts-1"
    input: str
    voice: str = "alloy"
    response_format: str = "wav"          # wav | pcm | flac (compressed on the device: the s16 samples, losslessly) | mp3 (refused)
    speed: float = 1.0                     # 0.25 .. 4.0, applied on the device after the vocoder (duration changes, pitch does not)
    # extension: the device audio output stage (fq3hip/audio_out.py).  Both absent: 16-bit PCM at the model's rate, as ever
    sample_rate: Optional[int] = None      # Hz, e.g. 8000, 16000, 44100, 48000
    encoding: Optional[str] = None         # s16 | mulaw | alaw (f32 is answered as s16)
    # extension: reproducible sampling.  An integer in [0, 2^64): the same request with the same seed gives the same audio, whatever
    # else the server is doing (the noise is a pure function of (seed, frame)); the reply carries X-Seed.
    # Absent: unseeded, as ever
    seed: Optional[int] = None
    # extension: long-form synthesis (fq3hip/long_form.py; lock scheduler).  true: the text is cut into segments
    # that decode side by side and are joined on the device into ONE stream; absent: taken when the text is longer than the
    # splitter's budget (max_chars); false: never.  The reply carries X-Segments
    long_form: Optional[bool] = None


class SessionRequest(BaseModel):
    voice: str = "alloy"
    response_format: str = "wav"          # wav | pcm | flac
    speed: float = 1.0                     # as in SpeechRequest
    sample_rate: Optional[int] = None
    encoding: Optional[str] = None
    seed: Optional[int] = None             # as in SpeechRequest


class SessionText(BaseModel):
    text: str = ""
    final: bool = False


class BatchWorker:
    """One thread owns the model and runs the continuous-batching decoder in streaming mode.  ``submit`` returns a queue that
    receives the utterance's PCM chunks (``np.ndarray``) as they are vocoded, then ``BatchWorker.DONE`` -- or an exception."""

    DONE = object()

    def __init__(self, model, lanes: int = 8, chunk_size: int = 12, prefix_cache_rows: int = 0):
        from .batching import MAX_LANES
        self.model, self.lanes = model, max(1, min(int(lanes), MAX_LANES))
        # the batch scheduler's prefix KV cache (FasterQwen3TTS.enable_prefix_cache(rows, batch=True)): off by default
        self.prefix_cache = model.enable_prefix_cache(int(prefix_cache_rows), batch=True) if int(prefix_cache_rows or 0) > 0 else None
        # ONE chunk size for the whole server: the lock-step decoder hands out chunks of this many frames and every request's
        # StreamingVocoder is built for the same number (a voice entry's own "chunk_size" only applies to the lock scheduler)
        self.chunk_size = max(1, int(chunk_size))
        self.inbox: "queue.Queue" = queue.Queue()
        # text sessions whose first token has not arrived: they wait here, beside the scheduler, and block nobody
        self.parked: list = []
        self.wake = threading.Event()           # a request arrived / a parked session's feeder received something
        self.park_timeout_s = 30.0              # a session that never sends a token is answered with an error and dropped
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def submit(self, voice_cfg: dict, text: str) -> "queue.Queue":
        out: "queue.Queue" = queue.Queue()
        self.inbox.put((voice_cfg, text, out))
        self.wake.set()
        return out

    def submit_text(self, voice_cfg: dict, feeder) -> "queue.Queue":
        """A text session: ``feeder`` (a ``TextFeeder``) receives the text while the utterance decodes.  The request enters the
        scheduler when its first token exists.  Same reply queue as :meth:`submit`."""
        out: "queue.Queue" = queue.Queue()
        feeder.waker = self.wake                 # (the scheduler puts its own event here when it arms the lane)
        self.inbox.put((voice_cfg, feeder, out))
        self.wake.set()
        return out

    def _run(self):
        import torch
        from .batching import BatchRequest
        from .model import StreamingVocoder
        m = self.model
        while True:
            first = None
            if not self.parked:
                first = self.inbox.get()
                if first is None:
                    return
            elif not any(sum(it[1].pending()) for it in self.parked):
                # only sessions without a first token: sleep until one has it (or a request arrives), bounded for the park timeout
                self.wake.wait(0.05)
                self.wake.clear()
                now = time.monotonic()
                for it in [it for it in self.parked if now - it[3] > self.park_timeout_s]:
                    self.parked.remove(it)
                    it[2].put(TimeoutError("the session received no text"))
                    it[2].put(self.DONE)
                try:
                    first = self.inbox.get_nowait()
                    if first is None:
                        return
                except queue.Empty:
                    continue
            waiting: Dict[int, Any] = {}
            levels: list = []                   # (``--level``) reports of finished utterances on their way to the host: (bytes, event, hook)
            counter = [0]
            try:
                with torch.inference_mode():
                    def prepare(item):
                        """(voice cfg, text, reply queue) -> BatchRequest, or None when the request failed before decoding."""
                        cfg, text, out = item[:3]
                        if not isinstance(text, str):
                            return prepare_text(item)
                        try:
                            inner, talker, config, tie, tam, tth, tpe, rc = m._prepare_generation(
                                text=text, language=cfg.get("language", "Auto"), ref_audio=cfg.get("ref_audio"),
                                ref_text=cfg.get("ref_text", ""), voice_clone_prompt=cfg.get("voice_clone_prompt"),
                                non_streaming_mode=False)
                        except Exception as exc:
                            out.put(exc)
                            return None
                        i = counter[0]
                        counter[0] += 1
                        spec = cfg.get("audio_output")            # the request's AudioOutSpec (create_app puts it there), or None
                        waiting[i] = (out, m.streaming_vocoder(rc, self.chunk_size) if spec is None else
                                      m.streaming_vocoder(rc, self.chunk_size, output=spec))
                        level_start(waiting[i][1], cfg)
                        kw = m._gen_kwargs(int(cfg.get("max_new_tokens", 2048)), 2, 0.9, 50, 1.0, True, 1.05)
                        seed_kw = {} if cfg.get("seed") is None else dict(seed=cfg["seed"])     # (unseeded: the call stays what it was)
                        return BatchRequest(i, talker, tie, tam, tth, tpe, config, kw, **seed_kw)

                    def level_start(voc, cfg):
                        """``--level``: the request's leveller starts from what its voice's last stream learned, and reports back"""
                        if getattr(voc, "level_spec", None) is not None and cfg.get("initial_gain_db") is not None:
                            import dataclasses
                            voc.level_spec = dataclasses.replace(voc.level_spec, initial_gain_db=float(cfg["initial_gain_db"]))
                        voc.on_level = cfg.get("on_level")

                    def level_end(voc):
                        """the finished utterance's report is copied behind its last chunk; this thread, which feeds every lane, does
                        not wait for it: ``level_poll`` hands it to the request's hook once the copy has landed"""
                        if getattr(voc, "level_spec", None) is None or getattr(voc, "on_level", None) is None:
                            return
                        if voc.level is not None:                      # (an utterance that ended without a final chunk)
                            with (contextlib.nullcontext() if voc.side is None else torch.cuda.stream(voc.side)):
                                voc.level_release()
                        rep = voc.level_report_async()
                        if rep is not None:
                            levels.append((rep[0], rep[1], voc.on_level))

                    def level_poll(wait=False):
                        for item in list(levels):
                            host, ev, hook = item
                            if wait:
                                ev.synchronize()
                            if wait or ev.query():
                                levels.remove(item)
                                hook(StreamingVocoder.level_gain_of(host))

                    def prepare_text(item):
                        """A text session: parked until its first token exists, then a request built around that token."""
                        cfg, feeder, out = item[:3]
                        n, closed = feeder.pending()
                        if not n and not closed:
                            if len(item) == 3:
                                self.parked.append((cfg, feeder, out, time.monotonic()))
                            return None
                        if len(item) == 4:
                            self.parked.remove(item)
                        i = counter[0]

                        def build(input_ids):
                            inner, talker, config, tie, tam, tth, tpe, rc = m._prepare_generation(
                                text=None, language=cfg.get("language", "Auto"), ref_audio=cfg.get("ref_audio"), ref_text="",
                                xvec_only=True, voice_clone_prompt=cfg.get("voice_clone_prompt"), non_streaming_mode=False,
                                input_ids=input_ids)
                            if rc is not None:
                                raise ValueError("text sessions need an x-vector-only voice")
                            return inner, talker, config, tie, tam, tth, tpe
                        try:
                            m._bind_lane_prompt_weights(m._batch_decoder(self.lanes))
                            kw = m._gen_kwargs(int(cfg.get("max_new_tokens", 2048)), 2, 0.9, 50, 1.0, True, 1.05)
                            seed_kw = {} if cfg.get("seed") is None else dict(seed=cfg["seed"])
                            req = m.text_batch_request(i, feeder, build, kw, **seed_kw)
                        except Exception as exc:
                            out.put(exc)
                            out.put(self.DONE)
                            return None
                        counter[0] += 1
                        spec = cfg.get("audio_output")
                        waiting[i] = (out, m.streaming_vocoder(None, self.chunk_size) if spec is None else
                                      m.streaming_vocoder(None, self.chunk_size, output=spec))
                        level_start(waiting[i][1], cfg)
                        return req

                    def source():
                        """Polled by the scheduler at every frame boundary: requests that arrived while the batch was decoding,
                        parked sessions whose first token has come."""
                        for it in list(self.parked):
                            req = prepare_text(it)
                            if req is not None:
                                return req
                        while True:
                            try:
                                item = self.inbox.get_nowait()
                            except queue.Empty:
                                return None
                            if item is None:                   # shutdown marker: finish what is running, then stop
                                self.inbox.put(None)
                                return None
                            req = prepare(item)
                            if req is not None:
                                return req

                    head = prepare(first) if first is not None else None
                    chunk_frames = self.chunk_size
                    for rid, codes, info in m._batch_decoder(self.lanes).run([head] if head is not None else [], on_error="yield",
                                                                             source=source, chunk_frames=chunk_frames):
                        out, voc = waiting[rid]
                        level_poll()
                        final = bool(info.get("is_final")) or "error" in info
                        if "error" in info or (codes is None and final and info.get("steps", 0) == 0):
                            out.put(RuntimeError(info.get("error", "generation returned no tokens")))
                        elif (getattr(voc, "output", None) is not None or getattr(voc, "limit_spec", None) is not None
                              or getattr(voc, "level_spec", None) is not None):
                            # the request asked for a rate / encoding, or the server limits: the chunk comes back encoded (or float32); the
                            # last one brings the tail that the output stage / the limiter held back
                            if codes is not None and codes.shape[0] > 0:
                                audio, _sr = voc.push(codes, info.get("codes_ready_event"), final=final)
                            else:
                                audio, _sr = voc.flush() if final else (np.zeros(0, np.uint8), 0)
                            if len(audio):
                                out.put(audio)
                        elif codes is not None and codes.shape[0] > 0:
                            audio, _sr = voc.push(codes, info.get("codes_ready_event"))
                            out.put(np.asarray(audio, dtype=np.float32))
                        if final:
                            level_end(voc)
                            out.put(self.DONE)
                            waiting.pop(rid, None)
                    level_poll(wait=True)                              # the scheduler is idle: the last reports may be waited for
                # the scheduler is done: nobody may be left without an answer (a request it never reported would otherwise
                # block its HTTP handler and an executor thread forever)
                for out, _ in waiting.values():
                    out.put(RuntimeError("the batch scheduler finished without an answer for this request"))
                    out.put(self.DONE)
                waiting.clear()
            except Exception as exc:            # a failed batch answers everyone who is still waiting
                for out, _ in waiting.values():
                    out.put(exc)
                    out.put(self.DONE)
                waiting.clear()


LEVEL_FIELDS = ("target_lufs", "ceiling_db", "max_gain_db", "smooth_hops", "min_blocks")


def voice_key(cfg: dict, name: str):
    """What the learned gains of ``--level`` are kept under: for a voice with a reference clip the leading fields of the model's voice
    prompt cache key -- ``(str(ref_audio), ref_text)``, so two names for one clip share a gain -- else the speaker's or the voice's name."""
    if cfg.get("ref_audio") is not None:
        return (str(cfg["ref_audio"]), cfg.get("ref_text", ""))
    return ("speaker", str(cfg["speaker"])) if cfg.get("speaker") else ("voice", str(name))


DEFAULT_LOUDNESS_TEXT = "The quick brown fox jumps over the lazy dog, and then it rests beside the quiet river for a while."


def create_app(model, voices: Dict[str, dict], default_voice: Optional[str] = None, scheduler: str = "lock", lanes: int = 8,
               chunk_size: int = 12, worker=None, prefix_cache_rows: int = 0, long_form=None, exact_streaming: bool = False,
               loudness: Optional[float] = None, loudness_text: str = DEFAULT_LOUDNESS_TEXT, limiter_db: Optional[float] = None,
               level: Optional[float] = None):
    """``worker``: a ready ``BatchWorker`` (or a stand-in with ``submit`` / ``submit_text``) instead of the one ``scheduler="batch"``
    would start.  ``prefix_cache_rows`` > 0: the model's prefix KV cache (``FasterQwen3TTS.enable_prefix_cache``) with that many rows:
    the engine's cache under the ``lock`` scheduler; under ``batch`` the ``BatchWorker`` started here creates the scheduler's own
    (``batch=True``: packed admission through ``PrefixCache.prefill_pack``).  A ``worker`` handed in brings its own (its
    ``prefix_cache`` attribute, if any, is what ``/health`` reports).  ``long_form``: the ``LongFormSpec`` of the long-form path
    (None: the defaults); under the ``lock`` scheduler ``lanes`` is the number of segments it decodes side by side.
    ``exact_streaming``: the model's ``exact_streaming()`` context is entered for the life of the app -- both schedulers and the text
    sessions then stream the one-pass decode of every utterance instead of the reference's windowing (the vocoders come from
    ``model.streaming_vocoder``, on whichever thread).  ``loudness`` (a target in LUFS; None: off; ``lock`` scheduler only): every
    configured voice is synthesised once with ``loudness_text`` under ``seeded(0)`` and measured on the device
    (``model.measure_loudness``); the streamed replies of that voice then run inside ``model.fixed_gain`` with the gain that brings the
    calibration sentence to the target, and carry ``X-Gain-Db``.  A voice whose measurement is invalid gets 0 dB; ``/health`` lists
    the gains and says which voices are calibrated.  ``limiter_db`` (a ceiling in dBFS; None: off; server-wide, both schedulers and
    the text sessions): the model's ``limiter()`` context is entered for the life of the app, behind the calibration, so every reply
    leaves through a true-peak look-ahead limiter on the device.  ``loudness`` and ``limiter_db`` together are the safe way to serve a
    levelled stream: the gain comes from one calibration sentence, and the limiter catches the reply that comes out hotter.
    ``level`` (a target in LUFS; None: off; server-wide, BOTH schedulers and the text sessions): the model's ``leveller()`` context is
    entered for the life of the app, so every stream is levelled while it runs (``fq3hip/leveller.py``: causal, zero latency; it does
    not limit -- without ``limiter_db`` one warning says so).  Per-voice memory: when a stream ends with a valid measure, its last
    target gain is remembered under the voice's key (``voice_key``) and the voice's next request starts from it as
    ``initial_gain_db``; that reply carries ``X-Initial-Gain-Db`` and ``/health`` lists what was learned.  The memory is a dict in
    this process, nothing is written to disk.  Not together with ``loudness``.  The leveller's defaults are not tuned on real voices."""
    from fastapi import FastAPI, HTTPException
    from .long_form import LongFormSpec
    long_spec = long_form if long_form is not None else LongFormSpec()
    from fastapi.responses import Response, StreamingResponse

    app = FastAPI(title="faster-qwen3-tts (MI355X) OpenAI-compatible API")
    lock = threading.Lock()
    if exact_streaming:
        if not hasattr(model, "exact_streaming"):
            raise ValueError("exact_streaming: this model has no exact_streaming() context")
        app.state.exact_streaming = contextlib.ExitStack()
        app.state.exact_streaming.enter_context(model.exact_streaming())
    if worker is None and scheduler == "batch":
        worker = BatchWorker(model, lanes, chunk_size, prefix_cache_rows=int(prefix_cache_rows or 0))
    prefix_cache = getattr(worker, "prefix_cache", None)
    if worker is None and int(prefix_cache_rows or 0) > 0:
        prefix_cache = model.enable_prefix_cache(int(prefix_cache_rows))
    sessions: Dict[str, dict] = {}
    sessions_lock = threading.Lock()             # (the gains ``level`` learns live under it too)
    sample_rate = int(getattr(model, "sample_rate", 24000))
    gains: Dict[int, dict] = {}                  # id(voice entry) -> its calibration (``loudness``)
    if loudness is not None:
        if worker is not None or scheduler == "batch":
            raise ValueError("--loudness is served by the lock scheduler (--scheduler lock): the batch worker decodes the voices of many "
                             "requests in one launch set and has no per-request gain yet")
        from .loudness import LoudnessSpec
        loud_spec = LoudnessSpec(target_lufs=float(loudness))
        if not isinstance(loudness_text, str) or not loudness_text.strip():
            raise ValueError("--loudness-text must not be empty")
        for name, vcfg in voices.items():
            with model.seeded(0):
                wavs, _sr = model.generate_voice_clone(non_streaming_mode=False, language=vcfg.get("language", "Auto"), text=loudness_text,
                                                       ref_audio=vcfg.get("ref_audio"), ref_text=vcfg.get("ref_text", ""),
                                                       voice_clone_prompt=vcfg.get("voice_clone_prompt"),
                                                       **({"instruct": vcfg["instruct"]} if vcfg.get("instruct") else {}))
            st = model.measure_loudness(wavs[0], loud_spec)
            gains[id(vcfg)] = dict(voice=name, calibrated=bool(st.valid), gain_db=round(float(st.gain_db), 3) if st.valid else 0.0,
                                   lufs=round(float(st.lufs), 3) if st.valid else None)
            logger.info("loudness: voice %r reads %s LUFS, gain %+.2f dB%s", name, gains[id(vcfg)]["lufs"], gains[id(vcfg)]["gain_db"],
                        "" if st.valid else " (could not be calibrated)")

    learned: Dict[Any, float] = {}               # voice key -> the last valid target gain (dB) of that voice's streams (``level``)
    if level is not None:
        if loudness is not None:
            raise ValueError("--level and --loudness answer the same question: give one")
        if not hasattr(model, "leveller"):
            raise ValueError("level: this model has no leveller() context")
        app.state.leveller = contextlib.ExitStack()
        app.state.level_spec = app.state.leveller.enter_context(model.leveller(target_lufs=float(level)))      # (ValueError outside [-40, -5])
        if limiter_db is None:
            logger.warning("--level without --limiter-db: the leveller does not limit, a passage louder than everything before it can "
                           "pass the ceiling (add --limiter-db)")

    def level_cfg(cfg: dict, name: str):
        """``level``: the request's voice entry with the gain its voice learned and the hook that learns the next -> (cfg, headers)"""
        if level is None:
            return cfg, {}
        key = voice_key(cfg, name)
        with sessions_lock:
            start = learned.get(key)

        def on_level(gain_db):
            if gain_db is not None and math.isfinite(gain_db):
                with sessions_lock:
                    learned[key] = round(float(gain_db), 3)
        cfg = dict(cfg, on_level=on_level, **({} if start is None else dict(initial_gain_db=start)))
        return cfg, ({} if start is None else {"X-Initial-Gain-Db": f"{start:.3f}"})

    if limiter_db is not None:
        if not hasattr(model, "limiter"):
            raise ValueError("limiter_db: this model has no limiter() context")
        app.state.limiter = contextlib.ExitStack()
        app.state.limiter_spec = app.state.limiter.enter_context(model.limiter(ceiling_db=float(limiter_db)))      # (ValueError outside [-20, 0])

    def resolve_voice(name: str) -> dict:
        if name in voices:
            return voices[name]
        if default_voice and default_voice in voices:
            logger.warning("Voice %r not configured; falling back to default voice %r", name, default_voice)
            return voices[default_voice]
        raise HTTPException(status_code=400, detail=f"Voice {name!r} is not configured. Available voices: {list(voices.keys())}")

    # FLAC is made by the device stage alone: a model without ``audio_output`` cannot answer it
    flac_ok = hasattr(model, "audio_output")

    def request_spec(req, fmt: str = "wav"):
        """The request's ``AudioOutSpec``, or None when it names neither a rate nor an encoding nor a speed other than 1 (today's
        path).  400 for an unknown encoding, a rate the resampler refuses or a speed outside [0.25, 4.0].  ``response_format="flac"``
        is the ``flac`` encoding of the stage (with the request's rate and speed); it is the whole answer's format, so a request that
        also names an ``encoding`` gets 400, and so does ``encoding="flac"`` under another format."""
        from .audio_out import AudioOutSpec
        if fmt == "flac":
            if req.encoding is not None:
                raise HTTPException(status_code=400, detail="response_format='flac' is an encoding of its own (the s16 samples, compressed "
                                                            "losslessly): leave 'encoding' out")
            try:
                return AudioOutSpec(req.sample_rate, "flac", req.speed).validate(sample_rate)
            except ValueError as exc:
                raise HTTPException(status_code=400, detail=str(exc))
        if req.sample_rate is None and req.encoding is None and req.speed == 1.0:
            return None
        enc = (req.encoding or "s16").lower()
        if enc == "flac":
            raise HTTPException(status_code=400, detail="encoding 'flac' is asked for with response_format='flac'")
        try:
            return AudioOutSpec(req.sample_rate, "s16" if enc == "f32" else enc, req.speed).validate(sample_rate)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))

    def request_seed(req) -> Optional[int]:
        """The request's seed, or None; 400 outside [0, 2^64)."""
        if req.seed is None:
            return None
        from .generate import validate_seed
        try:
            return validate_seed(req.seed)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))

    def seed_headers(seed: Optional[int]) -> Optional[dict]:
        return None if seed is None else {"X-Seed": str(seed)}

    def clone_kwargs(cfg: dict, text: str) -> dict:
        return dict(text=text, language=cfg.get("language", "Auto"), ref_audio=cfg.get("ref_audio"), ref_text=cfg.get("ref_text", ""),
                    voice_clone_prompt=cfg.get("voice_clone_prompt"))

    def long_segments(req) -> int:
        """How many segments the request's long-form path has, or 0 when it takes today's path.  400 when ``long_form: true`` cannot
        be served."""
        design = getattr(getattr(getattr(model, "model", None), "model", None), "tts_model_type", None) == "voice_design"
        able = hasattr(model, "generate_long_voice_clone_streaming") and not design
        if req.long_form:
            if worker is not None:
                raise HTTPException(status_code=400, detail="long_form is served by the lock scheduler (--scheduler lock); the batch "
                                                            "scheduler does not take segments yet")
            if not able:
                raise HTTPException(status_code=400, detail="long_form needs a clone or custom voice (a voice-design model would "
                                                            "change its voice between segments)")
        elif req.long_form is False or worker is not None or not able or len(req.input) <= long_spec.max_chars:
            return 0
        return len(long_spec.split(req.input))

    async def stream_chunks(cfg: dict, text: str, spec=None, long: bool = False) -> AsyncGenerator[bytes, None]:
        q: "queue.Queue" = queue.Queue()
        done = object()

        # a voice entry's optional "instruct" (an instruct turn ahead of the prompt: what the prefix cache reuses); lock scheduler only
        instruct_kw = {"instruct": cfg["instruct"]} if cfg.get("instruct") else {}

        def producer():
            try:
                with lock, (contextlib.nullcontext() if spec is None else model.audio_output(spec.sample_rate, spec.encoding, spec.speed)), \
                        (contextlib.nullcontext() if cfg.get("seed") is None else model.seeded(cfg["seed"])), \
                        (contextlib.nullcontext() if cfg.get("gain_db") is None else model.fixed_gain(cfg["gain_db"])), \
                        (contextlib.nullcontext() if cfg.get("initial_gain_db") is None else
                         model.leveller(**dict({k: getattr(app.state.level_spec, k) for k in LEVEL_FIELDS}, initial_gain_db=cfg["initial_gain_db"]))):
                    gen = (model.generate_long_voice_clone_streaming(chunk_size=cfg.get("chunk_size", 12), non_streaming_mode=False,
                                                                     lanes=lanes, long_form=long_spec, **clone_kwargs(cfg, text), **instruct_kw)
                           if long else
                           model.generate_voice_clone_streaming(chunk_size=cfg.get("chunk_size", 12), non_streaming_mode=False,
                                                                **clone_kwargs(cfg, text), **instruct_kw))
                    for chunk, _sr, _t in gen:
                        q.put(chunk)
                    if cfg.get("on_level") is not None:
                        cfg["on_level"](getattr(model, "last_level_gain_db", None))
            except Exception as exc:
                q.put(exc)
            finally:
                q.put(done)

        threading.Thread(target=producer, daemon=True).start()
        loop = asyncio.get_event_loop()
        while True:
            item = await loop.run_in_executor(None, q.get)
            if item is done:
                break
            if isinstance(item, Exception):
                raise item
            yield to_pcm16(item) if spec is None else np.ascontiguousarray(item).tobytes()

    async def box_response(box, fmt: str, on_end=None, spec=None, seed=None, headers=None):
        """The streaming body of a batch-scheduler reply queue (``BatchWorker.submit`` / ``submit_text``)."""
        loop = asyncio.get_event_loop()

        async def batch_stream():
            first = True
            while True:
                item = await loop.run_in_executor(None, box.get)
                if item is BatchWorker.DONE:
                    break
                if isinstance(item, Exception):
                    if first:
                        raise HTTPException(status_code=500, detail=repr(item))
                    logger.error("generation failed mid-stream: %r", item)
                    break
                if first and fmt == "wav":
                    # unknown data length: streaming
                    yield wav_header(sample_rate) if spec is None else wav_header_for(spec.out_rate(sample_rate), spec.encoding)
                first = False
                yield to_pcm16(item) if spec is None else np.ascontiguousarray(item).tobytes()

        # pull the first event before answering, so that a request that fails outright is a 500, not an empty 200
        gen = batch_stream()
        try:
            head = await gen.__anext__()
        except StopAsyncIteration:
            head = None
        except BaseException:
            if on_end is not None:
                on_end()
            raise

        async def replay():
            try:
                if head is not None:
                    yield head
                async for raw in gen:
                    yield raw
            finally:
                if on_end is not None:
                    on_end()

        return StreamingResponse(replay(), media_type=CONTENT_TYPES[fmt], headers=dict(seed_headers(seed) or {}, **(headers or {})) or None)

    # ---- text sessions: the text arrives in pieces while the audio is already streaming (batch scheduler) -----------------------
    def drop_session(sid: str):
        with sessions_lock:
            s = sessions.pop(sid, None)
        if s is not None:
            s["feeder"].close()               # a consumer that went away: the utterance ends at the text it has

    def live_session(sid: str) -> dict:
        with sessions_lock:
            s = sessions.get(sid)
        if s is None:
            raise HTTPException(status_code=404, detail=f"no such session: {sid!r} (unknown, finished or timed out)")
        return s

    @app.post("/v1/audio/speech/sessions")
    async def open_session(req: SessionRequest):
        if model is None:
            raise HTTPException(status_code=503, detail="Model not loaded")
        if worker is None or not hasattr(worker, "submit_text"):
            raise HTTPException(status_code=400, detail="text sessions need --scheduler batch")
        cfg = resolve_voice(req.voice)
        fmt = req.response_format.lower()
        if fmt not in ("wav", "pcm", "flac") or (fmt == "flac" and not flac_ok):
            raise HTTPException(status_code=400, detail=f"response_format {fmt!r} not supported for sessions. Use: wav, pcm")
        spec = request_spec(req, fmt)
        if spec is not None:
            cfg = dict(cfg, audio_output=spec)
        seed = request_seed(req)
        if seed is not None:
            cfg = dict(cfg, seed=seed)
        cfg, level_headers = level_cfg(cfg, req.voice)
        try:
            from .model import FasterQwen3TTS
            FasterQwen3TTS._refuse_icl_text_stream(True, cfg.get("voice_clone_prompt"))
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
        from .text_stream import TextFeeder
        feeder = TextFeeder(model._text_tokenize())
        sid = uuid.uuid4().hex
        now = time.monotonic()
        with sessions_lock:
            # sessions nobody ever read: their text ended (the client's `final`, or the scheduler's idle rule) long ago
            for old in [k for k, s in sessions.items() if not s["reading"] and s["feeder"].closed and now - s["t_closed"] > 60.0]:
                sessions.pop(old, None)
            sessions[sid] = dict(feeder=feeder, box=worker.submit_text(cfg, feeder), fmt=fmt, reading=False, t_closed=now, spec=spec,
                                 seed=seed, headers=level_headers)
        return {"id": sid} if seed is None else {"id": sid, "seed": seed}

    @app.post("/v1/audio/speech/sessions/{sid}/text")
    async def session_text(sid: str, req: SessionText):
        s = live_session(sid)
        try:
            if req.text:
                s["feeder"].feed(req.text)
            if req.final:
                s["feeder"].close()
                s["t_closed"] = time.monotonic()
        except ValueError as exc:                          # text after `final` (or after the idle rule closed the stream)
            raise HTTPException(status_code=409, detail=str(exc))
        return {"id": sid, "final": s["feeder"].closed}

    @app.get("/v1/audio/speech/sessions/{sid}/audio")
    async def session_audio(sid: str):
        s = live_session(sid)
        with sessions_lock:
            if s["reading"]:
                raise HTTPException(status_code=409, detail="this session's audio is being read already")
            s["reading"] = True
        return await box_response(s["box"], s["fmt"], on_end=lambda: drop_session(sid), spec=s["spec"], seed=s.get("seed"),
                                  headers=s.get("headers"))

    @app.get("/health")
    async def health():
        out = {"status": "ok", "model_loaded": model is not None, "scheduler": scheduler, "lanes": lanes if worker else 1}
        if prefix_cache is not None:
            out["prefix_cache"] = prefix_cache.stats()
        if exact_streaming:
            out["exact_streaming"] = True
        if loudness is not None:
            out["loudness"] = {"target_lufs": float(loudness),
                               "voices": {g["voice"]: {k: g[k] for k in ("gain_db", "lufs", "calibrated")} for g in gains.values()}}
        if limiter_db is not None:
            spec = app.state.limiter_spec                   # the LimiterSpec in force, as the model's context yielded it
            out["limiter"] = {k: float(getattr(spec, k)) for k in ("ceiling_db", "lookahead_ms", "hold_ms")}
        if level is not None:
            spec = app.state.level_spec                     # the LevelSpec in force, as the model's context yielded it
            with sessions_lock:
                known = {str(k): v for k, v in learned.items()}
            out["level"] = dict({k: getattr(spec, k) for k in LEVEL_FIELDS}, learned_gains_db=known)
        return out

    @app.post("/v1/audio/speech")
    async def create_speech(req: SpeechRequest):
        if model is None:
            raise HTTPException(status_code=503, detail="Model not loaded")
        if not req.input.strip():
            raise HTTPException(status_code=400, detail="'input' text is empty")
        cfg = resolve_voice(req.voice)
        fmt = req.response_format.lower()
        if fmt not in CONTENT_TYPES or (fmt == "flac" and not flac_ok):
            raise HTTPException(status_code=400, detail=f"response_format {fmt!r} not supported. Use: wav, pcm, mp3")
        if fmt == "mp3":
            raise HTTPException(status_code=400, detail="response_format='mp3' needs pydub + ffmpeg, which this image does not ship; use wav or pcm")
        spec = request_spec(req, fmt)
        seed = request_seed(req)
        gain = gains.get(id(cfg))
        if gain is not None:
            cfg = dict(cfg, gain_db=gain["gain_db"])
        if seed is not None:
            cfg = dict(cfg, seed=seed)
        cfg, level_headers = level_cfg(cfg, req.voice)
        n_segments = long_segments(req)
        if worker is not None:
            return await box_response(worker.submit(cfg if spec is None else dict(cfg, audio_output=spec), req.input), fmt, spec=spec,
                                      seed=seed, headers=level_headers)

        async def audio_stream():
            if fmt == "wav":
                # unknown data length: streaming
                yield wav_header(sample_rate) if spec is None else wav_header_for(spec.out_rate(sample_rate), spec.encoding)
            async for raw in stream_chunks(cfg, req.input, spec, long=n_segments > 0):
                yield raw

        headers = dict(seed_headers(seed) or {}, **level_headers)
        if gain is not None:
            headers["X-Gain-Db"] = f"{gain['gain_db']:.3f}"
        if n_segments > 0:
            headers["X-Segments"] = str(n_segments)
        return StreamingResponse(audio_stream(), media_type=CONTENT_TYPES[fmt], headers=headers or None)

    return app


def build_parser():
    p = argparse.ArgumentParser(description="OpenAI-compatible TTS server over the MI355X HIP path")
    p.add_argument("--model", default=os.environ.get("QWEN_TTS_MODEL", "Qwen/Qwen3-TTS-12Hz-1.7B-Base"))
    p.add_argument("--voices", default=os.environ.get("QWEN_TTS_VOICES"), metavar="FILE")
    p.add_argument("--ref-audio", default=os.environ.get("QWEN_TTS_REF_AUDIO"), metavar="FILE")
    p.add_argument("--ref-text", default=os.environ.get("QWEN_TTS_REF_TEXT", ""))
    p.add_argument("--language", default=os.environ.get("QWEN_TTS_LANGUAGE", "Auto"))
    p.add_argument("--host", default="0.0.0.0")
    p.add_argument("--port", type=int, default=8000)
    p.add_argument("--device", default="cuda")
    p.add_argument("--scheduler", default="batch", choices=["lock", "batch"])
    p.add_argument("--lanes", type=int, default=8)
    p.add_argument("--chunk-size", type=int, default=12, help="frames per streamed chunk (batch scheduler: server-wide)")
    p.add_argument("--voice-cache", help="directory of precomputed voice prompts serving ref_audio entries")
    p.add_argument("--synthetic", choices=["0.6b", "1.7b"])
    p.add_argument("--prefix-cache-rows", type=int, default=0, metavar="N",
                   help="keep the talker K/V rows of instruct turns on the device, up to N rows (default 0: off); under --scheduler batch "
                        "the packed admission reuses them, under --scheduler lock each request does")
    p.add_argument("--exact-streaming", action="store_true",
                   help="stream the one-pass decode of every utterance (codec stream states) instead of the reference's 25-frame windowing: "
                        "the audio no longer depends on the chunk size (default: off)")
    p.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                   help="calibrate every voice at start-up (one seeded synthesis of --loudness-text, measured on the device by BS.1770) and "
                        "stream its replies with the fixed gain that brings that sentence to LUFS; --scheduler lock only (default: off)")
    p.add_argument("--loudness-text", default=DEFAULT_LOUDNESS_TEXT, metavar="TEXT", help="the calibration sentence of --loudness")
    p.add_argument("--limiter-db", type=float, default=None, metavar="DB",
                   help="server-wide true-peak look-ahead limiter on the device: no sample of any reply leaves above DB dBFS (-20 to 0); both "
                        "schedulers and the text sessions.  With --loudness the two together are the safe way to serve a levelled stream: a "
                        "reply hotter than the calibration sentence is limited instead of clipped (default: off)")
    p.add_argument("--level", type=float, default=None, metavar="LUFS",
                   help="server-wide streaming loudness leveller on the device: every stream is brought to LUFS while it runs (causal BS.1770 "
                        "gain, zero latency); both schedulers and the text sessions.  A voice's next request starts from the gain its last "
                        "stream ended with (X-Initial-Gain-Db; kept in memory only).  It does not limit: add --limiter-db.  Its defaults are "
                        "not tuned on real voices (default: off)")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.level is not None and args.loudness is not None:
        parser.error("--level and --loudness answer the same question: give one")
    if args.level is not None and not -40.0 <= args.level <= -5.0:
        parser.error("--level is a target in LUFS, -40 to -5")
    if args.loudness is not None and args.scheduler == "batch":
        parser.error("--loudness is served by the lock scheduler: add --scheduler lock (the batch worker has no per-request gain yet)")
    if args.limiter_db is not None and not -20.0 <= args.limiter_db <= 0.0:
        parser.error("--limiter-db is a ceiling in dBFS, -20 to 0")
    if args.voices:
        with open(args.voices) as f:
            voices = json.load(f)
        default_voice = next(iter(voices))
    elif args.ref_audio:
        voices = {"default": {"ref_audio": args.ref_audio, "ref_text": args.ref_text, "language": args.language}}
        default_voice = "default"
    else:
        print("ERROR: provide --ref-audio <file> or --voices <config.json>", file=sys.stderr)
        sys.exit(1)
    from types import SimpleNamespace
    from .cli import load_model
    model = load_model(SimpleNamespace(model=args.model, device=args.device, dtype="bf16", backend="torch", synthetic=args.synthetic,
                                       voice_cache=args.voice_cache))
    import uvicorn
    logging.basicConfig(level=logging.INFO)
    uvicorn.run(create_app(model, voices, default_voice, args.scheduler, args.lanes, args.chunk_size,
                           prefix_cache_rows=args.prefix_cache_rows, exact_streaming=args.exact_streaming, loudness=args.loudness,
                           loudness_text=args.loudness_text, limiter_db=args.limiter_db, level=args.level), host=args.host, port=args.port)


if __name__ == "__main__":
    main()
