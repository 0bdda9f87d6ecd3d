"""Incremental text: decode while the text is still arriving.

In the step-by-step prompt layout (``non_streaming_mode=False``, ``prompt.py``) the prompt holds only the FIRST text token; every
later token is one row of the trailing-text table and frame ``g`` adds row ``g`` to the talker's input.  A row is
``text_projection(text_embedding(id))``: a function of the token id alone.  So frame ``g`` needs text token ``g + 1`` and nothing
later, and a session can be armed on the first token and fed the rest while it decodes:

* :class:`TextFeeder` -- the thread-safe way in: ``feed(str)`` / ``feed_ids(list)`` / ``close()`` from any thread;
* :class:`TextSession` -- the host's gate: appends what the feeder holds to the loop's open table
  (``Fq3Engine.decode_text_append``) and never queues frame ``g`` before row ``g`` has been appended or the table is closed;
* :func:`fast_generate_text_streaming` -- the generator contract of ``streaming.fast_generate_streaming`` on top of the two.

The identity contract: codes, chunk boundaries and timing keys are those of ``fast_generate_streaming`` on the whole text with
``non_streaming_mode=False``, bit for bit, whatever the cuts and the timing of the pieces.

Why the host gates although the device holds: ``run_frames`` refills the noise rings by the count of frames LAUNCHED while the
device reads ring row ``frame % noise_frames`` by the count of frames EMITTED; the two agree only if no launched frame is a no-op.
The device's hold rule (``frame_begin_body``: a frame whose row is missing leaves the loop untouched) is what makes a late append
harmless instead of a silent switch to the pad row, and what the lock-step lanes need, where the host cannot gate one lane.
"""
from __future__ import annotations

import threading
import time
from collections import deque
from typing import Callable, Generator, Iterable, List, Optional, Tuple

import torch

from .generate import NOISE_RING, _prefill_and_arm, _refill, validate_seed


class TextFeeder:
    """Thread-safe queue of text for one utterance.

    ``feed(str)`` tokenises whole words only: the tail after the last whitespace character is held back until more text or
    ``close()`` arrives, so a word is never tokenised in two halves (the whitespace itself stays with the held tail: byte-level BPE
    vocabularies attach a space to the word that follows it).  With the repository's ``ByteTokenizer`` (one id per UTF-8 byte) any
    cut therefore gives the ids of the whole text.  Whether a real Qwen tokenizer gives the same ids for whitespace-cut pieces as for
    the whole text has NOT been checked (no tokenizer files were available): merges across a whitespace boundary would break it.
    ``feed_ids`` bypasses the tokeniser for callers that hold token ids already.
    """

    def __init__(self, tokenize: Optional[Callable[[str], List[int]]] = None):
        self._tokenize = tokenize
        self._cv = threading.Condition()
        self._ids: deque = deque()
        self._tail = ""
        self._closed = False
        self.t_first: Optional[float] = None        # host time of the first piece received (first_text_ms)
        self.released: List[str] = []               # the text pieces handed to the tokeniser, in order
        self.t_oldest: Optional[float] = None       # time.monotonic() at which the oldest id still queued became available
        self.waker: Optional[threading.Event] = None        # set on every feed / close: the batch scheduler sleeps on it when no lane can advance

    def _release(self, text: str):
        if not text:
            return
        if self._tokenize is None:
            raise ValueError("this TextFeeder has no tokeniser: use feed_ids()")
        self.released.append(text)
        self._ids.extend(int(i) for i in self._tokenize(text))

    def _notify(self):
        if self._ids and self.t_oldest is None:
            self.t_oldest = time.monotonic()
        self._cv.notify_all()
        if self.waker is not None:
            self.waker.set()

    def feed(self, text: str) -> None:
        with self._cv:
            if self._closed:
                raise ValueError("feed() after close()")
            if self.t_first is None:
                self.t_first = time.time()
            buf = self._tail + text
            cut = max((i for i, ch in enumerate(buf) if ch.isspace()), default=-1)
            if cut > 0:
                self._release(buf[:cut])
                buf = buf[cut:]
            self._tail = buf
            self._notify()

    def feed_ids(self, ids: Iterable[int]) -> None:
        with self._cv:
            if self._closed:
                raise ValueError("feed_ids() after close()")
            if self.t_first is None:
                self.t_first = time.time()
            self._ids.extend(int(i) for i in ids)
            self._notify()

    def close(self) -> None:
        """No more text: releases the held tail.  Idempotent."""
        with self._cv:
            if not self._closed:
                tail, self._tail = self._tail, ""
                self._release(tail)
                self._closed = True
            self._notify()

    @property
    def closed(self) -> bool:
        with self._cv:
            return self._closed

    def pending(self) -> Tuple[int, bool]:
        """``(ids queued, closed)`` without taking anything: a batch front end admits a request once its first token exists."""
        with self._cv:
            return len(self._ids), self._closed

    def take(self, block: bool = False, limit: Optional[int] = None, timeout: Optional[float] = None) -> Tuple[List[int], bool]:
        """``(ids, closed)``: the ids queued so far (at most ``limit``) and whether the feeder is closed AND drained.  ``block``:
        wait until there is an id or the feeder is closed."""
        with self._cv:
            if block:
                self._cv.wait_for(lambda: self._ids or self._closed, timeout)
            n = len(self._ids) if limit is None else min(int(limit), len(self._ids))
            ids = [self._ids.popleft() for _ in range(n)]
            if not self._ids:
                self.t_oldest = None
            elif ids:
                self.t_oldest = time.monotonic()
            return ids, self._closed and not self._ids


def pump_text(feeder: TextFeeder, text_iter: Iterable[str]) -> threading.Thread:
    """Feed ``text_iter`` into ``feeder`` from a daemon thread; the feeder is closed when the iterable ends -- or raises: an
    abandoned source ends the utterance the way whole text does."""
    def run():
        try:
            for piece in text_iter:
                feeder.feed(piece)
        finally:
            feeder.close()
    th = threading.Thread(target=run, name="fq3-text-pump", daemon=True)
    th.start()
    return th


class TextSession:
    """The host side of one open text table: appends rows as the feeder yields ids, launches frames behind them.

    ``rows`` counts the rows appended (the closing ``tts_eos`` row included), ``issued`` the frames launched.  The invariant every
    launch keeps: frame ``g`` is queued only when ``g < rows`` or the table is closed.  Ids beyond the table's capacity are dropped and
    the table is closed: ``capacity = max_frames + 1`` rows are more than the loop can read (frame ``g`` reads row ``g < max_frames``).
    """

    def __init__(self, eng, feeder: TextFeeder, eos_id: int, capacity: int, talker_noise=None, pred_noise=None, refill=_refill, seed=None):
        self.eng, self.feeder, self.eos_id, self.capacity = eng, feeder, int(eos_id), int(capacity)
        self.seed = seed                         # a seeded session refills with the emitted-frame count (= issued: the gate below)
        self.tn, self.pn, self._refill = talker_noise, pred_noise, refill
        self.rows, self.closed, self.issued, self.refills = 0, False, 0, 0

    def _append(self, ids: List[int], final: bool):
        room = self.capacity - self.rows
        if final:
            ids = list(ids) + [self.eos_id]
        if len(ids) >= room:                     # the loop cannot reach further rows: close here
            ids, final = ids[:room], True
        if ids or final:
            self.eng.decode_text_append(ids, final)
        self.rows += len(ids)
        self.closed = self.closed or final

    def drain(self, block: bool) -> None:
        """Append what the feeder holds; ``block``: wait on the HOST for an id or the close (no frame is queued meanwhile)."""
        if self.closed:
            return
        ids, fin = self.feeder.take(block=block)
        if ids or fin:
            self._append(ids, fin)

    def _launch(self, count: int):
        while count > 0:
            if self.issued % NOISE_RING == 0:
                if self.seed is None:
                    self._refill(self.eng, self.tn, self.pn)
                else:
                    self._refill(self.eng, self.tn, self.pn, self.seed, self.issued)
                self.refills += 1
            k = min(count, NOISE_RING - self.issued % NOISE_RING)
            self.eng.decode_frames(k)
            self.issued += k
            count -= k

    def pump(self, target: int, block: bool) -> int:
        """Launch frames until ``issued == target``, each behind its text row.  ``block=False`` launches what the rows at hand
        allow and returns."""
        while self.issued < target:
            self.drain(block=False)
            avail = target if self.closed else min(self.rows, target)
            if avail > self.issued:
                self._launch(avail - self.issued)
                continue
            if not block:
                break
            self.drain(block=True)
        return self.issued


@torch.inference_mode()
def fast_generate_text_streaming(talker, talker_input_embeds, attention_mask, tts_pad_embed, config, predictor_graph, talker_graph,
                                 feeder: TextFeeder, tts_eos_id: int, max_new_tokens: int = 2048, min_new_tokens: int = 2,
                                 temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0, do_sample: bool = True,
                                 repetition_penalty: float = 1.05, chunk_size: int = 12,
                                 use_graph: bool = True, seed=None) -> Generator[Tuple[torch.Tensor, dict], None, None]:
    """``fast_generate_streaming`` for a text that is still arriving.  ``talker_input_embeds`` is the step-by-step prompt (it ends
    with the first text token against ``codec_bos``); ``feeder`` yields the ids of every LATER text token; the session appends
    ``tts_eos_id`` itself when the feeder is closed, as ``prompt.py`` ends the trailing table.  Yields ``(codes, timing)`` with the
    same keys, the same ``is_final`` rule and the same look-ahead of one chunk; the first chunk's timing also has ``first_text_ms``
    (first piece received -> first chunk's codes) when the feeder noted a first piece."""
    seed = validate_seed(seed)
    t_start = time.time()
    H = talker_input_embeds.shape[-1]
    empty = talker_input_embeds.new_zeros(1, 0, H)
    eng, tn, pn, max_frames = _prefill_and_arm(
        talker, talker_input_embeds, attention_mask, empty, tts_pad_embed, config, predictor_graph, talker_graph, max_new_tokens,
        min_new_tokens, temperature, top_k, top_p, do_sample, repetition_penalty, use_graph=use_graph, seed=seed)
    eng.decode_text_open(max_frames + 1)
    sess = TextSession(eng, feeder, tts_eos_id, max_frames + 1, tn, pn, seed=seed)
    torch.cuda.current_stream(eng.device).synchronize()
    t_prefill = time.time() - t_start
    emitted, chunk_count = 0, 0
    chunk_start = time.time()
    target = min(chunk_size, max_frames)
    while True:
        sess.pump(target, block=True)                 # the rest of this chunk's frames, each behind its row
        n, state = eng.decode_poll_state()            # host sync: chunk k is complete
        if state == 2:
            # cannot happen while the gate holds; a held frame that was launched has put the noise rings out of step
            raise RuntimeError("a frame was queued before its text row (noise rings out of step)")
        done = bool(state)
        new = n - emitted
        if new <= 0:
            break
        chunk = eng.decode_codes(emitted, new)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(eng.device))
        emitted = n
        is_final = new < chunk_size
        more = (not done) and (not is_final) and sess.issued < max_frames
        if more:
            # look-ahead: as much of chunk k+1 as the rows at hand allow decodes while the consumer vocodes chunk k
            target = sess.issued + min(chunk_size, max_frames - sess.issued)
            sess.pump(target, block=False)
        timing = {
            "chunk_index": chunk_count,
            "chunk_steps": new,
            "prefill_ms": t_prefill * 1000 if chunk_count == 0 else 0,
            "decode_ms": (time.time() - chunk_start) * 1000,
            "total_steps_so_far": emitted,
            "is_final": is_final,
            "codes_ready_event": ready,
        }
        if chunk_count == 0 and feeder.t_first is not None:
            timing["first_text_ms"] = (time.time() - feeder.t_first) * 1000
        yield chunk, timing
        chunk_count += 1
        chunk_start = time.time()
        if not more:
            break
