"""Continuous batching over ``Fq3Batch`` (``fq3_batch_*``): several utterances decode in lock-step over one weight
stream; a finished lane is re-armed with the next request at a frame boundary.  With ``staging`` contexts the next
requests are prefilled on a side stream WHILE the batch decodes, and a freed lane takes the staged prompt's KV over by a
block-table hand-over (``fq3_kv_adopt`` between contexts of one ``Fq3KvPool``: no KV row is copied), so admission costs the
running lanes a few tens of microseconds instead of a prefill.

KV memory follows the work, not the lane count: the contexts draw 64-key blocks from one pool; an idle lane or spare context
holds none, a staged request the blocks of its prompt + ``max_new_tokens`` (taken BEFORE its prefill is queued: a short pool
postpones the request instead of failing half-way), and a finished lane returns its blocks at once.

No reference equivalent -- the reference decodes one utterance at a time (``talker_graph.py:46`` /
``predictor_graph.py:70`` fix batch = 1 and ``examples/openai_server.py:71`` serialises requests with a lock); the
per-utterance semantics are the reference's (``generate.py:16-215``): same prefill, same first-token sampling, same
suppress / min_new / repetition-penalty policy, and -- because the batch kernels keep the single-stream arithmetic --
the same ids as ``fast_generate`` for the same noise.

INCREMENTAL TEXT (``BatchRequest.text_feeder``): a request may be armed on its first text token and fed the rest while it decodes.
Its lane holds an open text table on the device; before every batch of frames the scheduler drains all feeders and sends ONE
``Fq3Batch.text_append`` for all lanes.  Appends and frames share one stream, so what the device's hold rule does is known on the
host: after ``step`` frames such a lane has EMITTED ``min(emitted + step, rows published if open, max_frames)``.  For a text lane
``_Lane.issued`` is that count (for a whole-text lane launched = emitted, as ever), and the noise rings, the step bound, the frame
limit and the look-ahead clamp all follow it; every poll is checked against it.
"""
from __future__ import annotations

import threading
import time
from collections import deque
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Tuple

import torch

from ._lib import FQ3_ENOMEM
from .generate import (NOISE_RING, _arm_decode, _prefill_and_arm, _prefill_first_token, _prefill_first_tokens_launch,
                       _prefill_first_tokens_packed, _refill, validate_seed)
from .predictor_graph import PredictorGraph
from .talker_graph import TalkerGraph


MAX_LANES = 128         # kMaxLanes of csrc/batch_kernels.cuh (fq3_batch_create refuses more)
_clock = time.perf_counter


@dataclass
class BatchRequest:
    """One utterance: the tensors ``fast_generate`` takes plus its sampling arguments."""
    rid: Any
    talker: Any
    talker_input_embeds: torch.Tensor
    attention_mask: torch.Tensor
    trailing_text_hiddens: torch.Tensor
    tts_pad_embed: torch.Tensor
    config: Any
    gen_kwargs: Dict[str, Any] = field(default_factory=dict)
    # incremental text: ``talker_input_embeds`` is the step-by-step prompt built from the FIRST text token, ``trailing_text_hiddens`` an
    # empty [1, 0, H] table, ``text_feeder`` (a ``text_stream.TextFeeder``) yields the ids of every later token and ``tts_eos_id`` is
    # the row the scheduler appends when the feeder is closed
    text_feeder: Any = None
    tts_eos_id: Optional[int] = None
    # sampling seed (None: torch's global generator, as ever): the lane's noise is a pure function of (seed, emitted frame), so the codes
    # do not depend on the lane, its neighbours or the order of admission
    seed: Optional[int] = None


@dataclass
class _TextLane:
    """Host side of one lane's open text table (what ``text_stream.TextSession`` is to a single stream)."""
    feeder: Any
    eos_id: int
    capacity: int
    rows: int = 0                # rows appended (published in stream order before the next frames)
    closed: bool = False
    refilled_at: int = -1        # the emitted-frame count the noise rings were last refilled for
    t_last: float = 0.0          # host time the feeder last delivered something (idle rule)


@dataclass
class _Lane:
    index: int
    engine: Any
    talker_graph: Any
    predictor_graph: Any
    req: Optional[BatchRequest] = None
    tn: Optional[torch.Tensor] = None
    pn: Optional[torch.Tensor] = None
    issued: int = 0
    emitted: int = 0             # frames already handed out as partial chunks (chunk_frames mode)
    max_frames: int = 0
    t_arm: float = 0.0
    prefill_ms: float = 0.0
    first_batch: int = 0         # index of the first batch of frames queued after this tenant was armed (polls of earlier batches show its predecessor)
    copied: Any = None           # event: the last side-stream read of this lane's code buffer (a new tenant is armed after it)
    text: Optional[_TextLane] = None     # incremental text: `issued` then counts EMITTED frames (the host's model of the hold rule)
    seed: Optional[int] = None   # the tenant's sampling seed (BatchRequest.seed); a new tenant starts again at frame 0


@dataclass
class _Stage:
    """A spare context a pending request is prefilled into (side stream) before a lane is free."""
    engine: Any
    req: Optional[BatchRequest] = None
    kw: Optional[Dict[str, Any]] = None
    token: int = 0
    hidden: Optional[torch.Tensor] = None
    n_rows: int = 0
    n_pad: int = 0               # left padding of the staged prompt (counted by the prefill)
    ready: Any = None            # event: prefill + first token done (side stream)
    released: Any = None         # event: the lane has copied the KV rows out (main stream)
    t0: float = 0.0
    prefill_ms: float = 0.0


class BatchDecoder:
    """Drives up to ``len(engines)`` lanes.  ``engines[1:]`` must share ``engines[0]``'s weights
    (``Fq3Engine(..., share=engines[0])``)."""

    def __init__(self, engines: List[Any], predictor_policy: Optional[Dict[str, Any]] = None, poll_every: int = 8,
                 use_graph: bool = True, batch_factory=None, staging: Optional[List[Any]] = None, packed_prefill: bool = True,
                 prefix_cache=None):
        if batch_factory is None:
            from .engine import Fq3Batch as batch_factory
        policy = predictor_policy or dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9)
        self.lanes = [_Lane(i, e, TalkerGraph(e), PredictorGraph(e, **policy)) for i, e in enumerate(engines)]
        self.batch = batch_factory(engines)
        self.poll_every = max(1, int(poll_every))
        self.more_in_poll = 0
        self.use_graph = use_graph
        self._captured = False
        # spare contexts (same weights, not part of the lock-step batch) for prefilling ahead of admission
        self.stages = [_Stage(e) for e in (staging or [])]
        self._side = None
        self._unsynced: list = []   # groups staged with defer=True whose first tokens are still on the device (_stage_sync)
        self.kv_pool = None         # the pool the contexts draw their KV blocks from (set by whoever built them; read by bench.py)
        # lane groups the batch advances concurrently (set together with fq3_batch_set_option("groups"); None: the library's choice)
        self.n_groups: Optional[int] = None
        self._group_side: list = []     # the further groups' streams (_group_streams)
        # other streams the host keeps busy while the batch decodes (the vocoder's): the prefill stream and the lane groups' stream are
        # probed for a hardware queue shared with none of them (fq3hip/streams.py)
        self.beside: list = []
        # LOOK-AHEAD (round 4): the next batch of frames is queued BEFORE the host waits for the previous batch's poll, so the GPU works
        # while the host digests a poll (finishes, chunk events, admissions, staged prefills: ~2 ms per poll of 64 lanes, ~5 ms with a
        # staging group; measured on MI355X: 13 % of a 64-lane end-to-end run was an idle decode queue, profiles/r04_e2e_timeline_*.txt).
        # The poll is one launch + one copy in stream order (fq3_batch_poll_async), read when its event has fired.  A batch that is
        # EXPECTED to finish a lane (its frame limit falls in it) is waited for at once -- queuing past a known finish would only burn
        # frames on idle lanes.  0 = wait for every batch right after queuing it (the behaviour up to round 3; what a batch object
        # without poll_async gets).
        self.lookahead = 1 if hasattr(self.batch, "poll_async") else 0
        self._copy = None           # side stream the codes of streaming chunks are read out on while the look-ahead frames run
        self._polls: set = set()    # poll slots queued and not read yet (an abandoned run leaves some behind)
        # every context this scheduler will ever PREFILL into gets its workspace NOW: a lazy device allocation inside a staged
        # prefill would land in the middle of the running lanes' decode.  With spare contexts the lanes never prefill (they only
        # adopt), so their workspaces would be dead memory (~100 MB each at 0.6B / 2048 slots, ~380 MB at 1.7B / 6144).
        for e in ([st.engine for st in self.stages] if self.stages else list(engines)):
            reserve = getattr(e, "prefill_reserve", None)
            if reserve is not None:
                reserve()
        # requests staged together share ONE pass over the weights (fq3_prefill_batch; parity-tested at the engine level,
        # tests/test_gpu_decode.py).  Measured with the workspaces reserved up front (profiles/r03_packed_prefill.txt, 0.6B shapes,
        # 200-row prompts): first-wave TTFA 82.5 -> 63.6 ms at 8 lanes and 125 -> 89 ms at 16, aggregate 153.5 -> 156x / 229 -> 234x.
        self.packed_prefill = bool(packed_prefill)
        # PREFIX KV CACHE (fq3hip/prefix_cache.py; None = off): every prefill this scheduler queues goes through it -- the packed
        # groups through PrefixCache.prefill_pack, a single member through PrefixCache.prefill.  The cache serves THIS scheduler alone:
        # all its work is queued on the stream the scheduler prefills on (the side stream with spare contexts, the decode stream
        # without), which is what orders an evicted entry's blocks against their next tenant.
        self.prefix_cache = prefix_cache
        # FIRST WAVE (round 5): how many requests are prepared, prefilled and armed before the first frame is queued (None = one per lane,
        # the behaviour up to round 4).  With many lanes and many simultaneous requests, preparing all of them first puts every prompt
        # build and every prefill in front of EVERYBODY's first chunk (128 lanes: first-wave TTFA 348 ms, of which ~250 ms is that
        # queue); a first wave of 32 starts decoding after 32 of them and the others join at the following frame boundaries, staged
        # under the running frames (`stage_limit`: up to a quarter of the lanes per poll).  MEASURED on MI355X (profiles/r05_ttfa_first_wave.txt):
        # it does not help -- the followers' prefills run beside the first wave's frames and stretch them (128 lanes, wave of 32: first
        # chunks at 305 .. 513 ms against 340 ms for all 128 at once; end to end 1005x against 1025x) -- so None stays the default and
        # the knob is a measurement switch.  What the latency of N simultaneous requests is made of: ~35 ms + 2.35 ms per request
        # (prefill 1.1, first-chunk vocoder 0.6 - 0.7, prompt build 0.33, arming 0.09).
        self.first_wave: Optional[int] = None
        self.first_slice = 16                   # requests per slice of the pipelined first wave (_Run.stage_first_wave)
        # INCREMENTAL TEXT.  A feeder that has delivered nothing for `text_idle_timeout_s` seconds is closed by the scheduler: the
        # utterance ends the way whole text does and its lane and KV blocks come back.  30 s: an LLM that has not produced a token for
        # that long has stalled or gone, and the longest pause between two pieces of a live stream is well below it.
        self.text_idle_timeout_s: float = 30.0
        self.text_wait_s: float = 0.02          # bound of one host wait while no lane can advance (the source is polled in between)
        self._wake = threading.Event()          # set by every feeder of a text lane when it receives something
        # counters of the last run(): scheduler iterations, frames() calls, appends sent, host waits with nothing to decode, polls
        # that showed a held lane, polls that showed held and running lanes together, feeders closed by the idle rule
        self.text_stats: Dict[str, Any] = {}
        # host-time breakdown of the last run() (seconds; development aid, read by tools/batch_e2e_bench.py): where the scheduler's thread
        # spends its time between two batches of frames
        self.host_s: Dict[str, float] = {}

    def _side_stream(self, dev):
        """The prefill stream, made on first use: verified to run beside the decode (and vocoder) stream."""
        if self._side is None:
            from .streams import concurrent_stream
            self._side = concurrent_stream(dev, beside=self.beside)
        return self._side

    def _group_streams(self):
        """When the batch was told to advance several lane groups concurrently (``fq3_batch_set_option("groups")``, a measurement switch:
        one chain is faster at every lane count), the further groups' streams are ours, so that they share a hardware queue neither
        with the decode stream nor with the vocoder / prefill streams."""
        eng = self.lanes[0].engine
        n_groups = self.n_groups                                    # None: the library's choice (one chain)
        grouped = n_groups is not None and n_groups > 1
        if not grouped or not self._on_gpu(eng) or not hasattr(self.batch, "set_group_streams"):
            return
        from .streams import concurrent_stream
        if self.stages:
            self._side_stream(eng.device)
        self._group_side = [concurrent_stream(eng.device, beside=list(self.beside) + [self._side])]
        for _ in range(2, n_groups or 2):                           # further groups (measurement): beside the decode stream at least
            self._group_side.append(concurrent_stream(eng.device, beside=self._group_side))
        self.batch.set_group_streams(self._group_side)

    def _more(self, queue: list):
        """Pop the next event of a poll's batch; ``self.more_in_poll`` tells the consumer (read it right after receiving the event) how
        many more events of the SAME poll follow: utterances that finish / chunks that complete together can then be vocoded by one
        batched codec launch set.  (An attribute, not a timing key: the timing dicts keep exactly the reference's keys.)"""
        ev = queue.pop(0)
        self.more_in_poll = len(queue)
        return ev

    def set_predictor_policy(self, **policy):
        for ln in self.lanes:
            for k, v in policy.items():
                setattr(ln.predictor_graph, k, v)

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _kwargs(ln_pg, req: BatchRequest) -> Dict[str, Any]:
        kw = dict(max_new_tokens=2048, min_new_tokens=2, temperature=0.9, top_k=50, top_p=1.0, do_sample=True,
                  repetition_penalty=1.05)
        kw.update(req.gen_kwargs)
        # nucleus sampling (top_p < 1, sampling.py:57-65) is a per-lane policy of the loop state: the batch sampler kernels
        # branch to the LDS sorter for exactly the lanes that ask for it.  (Nothing here can fail: the values are validated by
        # fq3_decode_begin when the lane is armed.)
        return kw

    def _arm(self, ln: _Lane, req: BatchRequest):
        kw = self._kwargs(ln.predictor_graph, req)
        t0 = time.time()
        _eng, tn, pn, max_frames = _prefill_and_arm(
            req.talker, req.talker_input_embeds, req.attention_mask, req.trailing_text_hiddens, req.tts_pad_embed,
            req.config, ln.predictor_graph, ln.talker_graph, kw["max_new_tokens"], kw["min_new_tokens"],
            kw["temperature"], kw["top_k"], kw["top_p"], kw["do_sample"], kw["repetition_penalty"], use_graph=False,
            **({} if self.stages or self.prefix_cache is None else dict(cache=self.prefix_cache)),   # with spare contexts the cache lives on the side stream
            **self._seed_kw(self._seed_of(req)))
        self._seat(ln, req, tn, pn, max_frames, t0, (time.time() - t0) * 1000)

    def _seat(self, ln: _Lane, req: BatchRequest, tn, pn, max_frames: int, t_arm: float, prefill_ms: float):
        """The lane's new tenant, right after ``decode_begin``: it starts again at frame 0 with its own noise, seed and text table."""
        ln.req, ln.tn, ln.pn, ln.issued, ln.emitted, ln.max_frames = req, tn, pn, 0, 0, max_frames
        ln.seed = self._seed_of(req)
        ln.t_arm, ln.prefill_ms = t_arm, prefill_ms
        self._open_text(ln)

    @staticmethod
    def _seed_of(req):
        return validate_seed(getattr(req, "seed", None))

    @staticmethod
    def _seed_kw(seed) -> Dict[str, Any]:
        """``seed=`` for the generate.py helpers (a list for the packed ones) -- nothing at all when no request is seeded (the calls stay what they were)."""
        unseeded = all(s is None for s in seed) if isinstance(seed, list) else seed is None
        return {} if unseeded else dict(seed=seed)

    def _open_text(self, ln: _Lane):
        """Right after ``decode_begin``: a text-fed request's lane gets an open table of ``max_frames + 1`` rows (frame g reads row
        g < max_frames; the closing ``tts_eos`` row fits) and its feeder learns whom to wake."""
        ln.text = None
        req = ln.req
        if getattr(req, "text_feeder", None) is None or ln.max_frames <= 0:
            return
        if req.tts_eos_id is None:
            raise ValueError("a request with a text_feeder needs tts_eos_id")
        if int(req.trailing_text_hiddens.shape[-2]) != 0:
            raise ValueError("a request with a text_feeder carries an empty trailing table (the prompt holds the first token)")
        ln.engine.decode_text_open(ln.max_frames + 1)
        ln.text = _TextLane(req.text_feeder, int(req.tts_eos_id), ln.max_frames + 1, t_last=time.monotonic())
        req.text_feeder.waker = self._wake

    def _mark(self, engine):
        """Event after which the code tensors just read out are complete (recorded before further frames are queued)."""
        if not self._on_gpu(engine):
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(engine.device))
        return ev

    def _on_gpu(self, engine) -> bool:
        return torch.cuda.is_available() and getattr(engine.device, "type", "cpu") == "cuda"

    def _stage(self, st: _Stage, req: BatchRequest, req_ready=None):
        """Prefill + first token of ``req`` into the spare context, on the side stream (the host waits for the token, the
        main stream -- with lock-step frames already queued -- does not)."""
        self._stage_many([(st, req, req_ready)])

    def _stage_sync(self, upto=None):
        """The first tokens of the groups staged with ``defer=True``, oldest first: every group's tokens were copied to pinned host
        memory right behind its prefill (stream order), so reading group g waits for ITS prefill only -- the groups behind it keep the
        GPU busy while the host arms group g's lanes (round 6; until then ONE copy fetched all first tokens, and the GPU idled through
        the arming of a whole wave: 14 ms at 128 lanes).  ``upto``: stop once this stage's fields are complete (None = all groups)."""
        pend = self._unsynced
        while pend:
            group, kws, res, t0, host, done = pend.pop(0)
            if done is not None:
                done.synchronize()                                    # this group's prefill + its token copy; later groups still run
                toks = host.tolist()
            else:
                toks = torch.stack([r[0].reshape(()) for r in res]).cpu().tolist()
            ms = (time.time() - t0) * 1000
            hit = False
            for (st, req, _ev), kw, (_tok, hidden, n_rows, n_pad), tok in zip(group, kws, res, toks):
                st.req, st.kw, st.token, st.hidden, st.n_rows, st.n_pad = req, kw, int(tok), hidden, n_rows, int(n_pad)
                st.t0, st.prefill_ms = t0, ms
                hit = hit or st is upto
            if hit:
                break

    @staticmethod
    def _reserve_all(engines, items, kws, taken: list):
        """The KV blocks of every member's whole utterance (prompt + max_new_tokens + 1 slots, capped at max_seq_len) are taken
        BEFORE anything is queued: a short pool raises Fq3Error(FQ3_ENOMEM) here, and the caller returns the blocks of the contexts
        that ``taken`` lists.  Called on the stream the prefill runs on: the block-table entries are written by a launch on the
        CURRENT stream, and the prefill kernels read them."""
        for e, it, kw in zip(engines, items, kws):
            reserve = getattr(e, "kv_reserve", None)
            if reserve is not None:
                reserve(int(it[0].shape[1]) + int(kw["max_new_tokens"]) + 1)
                taken.append(e)

    @staticmethod
    def _row_groups(engines, items) -> Iterator[Tuple[int, int]]:
        """``(lo, hi)``: packed prefills share the leading context's workspace (max_seq_len rows): split the group where the rows run out."""
        lo, rows = 0, 0
        cap = int(getattr(engines[0], "max_seq_len", 1 << 30))
        for i, it in enumerate(items):
            n = int(it[0].shape[1])
            if i > lo and rows + n > cap:
                yield lo, i
                lo, rows = i, 0
            rows += n
        yield lo, len(items)

    @staticmethod
    def _left_pads(engines, items) -> List[int]:
        """Left padding of every prompt: one stack, one copy (the per-request int() of the synchronous path is a device wait each)."""
        from .generate import noted_n_pad
        masks = [it[1] for it in items]
        known = [0 if m is None else noted_n_pad(m) for m in masks]
        if all(k is not None for k in known):
            return [int(k) for k in known]                            # the prompt builder noted them: no device round trip at all
        return torch.stack([(m[0] == 0).sum() if m is not None else torch.zeros((), dtype=torch.long, device=engines[0].device) for m in masks]).cpu().tolist()

    def _prefill(self, engines, items, seeds, defer: bool) -> list:
        """``(first token, hidden, rows, left padding)`` per member, row group by row group (one member each without packed prefill)."""
        ck = {} if self.prefix_cache is None else dict(cache=self.prefix_cache)      # (nothing changes in the calls while it is off)
        cnt = self._left_pads(engines, items) if defer else None
        out = []
        for lo, hi in (self._row_groups(engines, items) if self.packed_prefill else [(i, i + 1) for i in range(len(items))]):
            if defer:
                out += _prefill_first_tokens_launch(engines[lo:hi], items[lo:hi], cnt[lo:hi], **ck, **self._seed_kw(seeds[lo:hi]))
            elif hi - lo > 1:
                out += _prefill_first_tokens_packed(engines[lo:hi], items[lo:hi], **ck, **self._seed_kw(seeds[lo:hi]))
            else:
                out.append(_prefill_first_token(engines[lo], *items[lo], **ck, **self._seed_kw(seeds[lo])))
        return out

    def _stage_many(self, group, defer: bool = False):
        """``[(spare context, request, ready event), ...]``: ONE packed prefill for the whole group when it has more than one
        member (``fq3_prefill_batch``: the layer weights are read once, not once per request).  ``defer`` (the pipelined first wave,
        GPU engines with packed prefill only): nothing is waited for -- the left-padding counts of the whole group cost one device
        round trip up front, the first tokens stay on the device until :meth:`_stage_sync` -- so the host goes on building the next
        prompts while these prefills run."""
        kws = [self._kwargs(self.lanes[0].predictor_graph, req) for _st, req, _ev in group]
        defer = bool(defer) and self.packed_prefill and self._on_gpu(group[0][0].engine)
        t0 = time.time()
        items = [(req.talker_input_embeds, req.attention_mask, req.config, kw["min_new_tokens"], kw["temperature"], kw["top_k"],
                  kw["top_p"], kw["do_sample"]) for (_st, req, _ev), kw in zip(group, kws)]
        engines = [st.engine for st, _req, _ev in group]
        taken: list = []
        host_toks = None
        seeds = [self._seed_of(req) for _st, req, _ev in group]
        try:
            if self._on_gpu(engines[0]):
                dev = engines[0].device
                side = self._side_stream(dev)
                for _st, _req, ev in group:
                    if ev is not None:
                        side.wait_event(ev)                                 # the request's tensors were produced on the main stream
                    else:
                        side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for st, _req, _ev in group:
                        if st.released is not None:
                            side.wait_event(st.released)                    # the previous tenant's hand-over has been queued
                    self._reserve_all(engines, items, kws, taken)
                    res = self._prefill(engines, items, seeds, defer)
                    if defer:
                        # the group's first tokens go to pinned host memory right behind its prefill: no wait here
                        flat = torch.stack([r[0].reshape(()) for r in res])
                        host_toks = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
                        host_toks.copy_(flat, non_blocking=True)
                    done = self._mark(engines[0])                           # (the current stream is the side stream here)
                for st, _req, _ev in group:
                    st.ready = done
            else:
                self._reserve_all(engines, items, kws, taken)
                res = self._prefill(engines, items, seeds, defer)
        except Exception:
            for e in taken:                                                 # a short pool or a failed prefill: nobody keeps blocks
                e.kv_release()
            raise
        if defer:
            for (st, req, _ev), kw in zip(group, kws):
                st.req, st.kw, st.token = req, kw, None               # (the stage is taken; token / hidden follow in _stage_sync)
            self._unsynced.append((group, kws, res, t0, host_toks, group[0][0].ready if host_toks is not None else None))
            return
        ms = (time.time() - t0) * 1000
        for (st, req, _ev), kw, (token, hidden, n_rows, n_pad) in zip(group, kws, res):
            st.req, st.kw, st.token, st.hidden, st.n_rows, st.n_pad = req, kw, token, hidden, n_rows, int(n_pad)
            st.t0, st.prefill_ms = t0, ms

    def _admit(self, ln: _Lane, st: _Stage):
        """Hand a staged request to a free lane at a frame boundary: the block-table hand-over (one tiny launch; a block-wise copy
        if the two contexts do not share a pool) + the arm kernel."""
        req, kw = st.req, st.kw
        gpu = self._on_gpu(ln.engine)
        if gpu:
            main = torch.cuda.current_stream(ln.engine.device)
            main.wait_event(st.ready)
            st.hidden.record_stream(main)
        ln.engine.kv_adopt(st.engine, st.n_rows)
        if gpu:
            st.released = self._mark(ln.engine)
        _eng, tn, pn, max_frames = _arm_decode(
            req.talker, req.config, st.token, st.hidden, st.n_rows, req.attention_mask, req.trailing_text_hiddens, req.tts_pad_embed,
            ln.predictor_graph, ln.talker_graph, kw["max_new_tokens"], kw["min_new_tokens"], kw["temperature"], kw["top_k"],
            kw["top_p"], kw["do_sample"], kw["repetition_penalty"], use_graph=False, n_pad=st.n_pad, **self._seed_kw(self._seed_of(req)))
        st.req, st.kw, st.hidden = None, None, None
        self._seat(ln, req, tn, pn, max_frames, st.t0, st.prefill_ms)

    def _feed_text(self, lanes: List[_Lane]) -> int:
        """Drain every text lane's feeder without blocking and send ONE append for all of them (the closing ``tts_eos`` row and the
        capacity clamp are those of ``TextSession._append``).  Returns the number of lanes that received something."""
        items = []
        now = time.monotonic()
        for ln in lanes:
            t = ln.text
            if t is None or t.closed:
                continue
            waited = getattr(t.feeder, "t_oldest", None)
            ids, fin = t.feeder.take(block=False)
            if ids and waited is not None:
                # arrival of the oldest id -> its append is queued (what the device adds: the frames queued ahead, <= lookahead + 1 batches)
                ms = (now - waited) * 1000
                self.text_stats["append_wait_n"] += 1
                self.text_stats["append_wait_ms_sum"] += ms
                self.text_stats["append_wait_ms_max"] = max(self.text_stats["append_wait_ms_max"], ms)
            if ids or fin:
                t.t_last = now
            elif now - t.t_last > self.text_idle_timeout_s:
                t.feeder.close()                                     # a stalled client: the utterance ends like whole text
                ids, fin = t.feeder.take(block=False)
                fin = True
                self.text_stats["idle_closed"] += 1
            if not (ids or fin):
                continue
            room = t.capacity - t.rows
            if fin:
                ids = list(ids) + [t.eos_id]
            if len(ids) >= room:                                     # the loop cannot reach further rows: close here
                ids, fin = ids[:room], True
            items.append((ln.index, ids, fin))
            t.rows += len(ids)
            t.closed = t.closed or fin
        if items:
            self.batch.text_append(items)
            self.text_stats["appends"] += 1
        return len(items)

    @staticmethod
    def _avail(ln: _Lane) -> int:
        """Frames the lane can have emitted once everything queued so far has run."""
        t = ln.text
        return ln.max_frames if t is None or t.closed else min(t.rows, ln.max_frames)

    def _drop_blocks(self, x, cancel: bool = False):
        """Return whatever KV blocks lane / stage ``x`` owns to the pool (a lane's device loop is cancelled first when asked: a lane that
        was armed must not append to blocks it no longer owns)."""
        eng = x.engine
        try:
            if cancel and getattr(eng, "decode_cancel", None) is not None:
                eng.decode_cancel()
            if getattr(eng, "kv_release", None) is not None:
                eng.kv_release()
        except Exception:
            pass

    def _discard_polls(self, slots):
        """Read and drop polls nobody will look at: a slot must have been read before it is armed again."""
        for slot in slots:
            self.batch.poll_wait(slot)
            self._polls.discard(slot)

    def _fetch(self, ln: _Lane, first: int, count: int, ev_done=None):
        """``(codes LongTensor[count, 16] from frame `first`, event after which they are complete)``.  With look-ahead frames in flight
        (``ev_done``: the event behind the batch that produced them) the read-out runs on the copy stream, beside those frames."""
        eng = ln.engine
        if self._copy is None or ev_done is None:
            return eng.decode_codes(first, count), self._mark(eng)
        with torch.cuda.stream(self._copy):
            self._copy.wait_event(ev_done)
            codes = eng.decode_codes(first, count)
            ev = torch.cuda.Event()
            ev.record(self._copy)
        ln.copied = ev
        return codes, ev

    def _finish(self, ln: _Lane, n: int, chunked: bool = False, ev_done=None) -> Tuple[Any, Optional[torch.Tensor], Dict[str, float]]:
        first = ln.emitted if chunked else 0
        ready_ev = None
        if n > first:
            if chunked:
                codes, ready_ev = self._fetch(ln, first, n - first, ev_done)
            else:
                codes = ln.engine.decode_codes(first, n - first)
        elif chunked and n > 0:                      # every frame already went out as a partial chunk
            codes = torch.empty(0, ln.engine.cfg.num_code_groups, dtype=torch.long, device=ln.engine.device)
        else:
            codes = None
        wall = time.time() - ln.t_arm
        timing = {"prefill_ms": ln.prefill_ms, "decode_s": max(wall - ln.prefill_ms / 1000, 0.0), "steps": n,
                  "ms_per_step": (1000 * wall / n) if n else 0.0, "steps_per_s": (n / wall) if wall > 0 else 0.0}
        if chunked:
            timing.update(is_final=True, total_steps_so_far=n)
            if codes is not None:
                timing["codes_ready_event"] = ready_ev if ready_ev is not None else self._mark(ln.engine)
        rid = ln.req.rid
        ln.req, ln.tn, ln.pn, ln.emitted, ln.text = None, None, None, 0, None
        # the lane's KV blocks go back to the pool now: the poll that found it finished waited for its last frame, and a done lane never
        # touches the cache again -- not in look-ahead frames still in flight either (done-lane guard, csrc/batch_kernels.cuh)
        release = getattr(ln.engine, "kv_release", None)
        if release is not None:
            release()
        return rid, codes, timing

    def _reset(self):
        """A previous run() may have been abandoned mid-utterance (a streaming consumer that stopped early, an exception in the
        caller): no lane carries a tenant, a partial-chunk counter or a staged request over into this one."""
        abandoned = [x for x in list(self.lanes) + list(self.stages)
                     if x.req is not None or getattr(x.engine, "kv_blocks", lambda: 0)() > 0]
        if abandoned:
            for x in abandoned:
                cancel = getattr(x.engine, "decode_cancel", None)
                if cancel is not None and isinstance(x, _Lane):
                    cancel()                                  # the device loop state stops at once instead of decoding to its own EOS
            if self._on_gpu(self.lanes[0].engine):
                torch.cuda.current_stream(self.lanes[0].engine.device).synchronize()       # its queued frames are over: the blocks may go
                if self._side is not None:
                    self._side.synchronize()
            for x in abandoned:
                release = getattr(x.engine, "kv_release", None)
                if release is not None:
                    release()
        self._discard_polls(sorted(self._polls))          # polls an abandoned run queued and never read
        self._unsynced = []                               # (first tokens an abandoned run left on the device: their stages are reset below)
        for ln in self.lanes:
            ln.req, ln.tn, ln.pn, ln.issued, ln.emitted, ln.text, ln.seed = None, None, None, 0, 0, None, None
        self._wake.clear()
        for st in self.stages:
            st.req, st.kw, st.hidden = None, None, None

    @torch.inference_mode()
    def run(self, requests: Iterable[BatchRequest], on_error: str = "raise",
            source: Optional[Callable[[], Optional[BatchRequest]]] = None, chunk_frames: Optional[int] = None
            ) -> Iterator[Tuple[Any, Optional[torch.Tensor], Dict[str, Any]]]:
        """Yields ``(rid, codes LongTensor[T, 16] or None, timing)`` as utterances finish (not in request order).
        ``on_error="yield"``: a request that cannot be armed (prompt longer than ``max_seq_len``, ...)
        is reported as ``(rid, None, {"error": repr(exc), "steps": 0})`` and the other lanes keep going; the default
        re-raises, like the single-utterance entry points.  ``source``: polled without blocking at every frame boundary
        for requests that arrived after the call (``None`` = nothing waiting): a server's inbox.
        ``chunk_frames``: streaming mode -- besides the final event every utterance yields partial events
        ``(rid, codes of the next whole chunks, {"is_final": False, "total_steps_so_far": n})`` as its frames complete, and
        its final event (``"is_final": True``) carries only the frames not handed out before (``None`` when the utterance
        produced no frame at all, an empty tensor when everything was already handed out)."""
        if on_error not in ("raise", "yield"):
            raise ValueError("on_error must be 'raise' or 'yield'")
        self._reset()
        yield from _Run(self, requests, on_error, source, chunk_frames).loop()


class _Run:
    """One call of ``BatchDecoder.run()``.  A request moves ``pending`` -> (a spare context from ``idle``, then ``ready``) -> a lane from
    ``free`` -> ``active``; a batch of frames moves through ``inflight`` until its poll is read, and what the poll found waits in ``outbox``
    until the next frames are queued.  The methods are the phases of :meth:`loop`, in its order."""

    def __init__(self, dec: BatchDecoder, requests, on_error: str, source, chunk_frames):
        self.dec, self.on_error, self.source = dec, on_error, source
        self.chunk_frames = int(chunk_frames) if chunk_frames is not None and int(chunk_frames) > 0 else None
        self.gpu = gpu = dec._on_gpu(dec.lanes[0].engine)
        self.stats = dec.text_stats = dict(iterations=0, frames_calls=0, appends=0, idle_waits=0, polls_held=0, polls_mixed=0, idle_closed=0,
                                           append_wait_n=0, append_wait_ms_sum=0.0, append_wait_ms_max=0.0)
        self.pending = deque(self.stamped(r) for r in requests)
        self.free = deque(dec.lanes)
        self.active: List[_Lane] = []
        self.idle = deque(dec.stages)
        self.ready: deque = deque()
        self.failed: List[Tuple[Any, None, Dict[str, Any]]] = []      # error events of requests that could not be staged
        self.outbox: List[Tuple[Any, Any, Dict[str, Any]]] = []       # streaming-mode events waiting for the next frames to be queued
        self.prof = dec.host_s = {"stage": 0.0, "admit": 0.0, "queue": 0.0, "poll_wait": 0.0, "digest": 0.0, "consumer": 0.0}
        # Requests taken from the source / staged per batch of frames while lanes decode.  A floor that keeps long utterances flowing
        # (lanes / 16 per poll refills every lane within 16 polls = 128 frames; two per poll -- the rule up to round 3 -- starves a
        # scheduler of more than ~50 lanes at 200-frame utterances: 128 lanes ran half empty), topped up by DEMAND: lanes that are
        # free now, lanes whose frame limit falls within the next four polls, and the recent rate of early (EOS) finishes, minus what
        # is staged already -- at most a quarter of the lanes per poll, so that the host work of one poll stays inside the batch of
        # frames queued ahead.  Short utterances (a 48-lane scheduler of 40-frame utterances turns over every 5 polls) are what
        # needs the top-up.
        self.per_poll = max(2, (len(dec.lanes) + 15) // 16)
        self.per_poll_cap = max(self.per_poll, len(dec.lanes) // 4)
        self.finish_rate = 0.0                                        # finishes per poll, exponentially averaged
        # (four poll slots, indexed by the batch number modulo 4: with `depth` batches unread and one being queued, depth <= 3 keeps a slot
        # from being re-armed before its poll has been read)
        self.depth = max(0, min(int(dec.lookahead), 3)) if hasattr(dec.batch, "poll_async") else 0
        dev = dec.lanes[0].engine.device
        self.feed_stream = dec._side_stream(dev) if gpu and dec.stages else None
        if self.chunk_frames and self.depth and gpu and dec._copy is None:
            # streaming: the codes of a chunk are read out beside the look-ahead frames, not behind them -- on the consumer's own stream
            # (the vocoder's, `beside[0]`: hardware queues are few), else on a stream probed for a queue of its own
            if dec.beside:
                dec._copy = dec.beside[0]
            else:
                from .streams import concurrent_stream
                dec._copy = concurrent_stream(dev, beside=[dec._side])
        self.inflight: deque = deque()      # batches of frames whose poll has not been read yet: (batch index, poll slot | None, event | None, model)
        self.batch_no = 0

    def stamped(self, req):
        """(request, event after which its tensors are ready): recorded on the main stream when the request arrives, so
        a side-stream prefill waits for THAT, not for the lock-step frames queued later."""
        return req, (self.dec._mark(self.dec.lanes[0].engine) if self.gpu and self.dec.stages else None)

    def stage_limit(self) -> int:
        """Requests to stage in this poll (the source is asked for what `pending` does not hold already)."""
        horizon = 4 * self.dec.poll_every
        soon = sum(1 for ln in self.active if ln.max_frames - ln.issued <= horizon)
        need = len(self.free) + soon + int(self.finish_rate + 0.999) - len(self.ready)
        return max(self.per_poll, min(need, self.per_poll_cap))

    def pull(self, cap: Optional[int] = None, on_main: bool = False):
        # while lanes decode, at most two new requests per frame boundary: whatever the source does to produce one (a
        # model's prompt build, say) runs on the host between two batches of queued frames.  Before anything decodes: only
        # what the first wave can take (one request per lane) -- every further prompt built now would delay the first frame
        dec, source, pending = self.dec, self.source, self.pending
        wave = len(dec.lanes) if dec.first_wave is None else max(1, min(int(dec.first_wave), len(dec.lanes)))
        budget = max(0, wave - len(pending) - len(self.ready)) if not self.active else max(0, self.stage_limit() - len(pending))
        if cap is not None:
            budget = min(budget, int(cap))
        if source is None or budget <= 0:
            return
        # with spare contexts the source runs under the PREFILL stream: whatever device work it does to produce a request (a
        # model's prompt build) neither queues behind the lock-step frames in flight nor -- where it waits for a value --
        # makes the host wait for them; the staged prefill that consumes it is on that stream anyway
        # (first wave, `on_main`: nothing decodes, the MAIN stream is idle -- the builder's host-to-device uploads are synchronous
        # copies, and on the prefill stream each would wait for the packed prefill queued in front of it)
        with torch.cuda.stream(None if on_main else self.feed_stream):           # (no stream: the context changes nothing)
            while budget > 0 and len(pending) < len(dec.lanes) + len(dec.stages):
                r = source()
                if r is None:
                    break
                pending.append(self.stamped(r))
                budget -= 1

    def stage_first_wave(self, slice_n: int):
        # FIRST WAVE, pipelined (round 5): nothing decodes yet, so the critical path to the first frame is "build the prompts (host)" +
        # "prefill them (GPU)".  They used to run one after the other (128 lanes: 39 ms + 96 ms); now the prompts arrive in slices and
        # every slice's packed prefill is QUEUED without waiting for its first tokens (`defer`), so the host builds slice k + 1 while the
        # GPU prefills slice k; one copy fetches all first tokens before the lanes are armed.
        t_ = _clock()
        try:
            while self.pending:                                   # nothing is decoding: nothing to overlap with but the prompt builds
                if self.stage_ahead(defer=True) == 0:
                    break
                self.pull(cap=slice_n, on_main=True)
        except BaseException:
            # the deferred stages hold a request but not yet its first token / hidden state: complete them when the interleaved
            # pull() (the caller's source) raised, so that no stage is left half-filled for the cleanup to find
            self.dec._stage_sync()
            raise
        # (no wait here: the admission loop reads each group's first tokens when it reaches the group's first stage, and
        # arms its lanes while the groups behind it are still being prefilled)
        self.prof["stage"] += _clock() - t_

    def stage_ahead(self, limit: int = 1 << 30, defer: bool = False) -> int:
        # while lanes decode, only a couple of prefills per batch of queued frames: the host waits for the staged requests'
        # first tokens, and the main stream must not run dry meanwhile.  Requests staged together are prefilled together.
        idle, pending, ready = self.idle, self.pending, self.ready
        group = [(idle.popleft(), *pending.popleft()) for _ in range(min(limit, len(pending), len(idle)))]
        if not group:
            return 0
        try:
            self.dec._stage_many(group, defer=defer)
            ready.extend(st for st, _r, _e in group)
            return len(group)
        except Exception as exc:
            if len(group) == 1 or self._pool_is_short(exc):           # nothing to isolate, or all of them wait for blocks
                self._not_staged(group, exc)
                return 0
        # a packed group failed (one prompt too long, the pool too short for all of them, ...): stage its members one by one so
        # that only the culprit fails
        for n, member in enumerate(group):
            try:
                self.dec._stage_many([member])
                ready.append(member[0])
            except Exception as exc:
                if self._pool_is_short(exc):
                    self._not_staged(group[n:], exc)                  # keep the order: nothing overtakes a postponed request
                    return n
                self._not_staged([member], exc)
        return len(group)

    def _pool_is_short(self, exc) -> bool:
        return getattr(exc, "code", None) == FQ3_ENOMEM and bool(self.active or self.ready)

    def _not_staged(self, members, exc):
        """What becomes of requests whose staging failed (everything but a pool that is short is one member's failure)."""
        if self._pool_is_short(exc):
            # the KV pool is short right now: lanes that finish give blocks back -- keep the requests (in order) for later
            for st, req, ev in reversed(members):
                self.idle.appendleft(st)
                self.pending.appendleft((req, ev))
            return
        st, req, _ev = members[0]
        self.idle.appendleft(st)
        if self.on_error == "raise":
            raise exc
        self.failed.append((req.rid, None, {"error": repr(exc), "steps": 0}))

    def report_failed(self):
        while self.failed:
            yield self.dec._more([self.failed.pop(0)])                # (an event that shares its poll with no other)

    def admit(self):
        """Admit at a frame boundary: every free lane takes the oldest staged request (without spare contexts: prefills the oldest
        pending one itself).  Returns the number of lanes it tried."""
        dec, free, ready, pending, idle = self.dec, self.free, self.ready, self.pending, self.idle
        t_admit = _clock()
        moved = 0                                                     # requests admitted / staged in this iteration
        while free and (ready or (pending and not dec.stages)):
            ln = free.popleft()
            moved += 1
            try:
                # a side-stream read of this lane's code buffer (streaming look-ahead) must be over before a new tenant's frames overwrite it
                if ln.copied is not None:
                    torch.cuda.current_stream(ln.engine.device).wait_event(ln.copied)
                    ln.copied = None
                if ready:
                    st = ready.popleft()
                    rid = st.req.rid
                    try:
                        if st.token is None:
                            dec._stage_sync(upto=st)                  # a deferred group: its first tokens (and only its) are waited for
                        dec._admit(ln, st)
                    finally:
                        idle.append(st)
                else:
                    req, _ev = pending.popleft()
                    rid = req.rid
                    dec._arm(ln, req)
                ln.first_batch = self.batch_no                        # the frames queued from now on are this tenant's
            except Exception as exc:
                free.appendleft(ln)
                # the lane may already own blocks (the hand-over of a staged request, or its own prefill, came before the step that
                # failed -- fq3_decode_begin rejecting a sampling argument, say): it has no tenant, so nothing else would return them
                dec._drop_blocks(ln, cancel=True)
                if self.on_error == "raise":
                    raise
                yield dec._more([(rid, None, {"error": repr(exc), "steps": 0})])
                continue
            if ln.max_frames <= 0:
                yield dec._more([dec._finish(ln, 0, self.chunk_frames is not None)])
                free.append(ln)
            else:
                self.active.append(ln)
        self.prof["admit"] += _clock() - t_admit
        return moved

    def queue_frames(self):
        """Queue the next batch of frames and its poll.  Returns ``(the text lanes, the lanes that could be given frames)``."""
        dec, active = self.dec, self.active
        # lock-step frames, never across a lane's noise-ring boundary (each lane refills its own rings); lanes whose frame limit is
        # already covered by the frames in flight need no more (they wait for their poll)
        need = [ln for ln in active if ln.issued < ln.max_frames]
        t_ = _clock()
        texted = [ln for ln in active if ln.text is not None]
        if texted:
            # text that arrived since the last batch: ONE append for all lanes, in stream order in front of the frames below.  A
            # text lane whose next row is still missing cannot advance: it neither bounds the step nor -- when no lane can
            # advance -- gets frames queued at all (they would all be holds)
            dec._wake.clear()
            dec._feed_text(texted)
            need = [ln for ln in need if dec._avail(ln) > ln.issued]
        if need:
            step = dec.poll_every
            seeded = []                                               # seeded lanes at a ring boundary: ONE fill for all of them below
            for ln in need:
                if ln.text is None:
                    at_boundary = ln.issued % NOISE_RING == 0
                else:
                    # once per 64 EMITTED frames: every frame before the boundary is in front of this in the stream, and a lane
                    # that sat held on the boundary comes here once, when it can go on
                    at_boundary = ln.issued % NOISE_RING == 0 and ln.text.refilled_at != ln.issued
                    if at_boundary:
                        ln.text.refilled_at = ln.issued
                if at_boundary and ln.seed is None:
                    _refill(ln.engine, ln.tn, ln.pn)
                elif at_boundary and (ln.tn is not None or ln.pn is not None):
                    seeded.append((ln.engine, ln.tn, ln.pn, ln.seed, ln.issued, None))
                step = min(step, NOISE_RING - ln.issued % NOISE_RING, max(ln.max_frames - ln.issued, 1))
            if seeded:
                type(seeded[0][0]).noise_fill_many(seeded, NOISE_RING)
            self.pull()                                               # stamp new arrivals before the frames are queued
            dec.batch.frames(step)
            self.stats["frames_calls"] += 1
            model = {}
            for ln in active:
                if ln.text is None:
                    if ln.issued < ln.max_frames:
                        ln.issued += step
                else:
                    # the hold rule on the host: the lane emits until its rows (or its frame limit) run out and holds there
                    got = min(ln.issued + step, dec._avail(ln))
                    model[ln.index] = (got, got < ln.issued + step and got < ln.max_frames)
                    ln.issued = got
            slot = ev_done = None
            if self.depth:
                slot = self.batch_no % 4
                dec.batch.poll_async(slot)                            # in stream order: behind these frames, in front of the next batch
                dec._polls.add(slot)
                if dec._copy is not None and self.chunk_frames is not None:
                    ev_done = dec._mark(dec.lanes[0].engine)
            self.inflight.append((self.batch_no, slot, ev_done, model))
            self.batch_no += 1
        self.prof["queue"] += _clock() - t_
        return texted, need

    def hand_out(self):
        while self.outbox:
            yield self.dec._more(self.outbox)

    def wait_polls(self, need):
        # wait for the oldest batch; for ALL of them when a lane's frame limit falls in the newest (a finish is expected: queuing
        # past it would burn frames on idle lanes) or when nothing more could be queued
        inflight, prof = self.inflight, self.prof
        expect = any(ln.issued >= ln.max_frames for ln in self.active)
        while inflight and (len(inflight) > self.depth or expect or not need):      # (`need`: the lanes that could be given frames)
            t_, w_ = _clock(), prof["poll_wait"]
            self.digest(inflight.popleft())
            prof["digest"] += _clock() - t_ - (prof["poll_wait"] - w_)
            if not self.active:                                       # frames queued past the last finish: nothing left to read in them
                self.dec._discard_polls([slot for _b, slot, _e, _m in inflight if slot is not None])
                inflight.clear()

    def digest(self, entry):
        """Read one batch's poll: chunk events and finishes of the lanes that were armed before it was queued."""
        dec, active, outbox, c = self.dec, self.active, self.outbox, self.chunk_frames
        bno, slot, ev_done, model = entry
        if slot is not None:
            t_ = _clock()
            # waits for THIS batch's frames only: later ones keep running.  (With text lanes in the batch the states come as ints:
            # 2 = held on its open table, which is "running" here -- poll_wait folds it into True.)
            n_all, d_all = dec.batch.poll_wait_states(slot) if model else dec.batch.poll_wait(slot)
            self.prof["poll_wait"] += _clock() - t_
            dec._polls.discard(slot)
        still = []
        seen_held = seen_run = False
        for ln in active:
            if ln.first_batch > bno:                                    # armed after this batch was queued: the poll shows its predecessor
                still.append(ln)
                continue
            if slot is not None:
                n, done = n_all[ln.index], d_all[ln.index]
            elif ln.text is not None:
                n, done = ln.engine.decode_poll_state()
            else:
                n, done = ln.engine.decode_poll()
            if ln.index in model:
                # the host's model of the hold rule against the device: a lane that ended (EOS, position limit) may be behind
                # the model, never ahead; a running or held lane is exactly where the model says
                want_n, want_held = model[ln.index]
                state = int(done)
                ok = (n <= want_n) if state == 1 else (n == want_n and (state == 2) == want_held)
                if not ok:
                    raise RuntimeError(f"lane {ln.index}: the poll shows {n} frames, state {state}; the host's model of the text "
                                       f"hold rule has {want_n} frames, {'held' if want_held else 'running'} (noise rings out of step)")
                seen_held = seen_held or state == 2
                seen_run = seen_run or state == 0
                done = state == 1                                   # held is running
            elif slot is not None and model:
                seen_run = seen_run or int(done) == 0
                done = int(done) == 1
            fin = done or n >= ln.max_frames
            if c is not None:
                # whole chunks, one event each (a poll can complete several); a finished utterance's last event carries
                # the remainder (at most one chunk) and the timing
                upto = n if fin else (n // c) * c
                while (upto - ln.emitted > c) if fin else (upto - ln.emitted >= c):
                    codes, ready_ev = dec._fetch(ln, ln.emitted, c, ev_done)
                    ln.emitted += c
                    outbox.append((ln.req.rid, codes, {"is_final": False, "total_steps_so_far": ln.emitted,
                                                       "codes_ready_event": ready_ev}))
            if fin:
                # like the chunk events, a finish goes out only once the next frames are queued: whatever the consumer does with
                # it (a vocoder launch set for a whole wave of utterances is ~15 ms of host time) then runs beside the decode of
                # the lanes' next tenants instead of in front of it
                outbox.append(dec._finish(ln, n, c is not None, ev_done))
                self.free.append(ln)
            else:
                still.append(ln)
        self.finish_rate = 0.5 * self.finish_rate + 0.5 * (len(active) - len(still))
        self.active = still
        self.stats["polls_held"] += int(seen_held)
        self.stats["polls_mixed"] += int(seen_held and seen_run)

    def loop(self):
        dec, prof, stats = self.dec, self.prof, self.stats
        slice_n = max(1, int(dec.first_slice))
        while True:
            stats["iterations"] += 1
            first_wave_phase = bool(dec.stages) and not self.active and not self.ready and not self.inflight
            self.pull(cap=slice_n if first_wave_phase else None, on_main=first_wave_phase)
            if not (self.pending or self.active or self.ready or self.failed or self.inflight):
                break
            if dec.stages and not self.active and not self.ready:
                self.stage_first_wave(slice_n)
            yield from self.report_failed()
            moved = yield from self.admit()
            if not self.active and not self.inflight:
                continue
            if dec.use_graph and not dec._captured:
                dec._group_streams()
                dec.batch.graph_capture()
                dec._captured = True
            texted, need = self.queue_frames()
            # the chunks and finishes found by the previous poll go out only now, with the next frames already queued, so
            # that whatever the consumer does with them (vocoding) overlaps the decode instead of stalling it
            t_ = _clock()
            yield from self.hand_out()
            prof["consumer"] += _clock() - t_
            if dec.stages and self.active:
                t_ = _clock()
                moved += self.stage_ahead(limit=self.stage_limit())   # prefills fly under the frames queued above
                prof["stage"] += _clock() - t_
            self.wait_polls(need)
            if self.inflight or (not self.active and not self.ready and not self.pending):   # frames are running (or nothing is left to overlap with)
                yield from self.hand_out()
            if texted and self.active and not need and not self.inflight and not moved:
                # every active lane waits for text and nothing is queued: what the last poll found goes out, then the host sleeps
                # until a feeder receives something -- bounded, so that the source and the idle rule are looked at in between.
                # No frame is queued meanwhile: nothing spins on the GPU.
                yield from self.hand_out()
                stats["idle_waits"] += 1
                dec._wake.wait(dec.text_wait_s)
        yield from self.hand_out()
        yield from self.report_failed()                               # belt and braces: no error event is ever dropped
