"""One call of ``FasterQwen3TTS._run_batch_streaming``: the event loop over the lock-step decode and the device work of a launch
group, a named step per audio stage.  The order of the launches and of the hand-out is ``stream_groups.StreamGroups``; this module
is what it calls (DESIGN.md sections 4.17 and 4.19)."""
from __future__ import annotations

import contextlib
from typing import Any, NamedTuple

import numpy as np
import torch

from .stream_groups import ExactDecode, StreamGroups, WindowDecode, landing_plan, push_runs, runs_of


class Landing(NamedTuple):
    """what ``launch`` hands to ``collect``"""
    host: Any                     # pinned memory: one tensor of the group's shape, or one span or None per row; None: nothing was copied
    landed: Any                   # the event behind the last copy, None: the rows stay on the device
    wav: Any                      # the rows on the device: one tensor, or one tensor per row
    encoded: Any                  # [(rows, GroupCopy)] per run for the rows with an output spec, or None


class BatchStreamRun:
    """Built once per call, behind the argument checks.  :meth:`events` is the generator the entry point hands on; :meth:`launch` and
    :meth:`collect` are the device work ``StreamGroups`` calls, ``launch`` as the steps ``_wait_inputs`` / ``_decode`` / gain /
    ``_level`` / ``_mark`` / ``_limit`` / ``_encode`` / ``_land``."""

    def __init__(self, model, prepared, gen_kwargs, chunk_size: int, lanes: int, rounds, stamp, seeds, device_audio: bool, outputs,
                 group_marks: bool, marks):
        from .model import _SideVocoder
        self.model, self.chunk_size = model, chunk_size
        self.stamp, self.device_audio, self.outputs, self.group_marks, self.marks = stamp, device_audio, outputs, group_marks, marks
        self.gain = None if device_audio else model._gain_tensor()       # (long form multiplies behind the join)
        self.limit = None if device_audio else getattr(model, "_limit", None)      # (and limits there, as one stream)
        self.lvl = None if device_audio else getattr(model, "_lvl", None)         # (and levels there, likewise)
        self.meta: dict = {}
        self.vocs, self.n_chunks = {}, {}
        self.dec = dec = model._batch_decoder(lanes)
        # ``batch_first_wave_streaming`` (attribute, default None = one request per lane): requests prepared and prefilled in front of the
        # first frame, the others joining at the following frame boundaries.  MEASURED (profiles/r05_ttfa_first_wave.txt): a smaller
        # first wave does not buy its members a lower latency -- the prefills of the followers run beside their first frames and
        # stretch them (128 lanes: p25 305 ms / p50 395 ms at a wave of 32 against 340 ms for everybody at once) -- so the default stays.
        dec.first_wave = getattr(model, "batch_first_wave_streaming", None)
        self.pairs = (rounds(dec, self.meta) if rounds is not None
                      else [model._batch_feed(prepared, gen_kwargs, len(dec.lanes), self.meta, dec.first_wave, seeds)])
        self.tok = tok = model.model.model.speech_tokenizer
        self.side = model._vocoder_stream(tok)
        self.batched = self.side is not None and hasattr(tok, "decode_tensor_batch")
        # chunks of different utterances that need the SAME decode shape (the first chunks of lanes that started together: reference + 8
        # frames in, the last 8 frames' samples out) go through one batched launch set on the vocoder stream, STREAM_GROUP at a time.
        # Round 6: a group is LAUNCHED as soon as it is full -- while the host still prepares the next group's inputs -- every group's
        # waveform goes to pinned host memory behind its launch set, and the groups are handed out one by one as their copies land: a
        # wave of 128 first chunks (four groups of 32) used to be prepared as a whole, launched group by group with a host wait after
        # each, and reached the caller all at once after the last group.  The bookkeeping -- the jobs of a poll ``[rid, meta, audio |
        # None, WindowDecode | ExactDecode | None]``, their classes, the launches made -- is ``stream_groups.StreamGroups``; ``launch`` and
        # ``collect`` below are the device work it calls.  Per utterance the order of the events is kept BY THE LAUNCHES, in both modes: a
        # launch pushes its members' own stages and stream states, so a chunk never joins a class that would launch in front of an
        # earlier chunk of its utterance that still waits (lanes re-used at staggered frames produce that; the classes up to that
        # chunk's are launched first).  Groups are handed out in launch order, markers without audio come last.
        self.groups = StreamGroups(self.launch, self.collect, _SideVocoder.STREAM_GROUP, getattr(tok, "stream_ctx_max", None))
        model._stream_group_stats = self.groups.stats   # the counters of the newest run (jobs, launches, order_launches), nothing else kept

    # ---- the event loop -----------------------------------------------------------------------------------------------------------
    def events(self):
        dec = self.dec
        for head, source in self.pairs:
            for rid, codes, info in dec.run(head, source=source, chunk_frames=self.chunk_size):
                voc = self._vocoder(rid)
                ev = info.pop("codes_ready_event", None)
                final = bool(info.get("is_final"))
                more = int(getattr(dec, "more_in_poll", 0))
                out_meta = dict(chunk_index=self.n_chunks[rid], total_steps_so_far=int(info.get("total_steps_so_far", 0)),
                                is_final=final, chunk_steps=0 if codes is None else int(codes.shape[0]))
                if codes is not None and codes.shape[0] > 0:
                    self._chunk(rid, voc, out_meta, codes, ev, final)
                elif final:
                    self._final_marker(rid, voc, out_meta, codes)
                if more <= 0:
                    yield from self._hand_out()
            yield from self._hand_out()

    def _vocoder(self, rid):
        """utterance ``rid``'s ``StreamingVocoder``, made at its first event: with its output spec and stage, its mark spec and pool"""
        voc = self.vocs.get(rid)
        if voc is None:
            from .model import StreamingVocoder
            model, outputs, marks = self.model, self.outputs, self.marks
            voc = self.vocs[rid] = (StreamingVocoder(self.tok, self.meta[rid], self.chunk_size, model.device, self.side, **model._exact_kw())
                                    if self.device_audio else model.streaming_vocoder(self.meta[rid], self.chunk_size))
            if outputs is not None and outputs[rid] is not None:
                voc.output, voc.stage = outputs[rid], model._take_stage(outputs[rid], self.side)
            if marks is not None and marks[rid] is not None:
                voc.mark_spec = marks[rid]
                voc.mark_pool = model.__dict__.setdefault("_mark_pools", {}).setdefault(marks[rid], [])
            self.n_chunks[rid] = 0
        return voc

    def _chunk(self, rid, voc, out_meta, codes, ev, final: bool) -> None:
        """an event with frames: a job for a launch group, or (synchronous tokenizer) its audio at once"""
        if self.batched:
            inp, first = voc.prepare(codes, ev)
            # exact mode: (new codes, drop, ev, None, stream state, frames before the push) -- the class is (min(F, ctx_max), n_new) and the
            # drop, so every steady-state chunk of every lane falls into one class; a state is pushed once per call, so the k-th chunk an
            # utterance adds in a poll goes into the k-th generation of the class (``StreamGroups.key_of``)
            d = (ExactDecode(inp, first, ev, None, voc.cstream, voc.frames_before) if voc.exact
                 else WindowDecode(inp, first, ev, voc.last_prefix))
            self.groups.add([rid, out_meta, None, d])
        else:
            staged = self.limit is not None or self.lvl is not None or voc.output is not None or voc.mark_spec is not None
            audio, _sr = voc.push(codes, ev, final=final) if staged else voc.push(codes, ev)
            if final and voc.output is not None:
                self.model._give_stage(voc.stage)
            self.groups.add([rid, out_meta, audio, None])
        self.n_chunks[rid] += 1

    def _final_marker(self, rid, voc, out_meta, codes) -> None:
        """a final event without frames: what the utterance's stages held back leaves as its audio"""
        groups, side = self.groups, self.side
        tail = np.zeros(1 if codes is None else 0, dtype=np.float32)
        if self.lvl is not None and voc.level is not None:
            groups.launch_open()                               # the utterance's chunks that still wait end its leveller's stream
            with (contextlib.nullcontext() if side is None else torch.cuda.stream(side)):
                voc.level_release()
        if voc.output is not None:
            # what the output stage (and a limiter in front of it) held back leaves as this event's audio
            groups.launch_open()
            tail, _sr = voc.flush()
            if voc.stage.flac and not voc.header_sent:
                from .audio_out import behind_header
                tail, voc.header_sent = behind_header(voc.stage, tail), True
            self.model._give_stage(voc.stage)
        elif (self.limit is not None and voc.limit is not None) or voc.mark_spec is not None:
            groups.launch_open()                               # the utterance's chunks that still wait go in front of its tail
            held, _sr = voc.flush()
            tail = held if len(held) else tail
        groups.add([rid, out_meta, tail, None])
        self.n_chunks[rid] += 1

    def _hand_out(self):
        """Ends a poll (or a run): what ``StreamGroups.flush`` hands out, stamped, as the entry point's events."""
        events = self.groups.flush()
        if self.group_marks:
            # the whole poll is collected before its first event goes out: with ``device_audio`` nothing is copied, so nothing is
            # waited for; a caller that lands copies (``flush`` hands groups out as they land) would wait for the last of them here
            events = list(events)
            for i, ev in enumerate(events):
                ev[1]["group_end"] = i == len(events) - 1
        for rid, m, audio, _d in events:
            rate = self.model._out_rate(self.outputs, rid)
            if self.stamp is not None:
                self.stamp(rid, m)
            yield rid, audio, rate, m

    # ---- the device work of one launch group --------------------------------------------------------------------------------------
    def launch(self, key, part) -> Landing:
        self._wait_inputs(part)
        with torch.cuda.stream(self.side):
            wav = self._decode(key, part)
            if self.gain is not None:
                from .loudness import apply_gain
                wav = apply_gain(wav.contiguous(), self.gain, self.side)
            finals = [bool(j[1].get("is_final")) for j in part]
            voc_of = [self.vocs[j[0]] for j in part]
            # a poll that completes two chunks of one shape puts an utterance into a part twice; a stage is pushed once per group
            # call, so such a part is cut into consecutive runs in which every utterance appears once (nearly always: one run)
            runs = runs_of(part)
            whole = self._level(voc_of, wav, finals, runs)
            # rows whose length changes lie back to back in device buffers: ``place[k]`` is (offset in the buffers' concatenation, count)
            wav, bufs, place = self._mark(voc_of, whole, finals, runs)
            wav, bufs, place = self._limit(voc_of, wav, bufs, place, finals, runs)
            staged = [k for k, v in enumerate(voc_of) if v.output is not None]
            encoded = self._encode(voc_of, wav, finals, runs, staged)
            return self._land(whole, wav, bufs, place, staged, encoded)

    def _wait_inputs(self, part) -> None:
        side = self.side
        for _rid, _meta, _audio, d in part:
            if d.ready is not None:
                side.wait_event(d.ready)
            else:
                side.wait_stream(torch.cuda.current_stream(torch.device(self.model.device)))

    def _decode(self, key, part):
        """the group's waveforms, one float32 row per job"""
        tok = self.tok
        _T, first, pf_len = key
        ds = [d for _rid, _meta, _audio, d in part]
        if pf_len == "exact":
            # exact mode: the group's stream states take their new frames in one push; `first` = samples in front of an ICL cut's floor
            wav = tok.stream_push([d.state for d in ds], torch.stack([d.codes for d in ds]))[:, first:]
        else:
            pfs = [d.prefix for d in ds] if pf_len > 0 else None   # (phase 1 behind ICL references: the voices' cached front-end states)
            if len(ds) == 1:
                wav = (tok.decode_tensor(ds[0].codes, first, prefix=pfs[0]) if pfs else tok.decode_tensor(ds[0].codes, first)).reshape(1, -1)
            else:
                stacked = torch.stack([d.codes for d in ds])
                wav = tok.decode_tensor_batch(stacked, first, prefixes=pfs) if pfs else tok.decode_tensor_batch(stacked, first)
        return wav.float()

    def _level(self, voc_of, wav, finals, runs):
        if self.lvl is None:
            return wav
        # every utterance's own leveller takes its row and writes a row of the same length: the group stays one tensor,
        # and the rows of a run go through ONE meter launch, ONE target launch and ONE multiply
        from .leveller import push_group as level_group
        rows, wav = wav, torch.empty(wav.shape, dtype=torch.float32, device=wav.device)
        for run in runs:
            level_group([voc_of[k].level_take() for k in run], [rows[k] for k in run], [finals[k] for k in run],
                        outs=[wav[k] for k in run])
            for k in run:
                if finals[k]:
                    voc_of[k].level_release()
        return wav

    def _mark(self, voc_of, whole, finals, runs):
        marked = {k for k, v in enumerate(voc_of) if v.mark_spec is not None}
        if not marked:
            return whole, [], [None] * len(voc_of)
        # every marked utterance's own watermark takes its row, under its own key: ONE launch per run.  A row comes back
        # shorter by the 256 to 511 samples the mark holds back, or longer at the end; rows without a mark pass untouched
        from .watermark import _push_group as mark_group
        return push_runs([[k for k in run if k in marked] for run in runs], whole, finals,
                         lambda k: voc_of[k].mark_take(), lambda k: voc_of[k].mark_release(), mark_group)

    def _limit(self, voc_of, wav, bufs, place, finals, runs):
        if self.limit is None:
            return wav, bufs, place
        # every utterance's own limiter takes its row: the rows come back shorter by what it holds back, or longer at the
        # end.  ONE launch per run; the rows lie back to back in the run's device buffer.  The limiter takes EVERY row, the marked
        # ones out of the mark's buffers, so ``bufs`` and ``place`` start afresh: the mark's placements are superseded
        from .limiter import _push_group as limit_group
        return push_runs(runs, wav, finals, lambda k: voc_of[k].limit_take(), lambda k: voc_of[k].limit_release(), limit_group)

    def _encode(self, voc_of, wav, finals, runs, staged):
        if not staged:
            return None
        # the rows with an output spec: one time-scale launch, one resample + encode launch per design, one pinned copy --
        # per run, as the stages in front: a stage is pushed once per group call
        from .audio_out import GroupCopy
        encoded = []
        for run in runs:
            rows = [k for k in run if k in staged]
            if rows:
                encoded.append((rows, GroupCopy([voc_of[k]._stage() for k in rows], [wav[k] for k in rows], [finals[k] for k in rows])))
        return encoded

    def _land(self, whole, wav, bufs, place, staged, encoded) -> Landing:
        """the copies to pinned memory and the event behind them; which row gets which span is ``stream_groups.landing_plan``"""
        side, n = self.side, len(place)
        host = landed = None
        if bufs:
            # (a mark or the limiter ran.)  The rows without an output spec: ONE pinned buffer behind one copy per run, and ONE event.
            # Without a limiter the rows that have no mark kept their place in the group's tensor: they alone are gathered and follow
            # in one more copy
            host = [None] * n
            if len(staged) < n:
                length, spans = landing_plan(n, int(whole.shape[1]), place, [int(b.numel()) for b in bufs], staged)
                pinned, at = torch.empty(length, dtype=torch.float32, pin_memory=True), 0
                for buf in bufs:
                    pinned[at:at + int(buf.numel())].copy_(buf, non_blocking=True)
                    at += int(buf.numel())
                plain = [k for k, s in enumerate(spans) if s is not None and place[k] is None]
                if plain:
                    pinned[at:].copy_(whole[plain].reshape(-1), non_blocking=True)
                host = [None if s is None else pinned[s[0]:s[0] + s[1]] for s in spans]
            landed = torch.cuda.Event()
            landed.record(side)
        elif not self.device_audio and len(staged) < n:
            host = torch.empty(wav.shape, dtype=wav.dtype, pin_memory=True)
            host.copy_(wav, non_blocking=True)
            landed = torch.cuda.Event()
            landed.record(side)
        elif staged:
            landed = encoded[-1][1].event                      # (one stream: the last run's copy lands last)
        return Landing(host, landed, wav, encoded)

    def collect(self, part, handle: Landing) -> None:
        if handle.landed is None:
            arr = handle.wav                                   # device rows: whoever takes them works on the vocoder stream
        else:
            handle.landed.synchronize()
            host = handle.host
            arr = ([None if h is None else h.numpy() for h in host] if isinstance(host, list) else
                   host.numpy() if host is not None else [None] * len(part))
        for k, j in enumerate(part):
            j[2] = arr[k]
        for rows, copy in handle.encoded or ():
            for k, a in zip(rows, copy.rows()):
                v = self.vocs[part[k][0]]
                if v.stage.flac and not v.header_sent:
                    # a FLAC stream: the utterance's first chunk starts with the stream header (length unknown)
                    from .audio_out import behind_header
                    a, v.header_sent = behind_header(v.stage, a), True
                part[k][2] = a
                if part[k][1].get("is_final"):
                    self.model._give_stage(v.stage)
