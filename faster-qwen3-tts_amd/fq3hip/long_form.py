"""Long-form synthesis: a text that needs more frames than one context holds is cut into segments, the segments decode side by side
in the lanes of one lock-step batch, and their waveforms are joined ON THE DEVICE into one PCM stream (``fq3_join_*``: leading and
trailing silence removed, a pause of zeros per boundary) in front of the existing output chain.

``split_text``     host: text -> [Segment(text, pause)], deterministic, no language model
``LongFormSpec``   the splitter's budget, the pauses and the join parameters; validates without a GPU
``SegmentJoin``    one output stream's join state on a device
``OrderedJoin``    the ordered hand-over: chunks of later segments wait as device tensors until the earlier segments have ended
``push_group``     the pushes of many ``SegmentJoin``s in one launch and one copy of their lengths
``OrderedJoinSet`` many texts' ordered hand-overs fed by one lock-step run: a round of pushes per group call

The default ``threshold``, ``max_chars`` and pauses are NOT measured on real voices (no checkpoint was available); they are
parameters for that reason."""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib

_ABBREVIATIONS = frozenset(("mr", "mrs", "ms", "dr", "prof", "st", "vs", "etc", "e.g", "i.e"))
_CLOSERS = "\"'”’»)]}」』）】"
_WESTERN = ".!?…"
_CJK = "。！？；"
_CLAUSE_MARKS = ",;:—，、"


class Segment(NamedTuple):
    text: str
    pause: str          # what follows the segment: clause | sentence | paragraph | end


def _dot_is_break(par: str, i: int) -> bool:
    """``par[i] == '.'``: False between digits, after a single capital letter, after a short abbreviation"""
    if 0 < i < len(par) - 1 and par[i - 1].isdigit() and par[i + 1].isdigit():
        return False
    j = i
    while j > 0 and (par[j - 1].isalpha() or par[j - 1] == "."):
        j -= 1
    word = par[j:i]
    if len(word) == 1 and word.isupper():
        return False
    return word.lower() not in _ABBREVIATIONS


def _sentences(par: str) -> List[tuple]:
    """The sentences of one paragraph (whitespace already single spaces, stripped): [(text, glued)], glued: no whitespace stood
    between it and the sentence before (CJK), so a merge puts none there either."""
    out, start, i, n = [], 0, 0, len(par)
    while i < n:
        ch = par[i]
        if ch in _CJK:
            j = i + 1
            while j < n and par[j] in _CLOSERS:
                j += 1
        elif ch in _WESTERN and (ch != "." or _dot_is_break(par, i)):
            j = i + 1
            while j < n and par[j] in _WESTERN:              # "?!", "..."
                j += 1
            while j < n and par[j] in _CLOSERS:
                j += 1
            if j < n and not par[j].isspace():
                i += 1
                continue
        else:
            i += 1
            continue
        piece = par[start:j].strip()
        if piece:
            out.append((piece, start > 0 and not par[start].isspace()))
        start = i = j
    piece = par[start:].strip()
    if piece:
        out.append((piece, start > 0 and not par[start].isspace()))
    return out


def _cut_long(sentence: str, max_chars: int) -> List[str]:
    """A sentence above the budget: cut at the last clause mark inside it, else at whitespace, else hard."""
    out, rest = [], sentence
    while len(rest) > max_chars:
        window = rest[:max_chars]
        cut = max(window.rfind(m) for m in _CLAUSE_MARKS) + 1            # behind the mark; 0: none
        if cut <= 0 or not rest[:cut].strip():
            cut = window.rfind(" ")
            if cut <= 0:
                cut = max_chars
        head = rest[:cut].strip()
        if head:
            out.append(head)
        rest = rest[cut:].strip()
    if rest:
        out.append(rest)
    return out


def split_text(text: str, max_chars: int = 240) -> List[Segment]:
    """Deterministic.  Joining the segments' texts with single spaces reproduces ``text`` up to runs of whitespace; every segment is
    within ``max_chars``.  An empty or whitespace-only text gives []."""
    if not isinstance(text, str):
        raise ValueError("text must be a string")
    if isinstance(max_chars, bool) or not isinstance(max_chars, (int, np.integer)) or max_chars < 1:
        raise ValueError(f"max_chars must be a positive integer, not {max_chars!r}")
    max_chars = int(max_chars)
    segs: List[Segment] = []
    for par in re.split(r"\n[ \t\r\f\v]*(?:\n[ \t\r\f\v]*)+", text.replace("\r\n", "\n").replace("\r", "\n")):
        par = " ".join(par.split())
        if not par:
            continue
        pieces: List[Segment] = []
        for s, glued in _sentences(par):
            if len(s) > max_chars:
                cuts = _cut_long(s, max_chars)
                pieces.extend(Segment(c, "clause") for c in cuts[:-1])
                pieces.append(Segment(cuts[-1], "sentence"))
            elif pieces and pieces[-1].pause == "sentence" and len(pieces[-1].text) + (not glued) + len(s) <= max_chars:
                pieces[-1] = Segment(pieces[-1].text + ("" if glued else " ") + s, "sentence")      # greedy merge inside the budget
            else:
                pieces.append(Segment(s, "sentence"))
        pieces[-1] = Segment(pieces[-1].text, "paragraph")
        segs.extend(pieces)
    if segs:
        segs[-1] = Segment(segs[-1].text, "end")
    return segs


def _default_pauses() -> Dict[str, int]:
    return {"clause": 120, "sentence": 300, "paragraph": 650}


@dataclass(frozen=True)
class LongFormSpec:
    """``max_chars``: the splitter's budget per segment.  ``pause_ms``: the zeros behind a segment by what follows it (at most 5000).
    ``threshold`` / ``lead_hops`` / ``tail_hops`` / ``hold_hops``: the join stage (hops of 10 ms).  Not tuned on real voices."""
    max_chars: int = 240
    pause_ms: Dict[str, int] = field(default_factory=_default_pauses)
    threshold: float = 0.005
    lead_hops: int = 2
    tail_hops: int = 5
    hold_hops: int = 100

    def __post_init__(self):
        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not is_int(self.max_chars) or self.max_chars < 1:
            raise ValueError(f"max_chars must be a positive integer, not {self.max_chars!r}")
        if not isinstance(self.pause_ms, dict) or set(self.pause_ms) != {"clause", "sentence", "paragraph"}:
            raise ValueError("pause_ms must have exactly the keys clause, sentence, paragraph")
        for k, v in self.pause_ms.items():
            if not is_int(v) or not 0 <= v <= 5000:
                raise ValueError(f"pause_ms[{k!r}] must be an integer in [0, 5000], not {v!r}")
        t = self.threshold
        if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not 0.0 < float(t) < 1.0:
            raise ValueError(f"threshold must lie in (0, 1), not {t!r}")
        if not is_int(self.lead_hops) or not 0 <= self.lead_hops <= 16:
            raise ValueError(f"lead_hops must be in [0, 16], not {self.lead_hops!r}")
        if not is_int(self.hold_hops) or not 0 <= self.hold_hops <= 400:
            raise ValueError(f"hold_hops must be in [0, 400], not {self.hold_hops!r}")
        if not is_int(self.tail_hops) or not 0 <= self.tail_hops <= self.hold_hops:
            raise ValueError(f"tail_hops must be in [0, hold_hops], not {self.tail_hops!r}")

    def pause_samples(self, pause: str, in_rate: int) -> int:
        """``end`` -> 0.  The pauses are zeros at the model's rate IN FRONT of the time-scale stage, so they scale with ``speed``."""
        return 0 if pause == "end" else int(self.pause_ms[pause]) * int(in_rate) // 1000

    def join_config(self, in_rate: int) -> "_lib.JoinConfig":
        return _lib.JoinConfig(int(in_rate), float(self.threshold), int(self.lead_hops), int(self.tail_hops), int(self.hold_hops))

    def split(self, text: str) -> List[Segment]:
        return split_text(text, self.max_chars)


def join_bound(in_rate: int, threshold: float, lead_hops: int, tail_hops: int, hold_hops: int, n_in: int, pause_samples: int = 0) -> int:
    """``fq3_join_bound`` (host only, no GPU): ``ValueError`` with the library's reason for a bad configuration or length."""
    lib = _lib.load()
    cfg = _lib.JoinConfig(int(in_rate), float(threshold), int(lead_hops), int(tail_hops), int(hold_hops))
    n = lib.fq3_join_bound(C.byref(cfg), int(n_in), int(pause_samples))
    if n < 0:
        raise ValueError(lib.fq3_last_error().decode("utf-8", "replace"))
    return int(n)


_HEAD = 4           # floats in front of the samples of a push buffer: the int64 length, then padding to 16 bytes


class SegmentJoin:
    """One output stream through the join stage.  ``push(pcm, end, pause_samples)`` takes the next float32 samples of the current
    segment (a device tensor; ``end`` 0: the segment goes on, 1: it ends and ``pause_samples`` zeros follow, 2: it and the stream end)
    and returns the joined samples this push settles as a device tensor.  How many that is depends on the data: ``push`` reads the
    8-byte length (one synchronisation of the stage's stream, as ``AudioOut.push`` does for FLAC); ``push_host`` moves length and
    samples in one transfer.  Work is enqueued on ``stream`` (default: the current stream at the time of the call)."""

    def __init__(self, in_rate: int, device, threshold: float = 0.005, lead_hops: int = 2, tail_hops: int = 5, hold_hops: int = 100,
                 stream=None):
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        if self.dev.type != "cuda":
            raise ValueError("SegmentJoin runs on the GPU; there is no CPU fallback")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.in_rate, self.stream = int(in_rate), stream
        self.cfg = _lib.JoinConfig(self.in_rate, float(threshold), int(lead_hops), int(tail_hops), int(hold_hops))
        self._lib = _lib.load()
        self._h = None
        if self._lib.fq3_join_bound(C.byref(self.cfg), 0, 0) < 0:                      # range errors first, without a HIP call
            raise ValueError(self._lib.fq3_last_error().decode("utf-8", "replace"))
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            _lib.check(self._lib.fq3_join_create(C.byref(self.cfg), C.byref(h)))
        self._h = h
        self.n_in = self.n_out = 0
        self.finished = False
        self._empty = torch.empty(0, dtype=torch.float32, device=self.dev)

    @classmethod
    def from_spec(cls, spec: LongFormSpec, in_rate: int, device, stream=None) -> "SegmentJoin":
        return cls(in_rate, device, spec.threshold, spec.lead_hops, spec.tail_hops, spec.hold_hops, stream)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.fq3_join_destroy(h)

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def bound(self, n_in: int, pause_samples: int = 0) -> int:
        n = self._lib.fq3_join_bound(C.byref(self.cfg), int(n_in), int(pause_samples))
        if n < 0:
            _lib.check(int(n))
        return int(n)

    def reset(self) -> None:
        """A new stream on the same object."""
        _lib.check(self._lib.fq3_join_reset(self._h, C.c_void_p(self._stream().cuda_stream)))
        self.n_in = self.n_out = 0
        self.finished = False

    def push_into(self, pcm: Optional[torch.Tensor], end: int, pause_samples: int, out: torch.Tensor, n_out: torch.Tensor) -> None:
        """The C call itself: ``out`` a contiguous float32 device tensor (a view at any float offset) with room for
        ``bound(n, pause)`` samples, ``n_out`` a device int64 that receives the count.  Raises ``Fq3Error`` with the library's code."""
        s = self._stream()
        with torch.cuda.device(self.dev), torch.cuda.stream(s):
            x = self._empty if pcm is None else pcm.reshape(-1)
            if x.dtype != torch.float32 or x.device != self.dev or not x.is_contiguous():
                x = x.to(device=self.dev, dtype=torch.float32).contiguous()
            if out.dtype != torch.float32 or out.device != self.dev or not out.is_contiguous() or out.dim() != 1:
                raise ValueError("out must be a contiguous 1-D float32 device tensor")
            if n_out.dtype != torch.int64 or n_out.device != self.dev or n_out.numel() < 1:
                raise ValueError("n_out must be a device int64 tensor")
            n = int(x.numel())
            _lib.check(self._lib.fq3_join_push(self._h, C.c_void_p(x.data_ptr() if n else None), n, int(end), int(pause_samples),
                                               C.c_void_p(out.data_ptr() if out.numel() else None), int(out.numel()),
                                               C.c_void_p(n_out.data_ptr()), C.c_void_p(s.cuda_stream)))
            if n:
                x.record_stream(s)
        self.n_in += n
        self.finished = self.finished or int(end) == 2

    def _push_buf(self, pcm, end, pause_samples) -> torch.Tensor:
        """-> device float32 buffer: the int64 length in the first 8 bytes, the samples from float ``_HEAD`` on (16-byte aligned)"""
        n = 0 if pcm is None else int(pcm.numel())
        if n < 0 or n > (1 << 40):
            raise ValueError("push length outside [0, 2^40]")
        with torch.cuda.device(self.dev), torch.cuda.stream(self._stream()):
            cap = n + (self.cfg.hold_hops + self.cfg.lead_hops + 1) * (self.in_rate // 100) + (max(0, int(pause_samples)) if int(end) == 1 else 0)
            buf = torch.empty(_HEAD + cap, dtype=torch.float32, device=self.dev)
            self.push_into(pcm, end, pause_samples, buf[_HEAD:], buf[:2].view(torch.int64))
        return buf

    def push(self, pcm: Optional[torch.Tensor], end: int = 0, pause_samples: int = 0) -> torch.Tensor:
        buf = self._push_buf(pcm, end, pause_samples)
        with torch.cuda.stream(self._stream()):                  # (the copy must queue behind the stage's launch, on ITS stream)
            n = int(buf[:2].view(torch.int64).item())            # the one synchronisation: how many samples this push settled
        self.n_out += n
        return buf[_HEAD: _HEAD + n]

    def push_host(self, pcm: Optional[torch.Tensor], end: int = 0, pause_samples: int = 0) -> np.ndarray:
        """``push`` with the result on the host: the length and the samples cross in one copy (one synchronisation)."""
        buf = self._push_buf(pcm, end, pause_samples)
        with torch.cuda.stream(self._stream()):
            host = buf.cpu().numpy()
        n = int(host[:2].view(np.int64)[0])
        self.n_out += n
        return host[_HEAD: _HEAD + n]


GROUP_MAX = _lib.FQ3_STAGE_GROUP_MAX


def push_group(joins, pcms, ends, pauses) -> list:
    """``[joins[i].push(pcms[i], ends[i], pauses[i]) for i]`` -- the same device tensors, bit for bit, and the same state and counters
    on every object -- with ONE launch of one workgroup per row instead of one launch per row (``fq3_join_push_group``, up to 32 rows
    a call), and ONE synchronisation per call instead of one per row: the rows' lengths lie side by side in one
    device int64 tensor and reach pinned memory in one copy behind one event.  The joins share a device and a stream and appear once;
    they may differ in their configuration.  Every row's room is its ``bound()``; the rows of a call lie in one device buffer, each
    starting on a 16-byte boundary.  A lone row takes its single push.  All or nothing over ANY number of rows: every check the
    library makes per row (an ended stream, ``end``, the length, the pause) is made here for all rows before the first call."""
    joins, pcms, ends, pauses = list(joins), list(pcms), [int(e) for e in ends], [int(p) for p in pauses]
    if not (len(joins) == len(pcms) == len(ends) == len(pauses)):
        raise ValueError("push_group: one pcm, one end and one pause per join")
    if len(set(map(id, joins))) != len(joins):
        raise ValueError("push_group: the same join twice in one call")
    if not joins:
        return []
    if len(joins) == 1:
        return [joins[0].push(pcms[0], ends[0], pauses[0])]
    for j, e in zip(joins, ends):
        # a call takes 32 rows, so what the library would refuse in a later call is refused here, before the first one moves anything:
        # an ended stream gets the library's own answer (FQ3_ESTATE), as ``push`` gives it; lengths and pauses are checked by
        # ``bound()`` below, for every row, in front of the first launch
        if not 0 <= e <= 2:
            raise ValueError("push_group: end must be 0, 1 or 2")
        if j.finished:
            j.push(None, 0, 0)
    lib, dev, s = joins[0]._lib, joins[0].dev, joins[0]._stream()
    for j in joins:
        if j.dev != dev or j._stream().cuda_stream != s.cuda_stream:
            raise ValueError("push_group: the joins of one call share a device and a stream")
    out: list = []
    with torch.cuda.device(dev), torch.cuda.stream(s):
        xs = []
        for j, pcm in zip(joins, pcms):
            x = j._empty if pcm is None else pcm.reshape(-1)
            if x.dtype != torch.float32 or x.device != dev or not x.is_contiguous():
                x = x.to(device=dev, dtype=torch.float32).contiguous()
            xs.append(x)
        for j, p in zip(joins, pauses):
            j.bound(0, p)                                          # (the pause range is checked whatever ``end`` says, as in the C call)
        caps = [j.bound(int(x.numel()), p if e == 1 else 0) for j, x, e, p in zip(joins, xs, ends, pauses)]
        offs, cursor = [], 0
        for cap in caps:
            offs.append(cursor)
            cursor += (cap + 3) // 4 * 4
        buf = torch.empty(cursor, dtype=torch.float32, device=dev)
        lens = torch.empty(len(joins), dtype=torch.int64, device=dev)
        base, lens_base, sp = buf.data_ptr(), lens.data_ptr(), C.c_void_p(s.cuda_stream)
        for a in range(0, len(joins), GROUP_MAX):
            b = min(len(joins), a + GROUP_MAX)
            B = b - a
            _lib.check(lib.fq3_join_push_group(
                (C.c_void_p * B)(*[j._h.value for j in joins[a:b]]), B,
                (C.c_void_p * B)(*[x.data_ptr() if x.numel() else None for x in xs[a:b]]),
                (C.c_int64 * B)(*[int(x.numel()) for x in xs[a:b]]), (C.c_int * B)(*ends[a:b]), (C.c_int64 * B)(*pauses[a:b]),
                (C.c_void_p * B)(*[base + 4 * o for o in offs[a:b]]), (C.c_int64 * B)(*caps[a:b]),
                (C.c_void_p * B)(*[lens_base + 8 * i for i in range(a, b)]), sp))
            for j, x, e in zip(joins[a:b], xs[a:b], ends[a:b]):        # the call was accepted as a whole: these rows have moved
                if x.numel():
                    x.record_stream(s)
                j.n_in += int(x.numel())
                j.finished = j.finished or e == 2
        host = torch.empty(len(joins), dtype=torch.int64, pin_memory=True)
        host.copy_(lens, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record(s)
    landed.synchronize()                                           # the one synchronisation: how many samples every row settled
    for j, o, n in zip(joins, offs, host.tolist()):
        j.n_out += int(n)
        out.append(buf[o: o + int(n)])
    return out


class OrderedJoinSet:
    """``T`` ordered hand-overs (one ``OrderedJoin`` per text, each with its own join, pauses, gains and stages) fed by ONE lock-step
    run.  ``feed_group([(text, segment, pcm, last), ...])`` takes what a vocoder group produced, in any interleaving of texts and
    segments, and returns the pieces ``(text, segment, tensor, stream ended)`` that became ready.  Per text the rule is
    ``OrderedJoin.feed``'s: chunks of segment ``k + 1`` wait until ``k`` has ended, and a text's pieces come strictly in text order.
    Consecutive ready chunks of one segment go out as ONE push (the join does not depend on how a segment is cut into pushes); round
    ``r`` then takes the r-th ready push of every text through ONE ``push_group`` and, behind it, through the group call of every
    stage the texts have: the gains, ``leveller.push_group``, ``limiter.push_group``, ``audio_out.push_group``.  A join appears at
    most once per round.  ``push_group`` (internal, tests): what joins a round's rows."""

    def __init__(self, ordered: List["OrderedJoin"], push_group=None):
        self.ordered = list(ordered)
        if len(set(id(o.join) for o in self.ordered)) != len(self.ordered):
            raise ValueError("OrderedJoinSet: every text has its own join")
        self._push_group = push_group
        self.rounds = 0                                            # group calls made so far (diagnostics)

    def _ready(self, oj: "OrderedJoin") -> list:
        """what ``OrderedJoin.feed`` would push now: [(segment, pcm or None, last)], the ready chunks of a segment as one push"""
        pushes = []
        while oj.cur < oj.n and oj._wait[oj.cur]:
            q, oj._wait[oj.cur] = oj._wait[oj.cur], []
            chunks = [pcm.reshape(-1) for pcm, _last in q if pcm is not None and pcm.numel()]
            pcm = None if not chunks else chunks[0] if len(chunks) == 1 else torch.cat(chunks)
            done = q[-1][1]
            pushes.append((oj.cur, pcm, done))
            if not done:
                break
            oj.cur += 1
        return pushes

    def feed_group(self, items) -> list:
        items = list(items)
        for t, k, _pcm, _last in items:                            # every error before any text moves
            if not 0 <= t < len(self.ordered):
                raise ValueError(f"text {t} is not one of the {len(self.ordered)} texts")
            oj = self.ordered[t]
            if not 0 <= k < oj.n or k < oj.cur:
                raise ValueError(f"text {t}: segment {k} is not open (current segment {oj.cur} of {oj.n})")
        ended = {(t, k) for t, oj in enumerate(self.ordered) for k, w in enumerate(oj._wait) if any(last for _pcm, last in w)}
        for t, k, _pcm, last in items:
            if (t, k) in ended:
                raise ValueError(f"text {t}: segment {k} was fed after its last chunk")
            if last:
                ended.add((t, k))
        for t, k, pcm, last in items:
            self.ordered[t]._wait[k].append((pcm, bool(last)))
        ready = [(t, self._ready(oj)) for t, oj in enumerate(self.ordered)]
        for oj in self.ordered:
            oj.max_waiting = max(oj.max_waiting, sum(len(w) for w in oj._wait))
        out = []
        for r in range(max((len(p) for _t, p in ready), default=0)):
            out.extend(self._round([(t, p[r]) for t, p in ready if len(p) > r]))
        return out

    def _round(self, rows) -> list:
        """one push of each of ``rows``' texts -- [(text, (segment, pcm, last))] -- through the join and the stages, group by group"""
        ojs = [self.ordered[t] for t, _p in rows]
        ends = [0 if not last else (2 if k == oj.n - 1 else 1) for oj, (_t, (k, _pcm, last)) in zip(ojs, rows)]
        join = self._push_group if self._push_group is not None else push_group
        ys = join([oj.join for oj in ojs], [p[1] for _t, p in rows], ends,
                  [oj.pauses[p[0]] if e == 1 else 0 for oj, (_t, p), e in zip(ojs, rows, ends)])
        self.rounds += 1
        finals = [e == 2 for e in ends]
        for i, (oj, (_t, (k, _pcm, _last))) in enumerate(zip(ojs, rows)):
            g = oj.gains[k] if isinstance(oj.gains, (list, tuple)) else oj.gains
            if g is not None:
                from .loudness import apply_gain
                ys[i] = apply_gain(ys[i].contiguous(), g, oj.join.stream)

        def through(stage_of, group):
            at = [i for i, oj in enumerate(ojs) if stage_of(oj) is not None]
            if at:
                got = group([stage_of(ojs[i]) for i in at], [ys[i].contiguous() for i in at], [finals[i] for i in at])
                for i, y in zip(at, got):
                    ys[i] = y
        if any(oj.leveller is not None for oj in ojs):
            from .leveller import push_group as level_group
            through(lambda oj: oj.leveller, level_group)
        if any(oj.limiter is not None for oj in ojs):
            from .limiter import push_group as limit_group
            through(lambda oj: oj.limiter, limit_group)
        if any(oj.audio_out is not None for oj in ojs):
            from .audio_out import push_group as out_group
            through(lambda oj: oj.audio_out, out_group)
        return [(t, k, y, e == 2) for (t, (k, _pcm, _last)), y, e in zip(rows, ys, ends)]

    @property
    def finished(self) -> bool:
        return all(oj.finished for oj in self.ordered)


class OrderedJoin:
    """The ordered hand-over between a batch of segments and ONE output stream.  ``feed(k, pcm, last)`` takes the next device chunk of
    segment ``k`` (``last``: the segment ends with it); segments may be fed in any interleaving.  Chunks of segment ``k + 1`` wait as
    device tensors until segment ``k`` has ended; what ``feed`` returns is the list of ``(segment_index, joined device tensor, stream
    ended)`` pieces that became ready, strictly in text order.  With ``audio_out`` (an ``AudioOut``) the joined samples go through that
    chain (join -> time-scale -> resample / encode -> FLAC, one stream) and the pieces are its output.  ``gains`` (None; a 1-element
    float32 device tensor; or a list of them, one per segment): what segment ``k`` contributes -- its samples and the pause behind
    them -- leaves the join multiplied by ``gains`` / ``gains[k]`` (``fq3_loud_apply``).  ``limiter`` (None, or a ``Limiter``): the
    joined and scaled stream goes through it in front of the chain.  ``leveller`` (None, or a ``Leveller``): in front of the limiter."""

    def __init__(self, join: SegmentJoin, pauses: List[int], audio_out=None):
        self.join, self.pauses, self.audio_out = join, [int(p) for p in pauses], audio_out
        self.gains = None                                          # a 1-element device tensor, or one per segment: see ``_emit``
        self.limiter = None                                        # a ``Limiter`` on the join's stream: the joined stream goes through it
        self.leveller = None                                       # a ``Leveller`` likewise, in front of the limiter
        self.n = len(self.pauses)
        self.cur = 0
        self._wait: List[List] = [[] for _ in range(self.n)]        # per segment: [(device tensor or None, last)]
        self.max_waiting = 0                                       # most chunks that waited at once (diagnostics)

    def _emit(self, k, pcm, last):
        end = 0 if not last else (2 if k == self.n - 1 else 1)
        y = self.join.push(pcm, end, self.pauses[k] if end == 1 else 0)
        g = self.gains[k] if isinstance(self.gains, (list, tuple)) else self.gains
        if g is not None:
            # level behind the join, in front of the chain: the join's silence decisions saw the raw samples, pause zeros stay zeros
            from .loudness import apply_gain
            y = apply_gain(y.contiguous(), g, self.join.stream)
        if self.leveller is not None:
            # the streaming loudness leveller: behind the gains, in front of the limiter; it holds nothing back
            y = self.leveller.push(y.contiguous(), final=end == 2)
        if self.limiter is not None:
            # behind the gains, in front of the chain: one stream, so the look-ahead is held back once and comes out at the end
            y = self.limiter.push(y.contiguous(), final=end == 2)
        if self.audio_out is not None:
            y = self.audio_out.push(y, final=end == 2)
        return (k, y, end == 2)

    def feed(self, k: int, pcm: Optional[torch.Tensor], last: bool):
        if not 0 <= k < self.n or k < self.cur:
            raise ValueError(f"segment {k} is not open (current segment {self.cur} of {self.n})")
        self._wait[k].append((pcm, bool(last)))
        out = []
        while self.cur < self.n and self._wait[self.cur]:
            q, self._wait[self.cur] = self._wait[self.cur], []
            done = False
            for pcm_k, last_k in q:
                if done:
                    raise ValueError(f"segment {self.cur} was fed after its last chunk")
                out.append(self._emit(self.cur, pcm_k, last_k))
                done = last_k
            if not done:
                break
            self.cur += 1
        self.max_waiting = max(self.max_waiting, sum(len(w) for w in self._wait))
        return out

    @property
    def finished(self) -> bool:
        return self.cur >= self.n
