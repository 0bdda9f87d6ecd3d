"""The launch-group layer of batch streaming (``FasterQwen3TTS._run_batch_streaming``), host bookkeeping only: which chunks of one
poll of the lock-step decode go through ONE batched vocoder launch set, in which order the launch sets are made, and in which order
their chunks are handed out.  The device work comes in as two callables, so the layer runs -- and is tested -- without a GPU
(``tests/test_stream_groups_cpu.py``).

A job is the list ``[rid, meta, audio | None, decode | None]``:

* ``decode`` of the windowed path: ``(codes_in, first_sample, ready_event[, prefix])`` -- what ``StreamingVocoder.prepare`` returned;
* ``decode`` of the exact path: ``(new_codes, drop, ready_event, None, stream_state, frames_before)``;
* ``decode = None``: an event that needs no launch (its ``audio`` is already there).  Per utterance only its LAST event may be one
  (the final marker), unless no job at all has a decode (a synchronous tokenizer: everything leaves in the order it came).

Order.  Jobs that need the same decode shape share a class; classes are launched in order of first
appearance, ``group`` jobs at a time, and a launch also pushes every member's own leveller, limiter, output stage or codec stream
state.  So per utterance LAUNCH order is state order, and the layer keeps it equal to the order the jobs came in:

* a job never joins a class that would launch in front of a still-waiting earlier job of the same utterance: the classes up to that
  job's are launched first (``stats["order_launches"]`` counts how often) and the job opens or joins a class behind them;
* a class that is full is launched at once, together with the classes opened before it, never the ones behind it;
* inside a class the members keep their order of arrival; an utterance that is in a class twice (windowed path: two chunks of one
  shape in one poll) is cut into ``runs`` by the launch, an exact-path class never holds an utterance twice (the k-th chunk an
  utterance adds in a poll goes into the k-th generation of its class: a stream state is pushed once per call).

Groups are handed out in launch order, markers without a decode last."""
from typing import Any, Callable, Dict, List, Optional


def window_plan(n_total: int, n_new: int, ref_len: int, prev_len: int, spf: Optional[float], min_cal: int, context: int,
                num_samples_total: Callable[[int], int]):
    """The arithmetic of one step of the reference's streaming windowing (``StreamingVocoder.prepare``), no tensors involved.
    ``n_total`` frames exist, the last ``n_new`` of them are new; ``prev_len`` / ``spf``: the state before the step (``spf`` None:
    phase 1).  Returns ``(start, n_in, first, prev_len, spf)``: the decode takes ``n_in`` frames and its ``waveform[first:]`` is the
    chunk's audio; ``start`` is None in phase 1 (the decode takes the ``ref_len`` reference frames and every frame so far), in phase 2
    the first frame of the window; ``prev_len`` / ``spf``: the state after the step."""
    if spf is None:
        n_in = ref_len + n_total
        n_audio = num_samples_total(n_in)
        cut = int(ref_len / max(n_in, 1) * n_audio) if ref_len else 0
        first = cut + prev_len
        prev_len = n_audio - cut
        return None, n_in, first, prev_len, (prev_len / n_total if n_total >= min_cal else None)
    start = max(0, n_total - n_new - context)
    n_in = n_total - start
    n_ctx = n_in - n_new
    return start, n_in, (int(round(n_ctx * spf)) if n_ctx > 0 else 0), prev_len, spf


def runs_of(part: list) -> List[List[int]]:
    """The indices of ``part`` cut into consecutive runs in which every utterance appears once (nearly always: one run).  A stage is
    pushed once per group call, and a poll that completes two chunks of one shape puts an utterance into a part twice."""
    runs, seen = [[]], set()
    for k, j in enumerate(part):
        if j[0] in seen:
            runs.append([])
            seen = set()
        seen.add(j[0])
        runs[-1].append(k)
    return runs


class StreamGroups:
    """``launch(key, part) -> handle`` makes one launch set for the jobs ``part`` (all of class ``key``, at most ``group`` of them) and
    returns at once; ``collect(part, handle)`` waits for it and fills the jobs' audio (``j[2]``).  ``ctx_max``: the codec stream's
    context bound (exact path: the class of a chunk is ``(min(frames_before, ctx_max), n_new)``)."""

    def __init__(self, launch: Callable[[Any, list], Any], collect: Callable[[list, Any], None], group: int, ctx_max: Optional[int] = None):
        self._launch, self._collect = launch, collect
        self.group, self.ctx_max = max(1, int(group)), ctx_max
        self.jobs: list = []                      # the events of one poll, in order
        self.open_classes: Dict[Any, list] = {}   # class -> its waiting jobs; insertion order = order of first appearance = launch order
        self.class_seq: Dict[Any, int] = {}       # open class -> its place in that order (never reused)
        self.waiting: Dict[Any, List[int]] = {}   # utterance -> the places of the classes its waiting jobs are in (ascending)
        self.added: Dict[Any, int] = {}           # (exact path) utterance -> chunks it added since the last flush
        self.queued: list = []                    # (part, handle) of the launches made, in launch order
        self._next = 0
        self.stats = dict(jobs=0, launches=0, order_launches=0)

    def key_of(self, j, generation: int = 0):
        """The class of a job: jobs of one class go through one batched decode."""
        d = j[3]
        if len(d) > 4:
            return ((generation, min(int(d[5]), self.ctx_max), int(d[0].shape[0])), int(d[1]), "exact")
        pf = d[3] if len(d) > 3 else None
        return (int(d[0].shape[0]), int(d[1]), pf.ref_len if pf is not None else 0)

    def add(self, j) -> None:
        self.jobs.append(j)
        self.stats["jobs"] += 1
        if j[3] is None:
            return
        rid, generation = j[0], 0
        if len(j[3]) > 4:
            generation = self.added.get(rid, 0)
            self.added[rid] = generation + 1
        key = self.key_of(j, generation)
        mine = self.waiting.get(rid)
        if mine and self.class_seq.get(key, self._next) < mine[-1]:
            # the class would launch in front of an earlier chunk of this utterance: that chunk's class and those before it go first
            self.stats["order_launches"] += 1
            self.launch_open(mine[-1])
        seq = self.class_seq.get(key)
        if seq is None:
            seq = self.class_seq[key] = self._next
            self._next += 1
        self.open_classes.setdefault(key, []).append(j)
        self.waiting.setdefault(rid, []).append(seq)
        if len(self.open_classes[key]) >= self.group:
            self.launch_open(seq)

    def launch_open(self, upto: Optional[int] = None) -> None:
        """Launches the open classes in order of first appearance: all of them, or those up to place ``upto``."""
        for key in [k for k in self.open_classes if upto is None or self.class_seq[k] <= upto]:
            members = self.open_classes.pop(key)
            del self.class_seq[key]
            for i in range(0, len(members), self.group):
                part = members[i:i + self.group]
                self.queued.append((part, self._launch(key, part)))
                self.stats["launches"] += 1
        if upto is None:
            self.waiting.clear()
        else:
            for rid in [r for r, seqs in self.waiting.items() if seqs[0] <= upto]:
                left = [s for s in self.waiting[rid] if s > upto]
                if left:
                    self.waiting[rid] = left
                else:
                    del self.waiting[rid]

    def flush(self):
        """Ends a poll: launches what is open and hands the poll's jobs out -- the groups in launch order, each as its audio has
        landed, then the markers without a decode."""
        self.launch_open()
        self.added.clear()
        plain = [j for j in self.jobs if j[3] is None]
        self.jobs = []
        groups, self.queued = self.queued, []
        for part, handle in groups:
            self._collect(part, handle)
            yield from part
        yield from plain

    @property
    def idle(self) -> bool:
        """nothing waits: no job, no open class, no launch that was not handed out"""
        return not (self.jobs or self.open_classes or self.class_seq or self.waiting or self.queued)
