"""CPU: the launch-group layer of batch streaming (fq3hip/stream_groups.py) driven by the real scheduler
(fq3hip/batching.py) over the fake lanes of test_batching_cpu.py, with a recording ``launch``.

What is at stake: a launch pushes every member's own leveller, limiter, output stage or codec stream state, so per utterance the
LAUNCHES must come in the order of its chunks -- not only what is handed out.  Lanes that are re-used at staggered frames give one
utterance two chunks of different shapes in a poll in which another utterance has already opened the second one's class; joining
that class launched the later chunk first.  ``ParentOrder`` below is that earlier rule: the named cases must fail on it."""
import math
import random
from types import SimpleNamespace

import pytest
import torch

import fq3hip.batching as Bt
from fq3hip.stream_groups import StreamGroups, runs_of, window_plan
from test_batching_cpu import FakeBatch, FakeLaneEngine, LookAheadBatch, _req

GROUP = 32                       # _SideVocoder.STREAM_GROUP (asserted against the product below)
SPF = 1920                       # samples per frame of the fake tokenizer
CONTEXT = 25                     # StreamingVocoder.CONTEXT_FRAMES
CTX_MAX = 16                     # the fake codec stream's context bound (exact keys)


class Shape:
    """what the key rule reads of a job's codes: ``shape[0]``"""

    def __init__(self, n):
        self.shape = (int(n), 16)


class ParentOrder(StreamGroups):
    """The windowed path's rule before the fix: a chunk joins the class of its shape wherever that class stands in the launch
    order, and a full class launches everything open.  (The exact path had its guard already and goes through the product's rule.)"""

    def add(self, j):
        if j[3] is None or len(j[3]) > 4:
            return super().add(j)
        self.jobs.append(j)
        key = self.key_of(j)
        self.class_seq.setdefault(key, len(self.class_seq))
        self.open_classes.setdefault(key, []).append(j)
        if len(self.open_classes[key]) >= self.group:
            self.launch_open()


class _AdoptEngine(FakeLaneEngine):
    def kv_adopt(self, src, n_rows):
        pass


def make_staged_decoder(monkeypatch, n_lanes, mode):
    """the scheduler as the model builds it: as many spare contexts as lanes, requests prefilled ahead and admitted by hand-over"""
    lanes = [_AdoptEngine([], i) for i in range(n_lanes)]
    spares = [_AdoptEngine([], 100 + i) for i in range(n_lanes)]

    def fake_prefill(eng, tie, tam, config, min_new, temperature, top_k, top_p, do_sample):
        return 7, torch.zeros(8), tie.shape[1], 0

    def fake_arm(talker, config, token, hidden, n_rows, tam, tth, tpe, pg, tg, max_new, min_new, temperature, top_k, top_p, do_sample, rp, use_graph, n_pad=None):
        eng = tg.engine
        cfg = eng.next_cfg
        eng.frames, eng.budget, eng.eos_after, eng.rid = 0, int(max_new), cfg.eos_after, cfg.rid
        return eng, torch.zeros(1), torch.zeros(1), int(max_new)

    monkeypatch.setattr(Bt, "_prefill_first_token", fake_prefill)
    monkeypatch.setattr(Bt, "_prefill_first_tokens_packed", lambda engs, items: [fake_prefill(e, *it) for e, it in zip(engs, items)])
    monkeypatch.setattr(Bt, "_arm_decode", fake_arm)
    monkeypatch.setattr(Bt, "_refill", lambda eng, tn, pn: None)
    monkeypatch.setattr(Bt, "TalkerGraph", lambda e: SimpleNamespace(engine=e))
    monkeypatch.setattr(Bt, "PredictorGraph", lambda e, **kw: SimpleNamespace(engine=e, **kw))
    dec = Bt.BatchDecoder(lanes, poll_every=8, batch_factory=FakeBatch if mode == "sync" else LookAheadBatch, staging=spares, packed_prefill=True)
    orig_admit = dec._admit

    def admit(ln, st):
        ln.engine.next_cfg = st.req.config
        return orig_admit(ln, st)

    dec._admit = admit
    return dec


def make_decoder(monkeypatch, n_lanes, mode, staged=False):
    if staged:
        return make_staged_decoder(monkeypatch, n_lanes, mode)
    engines = [FakeLaneEngine([], i) for i in range(n_lanes)]

    def fake_arm(talker, tie, tam, tth, tpe, config, pg, tg, max_new, min_new, temperature, top_k, top_p, do_sample, rp, use_graph):
        eng = tg.engine
        eng.frames, eng.budget, eng.eos_after, eng.rid = 0, int(max_new), config.eos_after, config.rid
        return eng, torch.zeros(1), torch.zeros(1), int(max_new)

    monkeypatch.setattr(Bt, "_prefill_and_arm", fake_arm)
    monkeypatch.setattr(Bt, "_refill", lambda eng, tn, pn: None)
    monkeypatch.setattr(Bt, "TalkerGraph", lambda e: SimpleNamespace(engine=e))
    monkeypatch.setattr(Bt, "PredictorGraph", lambda e, **kw: SimpleNamespace(engine=e, **kw))
    return Bt.BatchDecoder(engines, poll_every=8, batch_factory=FakeBatch if mode == "sync" else LookAheadBatch)


class Run:
    """One streaming run through the layer, as ``_run_batch_streaming`` drives it: a job per event, a flush at the end of every poll.
    ``keys``: "window" (the product's windowing arithmetic, ``ref_len`` reference frames in front), "exact", or a callable
    ``(rid, k) -> (T, first)`` that names the class of utterance rid's k-th chunk."""

    def __init__(self, dec, reqs, chunk, keys="window", cls=StreamGroups, group=GROUP, ref_len=0):
        self.launches, self.yielded, self.entered, self.polls = [], [], [], 0
        self.group = group
        sg = self.sg = cls(self.launch, self.collect, group, CTX_MAX)
        state, n_chunks = {}, {}
        prefix = SimpleNamespace(ref_len=ref_len) if ref_len else None
        for rid, codes, info in dec.run(reqs, chunk_frames=chunk):
            more = int(dec.more_in_poll)
            final = bool(info.get("is_final"))
            k = n_chunks.setdefault(rid, 0)
            meta = dict(chunk_index=k, is_final=final, seq=len(self.entered), poll=self.polls)
            if codes is not None and codes.shape[0] > 0:
                n_new = int(codes.shape[0])
                st = state.setdefault(rid, dict(n_total=0, prev_len=0, spf=None, frames=ref_len))
                if callable(keys):
                    t, first = keys(rid, k)
                    meta["key"], decode = (t, first, 0), (Shape(t), first, None)
                elif keys == "exact":
                    before, st["frames"] = st["frames"], st["frames"] + n_new
                    drop = 7 if k == 0 and ref_len else 0
                    meta["key"], decode = (min(before, CTX_MAX), n_new, drop), (Shape(n_new), drop, None, None, object(), before)
                else:
                    st["n_total"] += n_new
                    start, n_in, first, st["prev_len"], st["spf"] = window_plan(st["n_total"], n_new, ref_len, st["prev_len"], st["spf"],
                                                                             max(CONTEXT, chunk), CONTEXT, lambda n: SPF * n)
                    pf = prefix if start is None else None
                    meta["key"], decode = (n_in, first, ref_len if pf else 0), (Shape(n_in), first, None, pf)
                job = [rid, meta, None, decode]
            elif final:
                job = [rid, meta, "tail", None]
            else:
                continue
            n_chunks[rid] = k + 1
            self.entered.append(job)
            sg.add(job)
            if more <= 0:
                self.flush()
        self.flush()

    def launch(self, key, part):
        self.launches.append((self.polls, key, list(part)))
        return len(self.launches) - 1

    def collect(self, part, handle):
        assert self.launches[handle][2] == part
        for j in part:
            assert j[2] is None, "a job's audio is filled twice"
            j[2] = ("audio", handle)

    def flush(self):
        self.yielded.extend(self.sg.flush())
        assert self.sg.idle
        self.polls += 1

    # ---- the properties ---------------------------------------------------------------------------------------------------------
    def check_yield_order(self):
        per = {}
        for j in self.yielded:
            per.setdefault(j[0], []).append(j[1])
        for rid, metas in per.items():
            assert [m["chunk_index"] for m in metas] == list(range(len(metas))), (rid, [m["chunk_index"] for m in metas])
            assert [m["is_final"] for m in metas] == [False] * (len(metas) - 1) + [True], (rid, [m["is_final"] for m in metas])

    def check_launch_order(self):
        last = {}
        for _poll, key, part in self.launches:             # launch order, inside a launch the members' order
            for j in part:
                assert j[1]["seq"] > last.get(j[0], -1), f"utterance {j[0]}: chunk {j[1]['chunk_index']} is launched in front of an earlier one"
                last[j[0]] = j[1]["seq"]
            runs = runs_of(part)
            assert [k for run in runs for k in run] == list(range(len(part)))
            for run in runs:
                assert len({part[k][0] for k in run}) == len(run)
            if key[2] == "exact":
                assert len(runs) == 1, "a stream state is pushed twice in one call"

    def check_structure(self):
        assert sorted(j[1]["seq"] for j in self.yielded) == list(range(len(self.entered)))            # every job leaves exactly once
        launched = [j[1]["seq"] for _p, _k, part in self.launches for j in part]
        assert sorted(launched) == [j[1]["seq"] for j in self.entered if j[3] is not None]            # and is launched exactly once
        assert all(j[2] is not None for j in self.yielded)
        assert self.sg.idle and self.sg.stats["launches"] == len(self.launches)
        for poll, key, part in self.launches:
            assert 1 <= len(part) <= self.group
            want = {j[1]["key"] for j in part}
            assert len(want) == 1 and {j[1]["poll"] for j in part} == {poll}
            want = want.pop()
            got = (key[0][1:] + (key[1],)) if key[2] == "exact" else key
            assert got == want, (key, want)

    def check(self):
        self.check_structure()
        self.check_launch_order()
        self.check_yield_order()
        return self

    def launches_per_poll(self):
        """-> {poll: (launches made, sum over the poll's classes of ceil(jobs / group))}"""
        made, jobs = {}, {}
        for poll, key, part in self.launches:
            made[poll] = made.get(poll, 0) + 1
            jobs.setdefault(poll, {}).setdefault(key, 0)
            jobs[poll][key] += len(part)
        return {p: (made[p], sum(math.ceil(n / self.group) for n in jobs[p].values())) for p in made}


NAMED = [((4, 12, 8), 4, "sync"), ((4, 12, 8), 4, "lookahead"), ((8, 32, 24), 12, "lookahead"),
         ((8, 38, 30), 4, "sync"), ((8, 38, 30), 4, "lookahead")]


def test_the_group_size_is_the_products():
    from fq3hip.model import _SideVocoder
    assert _SideVocoder.STREAM_GROUP == GROUP


@pytest.mark.parametrize("budgets,chunk,mode", NAMED)
def test_named_cases_keep_every_utterances_order(monkeypatch, budgets, chunk, mode):
    """three requests on two lanes: the lane that finishes first is re-used at a staggered frame"""
    dec = make_decoder(monkeypatch, 2, mode)
    run = Run(dec, [_req(i, b) for i, b in enumerate(budgets)], chunk).check()
    assert run.sg.stats["order_launches"] > 0                       # the situation arises, and the rule is what resolves it
    dec = make_decoder(monkeypatch, 2, mode)
    Run(dec, [_req(i, b) for i, b in enumerate(budgets)], chunk, keys="exact").check()


@pytest.mark.parametrize("budgets,chunk,mode", NAMED)
def test_named_cases_fail_at_the_earlier_ordering(monkeypatch, budgets, chunk, mode):
    """the checks catch the bug: with the rule as it was, the launch order AND the yield order break at every named case (the
    structure holds: nothing was lost, only swapped)"""
    dec = make_decoder(monkeypatch, 2, mode)
    run = Run(dec, [_req(i, b) for i, b in enumerate(budgets)], chunk, cls=ParentOrder)
    run.check_structure()
    with pytest.raises(AssertionError, match="is launched in front of an earlier one"):
        run.check_launch_order()
    with pytest.raises(AssertionError):
        run.check_yield_order()


def test_is_final_in_front_of_its_chunk_at_the_earlier_ordering(monkeypatch):
    dec = make_decoder(monkeypatch, 2, "sync")
    run = Run(dec, [_req(i, b) for i, b in enumerate((8, 38, 30))], 4, cls=ParentOrder)
    finals = {}
    for j in run.yielded:
        finals.setdefault(j[0], []).append(j[1]["is_final"])
    assert any(True in f[:-1] for f in finals.values())


def _sweep():
    rng = random.Random(20240611)
    cases = []
    for mode in ("sync", "lookahead"):
        for chunk in (4, 12):
            for lanes in (2, 3):
                for _ in range(60):
                    n = rng.randint(3, 5)
                    budgets = [rng.randint(4, 63) for _ in range(n)]
                    eos = [rng.randint(1, b) if rng.random() < 0.25 else 10 ** 9 for b in budgets]
                    cases.append((mode, chunk, lanes, budgets, eos, len(cases) % 2 == 1))
    return cases


@pytest.mark.parametrize("keys,ref_len", [("window", 0), ("window", 9), ("exact", 0), ("exact", 9)])
def test_seeded_sweep_of_staggered_budgets(monkeypatch, keys, ref_len):
    fired = 0
    for mode, chunk, lanes, budgets, eos, staged in _sweep():
        dec = make_decoder(monkeypatch, lanes, mode, staged)
        reqs = [_req(i, b, eos_after=e) for i, (b, e) in enumerate(zip(budgets, eos))]
        try:
            run = Run(dec, reqs, chunk, keys=keys, ref_len=ref_len).check()
        except AssertionError as e:
            raise AssertionError(f"{mode} chunk={chunk} lanes={lanes} staged={staged} budgets={budgets} eos={eos}: {e}") from e
        fired += run.sg.stats["order_launches"] > 0
        got = {}
        for j in run.yielded:
            got[j[0]] = got.get(j[0], 0) + 1
        assert set(got) == set(range(len(budgets)))
    if keys == "window":
        assert fired > 0                                            # the sweep reaches the situation the rule is for


@pytest.mark.parametrize("group", [1, 2, 3, 32])
def test_any_key_assignment_keeps_the_properties(monkeypatch, group):
    """the properties do not lean on the windowing's keys: every chunk gets a class drawn from a small pool, so classes recur within
    an utterance, between utterances, and in any order; small groups make full classes launch in the middle of a poll"""
    rng = random.Random(77 + group)
    fired = 0
    for trial in range(60):
        lanes, n = rng.choice((2, 3, 5)), rng.randint(3, 8)
        table, pool = {}, rng.randint(1, 4)
        keys = lambda rid, k: table.setdefault((rid, k), (rng.randint(1, pool), rng.randint(0, 1)))  # noqa: E731
        dec = make_decoder(monkeypatch, lanes, rng.choice(("sync", "lookahead")))
        reqs = [_req(i, rng.randint(1, 40), eos_after=rng.choice((10 ** 9, rng.randint(1, 40)))) for i in range(n)]
        try:
            run = Run(dec, reqs, rng.choice((1, 2, 4)), keys=keys, group=group).check()
        except AssertionError as e:
            raise AssertionError(f"trial {trial}: {e}") from e
        fired += run.sg.stats["order_launches"]
    assert fired > 0 or group == 1                                  # (a group of one launches every job at once: nothing ever waits)


def test_jobs_fed_directly_exact_generations_and_markers():
    """without a scheduler: an utterance's chunks of one exact class go into successive generations; a class that fills launches
    with the classes in front of it only; markers leave last"""
    made = []
    sg = StreamGroups(lambda key, part: made.append((key, [j[0] for j in part])) or len(made), lambda part, h: [j.__setitem__(2, h) for j in part], 2, CTX_MAX)
    ex = lambda rid, before: [rid, {}, None, (Shape(4), 0, None, None, object(), before)]  # noqa: E731
    for rid in (0, 1, 2):
        sg.add(ex(rid, 40))
        sg.add(ex(rid, 44))
    sg.add([2, {}, "tail", None])
    out = list(sg.flush())
    assert [m for _k, m in made] == [[0, 1], [0, 1], [2], [2]]
    assert [k[0][0] for k, _m in made] == [0, 1, 0, 1] and sg.stats["order_launches"] == 0
    assert [(j[0], j[2]) for j in out] == [(0, 1), (1, 1), (0, 2), (1, 2), (2, 3), (2, 4), (2, "tail")] and sg.idle


@pytest.mark.parametrize("n", [3, 32, 33, 128])
@pytest.mark.parametrize("keys", ["window", "exact"])
def test_lanes_that_start_together_still_share_their_launches(monkeypatch, n, keys):
    """grouping survives the rule: equal budgets on N lanes give, per poll, ceil(jobs of a class / STREAM_GROUP) launches per class --
    not one launch per job, and no part-filled launch in front of a full one"""
    for mode in ("sync", "lookahead"):
        for chunk, budget in ((4, 22), (12, 40), (12, 36)):
            dec = make_decoder(monkeypatch, n, mode)
            run = Run(dec, [_req(i, budget) for i in range(n)], chunk, keys=keys).check()
            per_poll = run.launches_per_poll()
            assert per_poll and all(made == want for made, want in per_poll.values()), (mode, chunk, per_poll)
            assert run.sg.stats["order_launches"] == 0
            assert len(run.launches) < len(run.entered) or n == 1
            chunks = sum(1 for j in run.entered if j[3] is not None)
            assert chunks == n * math.ceil(budget / chunk)


def test_window_plan_is_the_references_windowing():
    """phase 1 re-decodes everything behind the reference until max(25, chunk) frames exist, phase 2 decodes 25 context frames and
    the new chunk: against the arithmetic written out, for chunks of any size"""
    rng = random.Random(3)
    for ref_len in (0, 9):
        for chunk in (1, 4, 12, 30):
            total = prev = 0
            spf = None
            for _ in range(20):
                n_new = rng.randint(1, chunk)
                total += n_new
                got = window_plan(total, n_new, ref_len, prev, spf, max(25, chunk), 25, lambda n: SPF * n + 5)
                if spf is None:
                    n_audio = SPF * (ref_len + total) + 5
                    cut = int(ref_len / (ref_len + total) * n_audio) if ref_len else 0
                    want = (None, ref_len + total, cut + prev, n_audio - cut, (n_audio - cut) / total if total >= max(25, chunk) else None)
                else:
                    ctx = min(25, total - n_new)
                    want = (total - n_new - ctx, ctx + n_new, int(round(ctx * spf)) if ctx else 0, prev, spf)
                assert got == want
                _start, _n_in, _first, prev, spf = got
