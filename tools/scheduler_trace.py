#!/usr/bin/env python3
"""CPU: the call sequence of the continuous-batching scheduler (fq3hip/batching.py) over scripted fake engines and a fake batch
object, recorded scenario by scenario.  The trace holds, in order, every call the scheduler makes on them (frames, polls, text
appends, the graph capture, KV reserve / release / hand-over, cancels, code read-outs), the arm / prefill helper it chose with its
engines and seeds, the noise refills, and every event it yields with ``more_in_poll`` read right after it.  Wall-clock values are
left out; of ``text_stats`` the keys that depend on them (``idle_waits``, ``append_wait_*``) are left out.

    python tools/scheduler_trace.py --write      # tests/golden/scheduler_trace.json
    python tools/scheduler_trace.py              # print the trace

tests/test_batching_trace_cpu.py regenerates the trace and compares it with the file: a refactor of the scheduler leaves it
byte-identical, anything else is a behaviour change."""
import json
import os
import sys
from types import SimpleNamespace
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd"))

import fq3hip.batching as Bt                       # noqa: E402
from fq3hip._lib import FQ3_ENOMEM, Fq3Error       # noqa: E402
from fq3hip.text_stream import TextFeeder          # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scheduler_trace.json")
EOS_ROW = 999
BIG = 10 ** 9


class Pool:
    """64-slot KV blocks shared by the contexts of one scheduler; ``blocks`` = None never runs out."""

    def __init__(self, blocks=None):
        self.free = blocks

    def take(self, n):
        if self.free is not None:
            if n > self.free:
                raise Fq3Error(FQ3_ENOMEM, "KV pool exhausted")
            self.free -= n

    def give(self, n):
        if self.free is not None:
            self.free += n


class Engine:
    """One context of the fake device.  As a lane it applies the hold rule of the frame kernel: a lane whose text table is open and
    whose next row is missing stays where it is and polls 2."""

    def __init__(self, log, idx, max_seq_len=4096):
        self.log, self.idx = log, idx
        self.dtype, self.device = torch.float32, torch.device("cpu")
        self.max_seq_len = max_seq_len
        self.cfg = SimpleNamespace(num_code_groups=16, talker=SimpleNamespace(hidden_size=8, num_hidden_layers=1),
                                   predictor=SimpleNamespace(hidden_size=8, num_hidden_layers=1, vocab_size=32))
        self.emitted, self.budget, self.eos_after, self.rid = 0, 0, BIG, None
        self.rows, self.open, self.cap, self.state = 0, False, 0, 1

    def arm(self, config, max_new):
        self.emitted, self.budget, self.eos_after, self.rid, self.state, self.open = 0, int(max_new), config.eos_after, config.rid, 0, False

    def set_predictor_sampling(self, **kw):
        pass

    def frame(self):
        if self.state == 1:
            return
        if self.emitted >= min(self.budget, self.eos_after):
            self.state = 1
        elif self.open and self.emitted >= self.rows:
            self.state = 2
        else:
            self.state = 0
            self.emitted += 1

    def snapshot(self):
        return self.emitted, (1 if (self.state == 1 or self.emitted >= self.eos_after) else self.state)

    def decode_text_open(self, cap):
        self.log.append(["decode_text_open", self.idx, int(cap)])
        self.rows, self.open, self.cap = 0, True, int(cap)

    def decode_poll_state(self):
        self.log.append(["decode_poll_state", self.idx])
        return self.snapshot()

    def decode_poll(self):
        self.log.append(["decode_poll", self.idx])
        n, st = self.snapshot()
        return n, bool(st)

    def decode_codes(self, first, count):
        self.log.append(["decode_codes", self.idx, int(first), int(count)])
        return torch.full((count, 16), float(self.rid)).long()

    def kv_adopt(self, src, n_rows):
        self.log.append(["kv_adopt", self.idx, src.idx, int(n_rows)])

    @staticmethod
    def noise_fill_many(items, ring_frames=None):
        items[0][0].log.append(["noise_fill_many", [[it[0].idx, it[3], it[4]] for it in items], ring_frames])


class PooledEngine(Engine):
    """A context that draws its KV blocks from a pool and whose device loop can be cancelled."""

    def __init__(self, log, idx, pool, max_seq_len=4096):
        super().__init__(log, idx, max_seq_len)
        self.pool, self.blocks = pool, 0

    def prefill_reserve(self):
        self.log.append(["prefill_reserve", self.idx])

    def kv_reserve(self, n_slots):
        self.log.append(["kv_reserve", self.idx, int(n_slots)])
        want = (int(n_slots) + 63) // 64
        if want > self.blocks:
            self.pool.take(want - self.blocks)
            self.blocks = want

    def kv_release(self, keep=0):
        self.log.append(["kv_release", self.idx])
        self.pool.give(self.blocks)
        self.blocks = 0

    def kv_blocks(self):
        return self.blocks

    def kv_adopt(self, src, n_rows):
        super().kv_adopt(src, n_rows)
        self.pool.give(self.blocks)
        self.blocks, src.blocks = src.blocks, 0

    def decode_cancel(self):
        self.log.append(["decode_cancel", self.idx])
        self.state = 1


class Batch:
    def __init__(self, engines):
        self.engines, self.log = engines, engines[0].log

    def graph_capture(self):
        self.log.append(["graph_capture"])

    def frames(self, n):
        self.log.append(["frames", int(n)])
        for _ in range(n):
            for e in self.engines:
                e.frame()

    def text_append(self, items):
        self.log.append(["text_append", [[lane, list(ids), bool(fin)] for lane, ids, fin in items]])
        for lane, ids, fin in items:
            e = self.engines[lane]
            assert e.open and e.rows + len(ids) <= e.cap, "append to a closed table or past its capacity"
            e.rows += len(ids)
            if fin:
                e.open = False


class LookAheadBatch(Batch):
    """With the batch poll: a snapshot taken in stream order, i.e. when ``poll_async`` is called."""

    def __init__(self, engines):
        super().__init__(engines)
        self.slots = {}

    def poll_async(self, slot):
        assert slot not in self.slots, "a poll slot is re-used before it was read"
        self.log.append(["poll_async", int(slot)])
        self.slots[slot] = [e.snapshot() for e in self.engines]

    def poll_wait_states(self, slot):
        self.log.append(["poll_wait_states", int(slot)])
        snap = self.slots.pop(slot)
        return [n for n, _d in snap], [d for _n, d in snap]

    def poll_wait(self, slot):
        self.log.append(["poll_wait", int(slot)])
        snap = self.slots.pop(slot)
        return [n for n, _d in snap], [bool(d) for _n, d in snap]


BATCHES = {"sync": Batch, "lookahead": LookAheadBatch}


def _seeds(seed):
    return list(seed) if isinstance(seed, (list, tuple)) else seed


def _helpers(log):
    """The module-level names the scheduler looks up at call time, as recording fakes."""
    def prefill_and_arm(talker, tie, tam, tth, tpe, config, pg, tg, max_new, min_new, temperature, top_k, top_p, do_sample, rp,
                        use_graph, cache=None, seed=None):
        eng = tg.engine
        log.append(["prefill_and_arm", eng.idx, config.rid, seed, cache is not None])
        if getattr(config, "bad_arm", False):
            if hasattr(eng, "blocks"):
                eng.pool.take(3)                      # the failing arm took blocks before it raised
                eng.blocks = 3
            raise RuntimeError("Input is too long")
        eng.arm(config, max_new)
        return eng, "tn%d" % eng.idx, "pn%d" % eng.idx, int(max_new)

    def arm_decode(talker, config, token, hidden, n_rows, tam, tth, tpe, pg, tg, max_new, min_new, temperature, top_k, top_p, do_sample,
                   rp, use_graph, n_pad=None, seed=None):
        eng = tg.engine
        log.append(["arm_decode", eng.idx, config.rid, int(token), int(n_rows), n_pad, seed])
        if getattr(config, "bad_arm", False):
            raise RuntimeError("temperature must be positive")
        eng.arm(config, max_new)
        return eng, "tn%d" % eng.idx, "pn%d" % eng.idx, int(max_new)

    def one(eng, tie, tam, config, min_new, temperature, top_k, top_p, do_sample):
        if getattr(config, "bad", False):
            raise RuntimeError("Input is too long")
        return 100 + config.rid, torch.zeros(8), int(tie.shape[1]), 0

    def prefill_first_token(eng, tie, tam, config, min_new, temperature, top_k, top_p, do_sample, cache=None, seed=None):
        log.append(["prefill_first_token", eng.idx, config.rid, seed, cache is not None])
        return one(eng, tie, tam, config, min_new, temperature, top_k, top_p, do_sample)

    def prefill_first_tokens_packed(engs, items, cache=None, seed=None):
        log.append(["prefill_first_tokens_packed", [e.idx for e in engs], [it[2].rid for it in items], _seeds(seed), cache is not None])
        return [one(e, *it) for e, it in zip(engs, items)]     # a packed group fails as a whole

    def prefill_first_tokens_launch(engs, items, cnt, cache=None, seed=None):
        log.append(["prefill_first_tokens_launch", [e.idx for e in engs], [it[2].rid for it in items], list(cnt), _seeds(seed), cache is not None])
        return [one(e, *it) for e, it in zip(engs, items)]

    def refill(eng, tn, pn):
        log.append(["refill", eng.idx, eng.emitted])

    return dict(_prefill_and_arm=prefill_and_arm, _arm_decode=arm_decode, _prefill_first_token=prefill_first_token,
                _prefill_first_tokens_packed=prefill_first_tokens_packed, _prefill_first_tokens_launch=prefill_first_tokens_launch,
                _refill=refill, TalkerGraph=lambda e: SimpleNamespace(engine=e),
                PredictorGraph=lambda e, **kw: SimpleNamespace(engine=e, **kw))


def req(rid, max_new, eos_after=BIG, feeder=None, seed=None, rows=4, **flags):
    cfg = SimpleNamespace(rid=rid, eos_after=eos_after, **flags)
    trailing = torch.zeros(1, 2 if feeder is None else 0, 8)
    return Bt.BatchRequest(rid, None, torch.zeros(1, rows, 8), torch.ones(1, rows), trailing, torch.zeros(1, 1, 8), cfg,
                           dict(max_new_tokens=max_new), text_feeder=feeder, tts_eos_id=None if feeder is None else EOS_ROW, seed=seed)


class Bench:
    """One decoder over fakes and the log all of them write to."""

    def __init__(self, batch="sync", lanes=3, spares=0, pool=False, pool_blocks=None, max_seq_len=4096, **knobs):
        self.log = []
        self._patch = mock.patch.multiple(Bt, **_helpers(self.log))
        self._patch.start()
        if pool:
            p = Pool(pool_blocks)
            mk = lambda i: PooledEngine(self.log, i, p, max_seq_len)
        else:
            mk = lambda i: Engine(self.log, i, max_seq_len)
        self.engines = [mk(i) for i in range(lanes)]
        self.spares = [mk(10 + i) for i in range(spares)]
        prefix_cache = knobs.pop("prefix_cache", None)
        self.dec = Bt.BatchDecoder(self.engines, poll_every=8, batch_factory=BATCHES[batch], staging=self.spares or None,
                                   prefix_cache=prefix_cache)
        self.dec.text_wait_s = 0.001
        for k, v in knobs.items():
            setattr(self.dec, k, v)

    def source(self, late=(), script=None):
        """``source`` for ``run``: at scheduler iteration i performs ``script[i]`` = [(feeder, ids, close), ...] once, then hands out
        the late requests one per call."""
        late, done, dec = list(late), set(), self.dec

        def source():
            it = dec.text_stats["iterations"]
            for k in sorted(script or {}):
                if k <= it and k not in done:
                    done.add(k)
                    for feeder, ids, close in script[k]:
                        if ids:
                            feeder.feed_ids(ids)
                        if close:
                            feeder.close()
            return late.pop(0) if late else None
        return source

    def run(self, requests, stop_after=None, **kw):
        """Drain (or abandon after ``stop_after`` events) one ``run()``; every event goes into the log."""
        self.log.append(["run", sorted(k for k in kw if k != "source")])
        gen = self.dec.run(requests, **kw)
        try:
            for n, (rid, codes, info) in enumerate(gen, 1):
                self.log.append(["event", rid, None if codes is None else int(codes.shape[0]), info.get("is_final"),
                                 info.get("total_steps_so_far"), info.get("steps"), info.get("error"), self.dec.more_in_poll])
                if n == stop_after:
                    gen.close()
                    self.log.append(["abandoned"])
                    return
        except Exception as exc:
            self.log.append(["raised", repr(exc)])
        stats = {k: v for k, v in self.dec.text_stats.items() if k != "idle_waits" and not k.startswith("append_wait_")}
        self.log.append(["text_stats", stats])

    def close(self):
        self._patch.stop()
        return self.log


def _mixed():
    """7 requests with mixed budgets and early EOS; request 2 crosses the 64-frame noise-ring boundary; 5 and 6 arrive late."""
    return ([req(0, 20), req(1, 40, eos_after=13), req(2, 70), req(3, 8), req(4, 16)], [req(5, 33, eos_after=33), req(6, 25, eos_after=5)])


def s_mixed(batch, **kw):
    b = Bench(batch, **kw)
    first, late = _mixed()
    b.run(first, source=b.source(late))
    return b.close()


def s_chunked(batch):
    b = Bench(batch)
    b.run([req(0, 12), req(1, 0), req(2, 10), req(3, 40, eos_after=7), req(4, 8)], chunk_frames=4)
    return b.close()


def s_error_in_packed_group(batch):
    b = Bench(batch, lanes=2, spares=3, pool=True)
    b.run([req(0, 12), req(1, 9, bad=True), req(2, 16), req(3, 8)], on_error="yield", source=b.source([req(4, 8, bad=True), req(5, 8)]))
    return b.close()


def s_error_at_arming(batch, spares):
    b = Bench(batch, lanes=2, spares=spares, pool=True)
    b.run([req(0, 12), req(1, 9, bad_arm=True), req(2, 16)], on_error="yield")
    b.run([req(3, 8), req(4, 9, bad_arm=True)])                       # on_error="raise"
    return b.close()


def s_enomem(batch, first, late, blocks, on_error="raise"):
    """Every request needs 4 + 100 + 1 slots = 2 blocks."""
    b = Bench(batch, lanes=2, spares=3, pool=True, pool_blocks=blocks)
    b.run(first, on_error=on_error, source=b.source(late))
    return b.close()


def s_seeded(batch):
    b = Bench(batch)
    b.run([req(0, 70, seed=100), req(1, 70), req(2, 70, seed=7), req(3, 8, seed=5)])
    return b.close()


def s_staged_seeded_cache(batch):
    b = Bench(batch, lanes=2, spares=3, pool=True, prefix_cache=object())
    b.run([req(0, 20, seed=3), req(1, 12), req(2, 16, seed=2 ** 64 - 1), req(3, 8), req(4, 8)])
    return b.close()


def s_text(batch):
    """Lanes 0 and 1 are text lanes, lane 2 carries whole text.  Feeder 0 pauses before, ON and after the ring boundary and then
    delivers more rows than the table holds (capacity clamp); feeder 1 closes early; the late request 3 is a text lane closed at once."""
    b = Bench(batch)
    f0, f1, f3 = TextFeeder(), TextFeeder(), TextFeeder()
    script = {1: [(f0, list(range(60)), False), (f1, list(range(5)), False)],
              6: [(f1, list(range(3)), True)],
              20: [(f0, list(range(4)), False)],
              26: [(f0, list(range(6)), False)],
              32: [(f0, list(range(100)), True)],
              40: [(f3, list(range(2)), True)]}
    b.run([req(0, 80, feeder=f0), req(1, 30, feeder=f1), req(2, 70)], source=b.source([req(3, 12, feeder=f3)], script))
    return b.close()


def s_abandoned(batch):
    b = Bench(batch, pool=True)
    b.run([req(0, 40), req(1, 24)], chunk_frames=8, stop_after=2)
    b.run([req(2, 20)], chunk_frames=8)
    return b.close()


def scenarios():
    out = {}
    for batch in ("sync", "lookahead"):
        out[f"mixed_{batch}"] = s_mixed(batch)
        out[f"staged_{batch}"] = s_mixed(batch, spares=2, pool=True, first_slice=2)
        out[f"chunked_{batch}"] = s_chunked(batch)
        out[f"text_{batch}"] = s_text(batch)
        out[f"abandoned_{batch}"] = s_abandoned(batch)
    out["staged_first_wave2"] = s_mixed("lookahead", spares=2, pool=True, first_slice=2, first_wave=2)
    out["staged_split_rows"] = s_mixed("lookahead", spares=3, pool=True, max_seq_len=8)        # 4-row prompts: packed groups of two
    out["staged_unpacked"] = s_mixed("lookahead", spares=2, pool=True, packed_prefill=False)
    out["staged_seeded_cache"] = s_staged_seeded_cache("lookahead")
    out["error_in_packed_group"] = s_error_in_packed_group("lookahead")
    out["error_at_arming_direct"] = s_error_at_arming("lookahead", 0)
    out["error_at_arming_staged"] = s_error_at_arming("lookahead", 2)
    # three blocks: the first wave's group fails as a whole with nothing active, then one by one -- request 0 is staged, 1 is postponed
    # behind it and 2 behind 1
    out["enomem_first_wave"] = s_enomem("lookahead", [req(0, 100), req(1, 100), req(2, 100)], [], 3)
    # request 0 decodes; 1 and 2 arrive together and the pool is short for the second of them: both wait, 3 stays behind them
    out["enomem_while_active"] = s_enomem("lookahead", [req(0, 100)], [req(1, 100), req(2, 100), req(3, 100)], 5)
    out["enomem_nothing_active_yield"] = s_enomem("lookahead", [req(0, 100), req(1, 300)], [], 3, on_error="yield")
    out["enomem_nothing_active_raise"] = s_enomem("lookahead", [req(0, 300)], [], 3)
    out["seeded_ring"] = s_seeded("lookahead")
    return out


def render(trace) -> str:
    """One entry per line: a diff of two traces reads as the calls that moved."""
    parts = []
    for name, entries in trace.items():
        lines = ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in entries)
        parts.append(f' {json.dumps(name)}: [\n{lines}\n ]')
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main():
    text = render(scenarios())
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as f:
            f.write(text)
        print(f"wrote {GOLDEN}: {len(text)} bytes")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
