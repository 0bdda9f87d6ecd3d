"""CPU: incremental text in the lock-step scheduler (fq3hip/batching.py) against a fake device that applies the hold rule of
``frame_begin_body`` -- a lane whose text table is open and whose next row is missing stays where it is and polls 2 -- plus the
C ABI of ``fq3_batch_text_append`` as far as it can be seen without a device.

The feeders are driven by scripts keyed to the scheduler's iteration counter (``BatchDecoder.text_stats["iterations"]``), read from
the ``source`` callback, so nothing here depends on the wall clock except the idle rule, which is given a timeout of its own."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import fq3hip.batching as Bt
from fq3hip.text_stream import TextFeeder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS_ROW = 999


class HoldEngine:
    """One lane of the fake device: ``emitted`` frames, a text table of ``rows`` rows that may be ``open``."""

    def __init__(self, idx):
        self.idx = idx
        self.dtype, self.device = torch.float32, torch.device("cpu")
        self.max_seq_len = 4096
        self.cfg = SimpleNamespace(num_code_groups=16, talker=SimpleNamespace(hidden_size=8, num_hidden_layers=1),
                                   predictor=SimpleNamespace(hidden_size=8, num_hidden_layers=1, vocab_size=32))
        self.emitted, self.budget, self.eos_after, self.rid = 0, 0, 10 ** 9, None
        self.rows, self.open, self.cap, self.state, self.ids = 0, False, 0, 1, []
        self.held_frames = 0

    def set_predictor_sampling(self, **kw):
        pass

    def frame(self):
        if self.state == 1:
            return
        if self.emitted >= min(self.budget, self.eos_after):
            self.state = 1
        elif self.open and self.emitted >= self.rows:
            self.state = 2
            self.held_frames += 1
        else:
            self.state = 0
            self.emitted += 1

    def decode_text_open(self, cap):
        self.rows, self.open, self.cap, self.ids = 0, True, int(cap), []

    def decode_poll_state(self):
        st = 1 if (self.state == 1 or self.emitted >= self.eos_after) else self.state
        return self.emitted, st

    def decode_poll(self):
        n, st = self.decode_poll_state()
        return n, bool(st)

    def decode_codes(self, start, count):
        return torch.full((count, 16), float(self.rid)).long()


class HoldBatch:
    def __init__(self, engines):
        self.engines, self.calls, self.captured, self.appends = engines, [], 0, []

    def graph_capture(self):
        self.captured += 1

    def frames(self, n):
        self.calls.append(("frames", n))
        for _ in range(n):
            for e in self.engines:
                e.frame()

    def text_append(self, items):
        assert len({l for l, _i, _f in items}) == len(items)
        self.appends.append([(l, list(ids), f) for l, ids, f in items])
        for l, ids, f in items:
            e = self.engines[l]
            assert e.open and e.rows + len(ids) <= e.cap, "append to a closed table or past its capacity"
            e.rows += len(ids)
            e.ids += list(ids)
            if f:
                e.open = False


class HoldLookAhead(HoldBatch):
    def __init__(self, engines):
        super().__init__(engines)
        self.slots = {}

    def poll_async(self, slot):
        assert slot not in self.slots
        self.slots[slot] = [e.decode_poll_state() for e in self.engines]

    def poll_wait_states(self, slot):
        snap = self.slots.pop(slot)
        return [n for n, _d in snap], [d for _n, d in snap]

    def poll_wait(self, slot):
        n, d = self.poll_wait_states(slot)
        return n, [bool(x) for x in d]


class IgnoresHold(HoldLookAhead):
    """A device that does not hold: it emits a frame although the row is missing."""

    def frames(self, n):
        self.calls.append(("frames", n))
        for _ in range(n):
            for e in self.engines:
                if e.state != 1 and e.emitted < e.budget:
                    e.emitted += 1


def _sched(monkeypatch, mod, factory, n_lanes=3):
    engines = [HoldEngine(i) for i in range(n_lanes)]
    refills = []

    def fake_arm(talker, tie, tam, tth, tpe, config, pg, tg, max_new, min_new, temperature, top_k, top_p, do_sample, rp, use_graph):
        eng = tg.engine
        eng.emitted, eng.budget, eng.eos_after, eng.rid, eng.state, eng.open = 0, int(max_new), config.eos_after, config.rid, 0, False
        return eng, torch.zeros(1), torch.zeros(1), int(max_new)

    monkeypatch.setattr(mod, "_prefill_and_arm", fake_arm)
    monkeypatch.setattr(mod, "_refill", lambda eng, tn, pn: (refills.append((eng.idx, eng.emitted)), factory_calls(eng).append(("refill", eng.idx))))
    monkeypatch.setattr(mod, "TalkerGraph", lambda e: SimpleNamespace(engine=e))
    monkeypatch.setattr(mod, "PredictorGraph", lambda e, **kw: SimpleNamespace(engine=e, **kw))
    dec = mod.BatchDecoder(engines, poll_every=8, batch_factory=factory)

    def factory_calls(_eng):
        return dec.batch.calls
    return dec, engines, refills


def _req(rid, max_new, feeder=None, eos_after=10 ** 9):
    cfg = SimpleNamespace(rid=rid, eos_after=eos_after)
    if feeder is None:
        return Bt.BatchRequest(rid, None, torch.zeros(1, 4, 8), torch.ones(1, 4), torch.zeros(1, 2, 8), torch.zeros(1, 1, 8), cfg,
                               dict(max_new_tokens=max_new))
    return Bt.BatchRequest(rid, None, torch.zeros(1, 4, 8), torch.ones(1, 4), torch.zeros(1, 0, 8), torch.zeros(1, 1, 8), cfg,
                           dict(max_new_tokens=max_new), text_feeder=feeder, tts_eos_id=EOS_ROW)


def _scripted(dec, script):
    """``source`` for ``run``: at scheduler iteration i performs ``script[i]`` = [(feeder, ids, close), ...] once, yields no request."""
    done = set()

    def source():
        it = dec.text_stats["iterations"]
        for k in sorted(script):
            if k <= it and k not in done:
                done.add(k)
                for feeder, ids, close in script[k]:
                    if ids:
                        feeder.feed_ids(ids)
                    if close:
                        feeder.close()
        return None
    return source


@pytest.mark.parametrize("factory", [HoldBatch, HoldLookAhead])
def test_emitted_frame_model_and_refills(monkeypatch, factory):
    """Two text lanes and one whole-text lane, 150 frames each.  Lane 0's text pauses before, ON and after the ring boundary at 64
    (rows stop at 60, 64, 70); lane 1 is fed generously.  Every poll agrees with the model (the scheduler raises otherwise), a held
    lane is never finished, and every lane refills exactly at ITS emitted frames 0, 64, 128 -- the fake records the lane's emitted
    count at the refill, which is the boundary only if no frame in front of the refill is still to come."""
    dec, engines, refills = _sched(monkeypatch, Bt, factory)
    dec.text_wait_s = 0.001
    f0, f1 = TextFeeder(), TextFeeder()
    script = {1: [(f0, list(range(60)), False), (f1, list(range(200)), True)],
              30: [(f0, list(range(4)), False)],          # rows 64: held ON the boundary
              45: [(f0, list(range(6)), False)],          # rows 70
              60: [(f0, list(range(100)), True)]}
    out = {rid: codes for rid, codes, _t in dec.run([_req(0, 150, f0), _req(1, 150, f1), _req(2, 150)], source=_scripted(dec, script))}
    assert {r: c.shape[0] for r, c in out.items()} == {0: 150, 1: 150, 2: 150}
    for lane in range(3):
        assert [r for r in refills if r[0] == lane] == [(lane, 0), (lane, 64), (lane, 128)]
    assert engines[0].held_frames > 0                      # lane 0 really held while the others ran ...
    if factory is HoldLookAhead:
        assert dec.text_stats["polls_held"] > 0 and dec.text_stats["polls_mixed"] > 0
    # the capacity clamp of TextSession._append: max_frames + 1 = 151 rows are all the loop can read, the table closes there
    assert not engines[0].open and not engines[1].open
    assert engines[0].ids == list(range(60)) + list(range(4)) + list(range(6)) + list(range(81)) and engines[1].ids == list(range(151))
    assert all(len(a) >= 1 for a in dec.batch.appends) and dec.text_stats["appends"] == len(dec.batch.appends)


def test_no_frames_while_every_lane_waits(monkeypatch):
    """All active lanes starved from iteration 3 to iteration 40: the scheduler queues nothing meanwhile (it sleeps on the feeders'
    wake-up event) and goes on to the same lengths."""
    dec, engines, refills = _sched(monkeypatch, Bt, HoldLookAhead, n_lanes=2)
    dec.text_wait_s = 0.001
    f0, f1 = TextFeeder(), TextFeeder()
    script = {1: [(f0, list(range(10)), False), (f1, list(range(16)), False)],
              40: [(f0, list(range(50)), True), (f1, list(range(50)), True)]}
    out = {rid: codes for rid, codes, _t in dec.run([_req(0, 40, f0), _req(1, 40, f1)], source=_scripted(dec, script))}
    assert {r: c.shape[0] for r, c in out.items()} == {0: 40, 1: 40}
    n_frames = [c for c in dec.batch.calls if c[0] == "frames"]
    # 16 rows at poll_every 8 are two calls, the remaining 24..30 frames (+ the call that finds the frame limit) at most five more
    assert len(n_frames) <= 2 + 5, n_frames
    assert dec.text_stats["idle_waits"] >= 30
    assert engines[0].held_frames <= 8 and engines[1].held_frames == 0        # lane 0 held only inside the batch that ran lane 1 to row 16


def test_idle_timeout_closes_a_silent_feeder(monkeypatch):
    dec, engines, refills = _sched(monkeypatch, Bt, HoldLookAhead, n_lanes=2)
    dec.text_wait_s, dec.text_idle_timeout_s = 0.005, 0.05
    f0 = TextFeeder()
    f0.feed_ids([1, 2, 3])
    out = list(dec.run([_req(0, 20, f0)]))
    # the utterance ends the way whole text does: tts_eos after the last row, pad rows behind it, the frame limit
    assert out[0][0] == 0 and out[0][1].shape[0] == 20
    assert f0.closed and dec.text_stats["idle_closed"] == 1 and engines[0].ids == [1, 2, 3, EOS_ROW]
    assert all(ln.req is None and ln.text is None for ln in dec.lanes)          # the lane came back


def test_a_poll_that_disagrees_with_the_model_raises(monkeypatch):
    dec, engines, refills = _sched(monkeypatch, Bt, IgnoresHold, n_lanes=2)
    dec.text_wait_s = 0.001
    f0 = TextFeeder()
    f0.feed_ids([1, 2, 3])
    with pytest.raises(RuntimeError, match="hold rule"):
        list(dec.run([_req(0, 40, f0), _req(1, 40)]))


# the call sequence of a whole-text-only run, recorded from the fake with the scheduler as it was before text lanes existed
_F8 = ("frames", 8)
_HEAD = [("refill", 0), ("refill", 1), ("refill", 2)] + [_F8] * 8 + [("refill", 0), ("refill", 1), ("refill", 2), ("frames", 6), ("refill", 1), _F8, _F8]
_TAIL = [_F8] * 4 + [("frames", 4), ("refill", 0), _F8, _F8, ("frames", 6)]
WHOLE_TEXT_CALLS = {
    "sync": _HEAD + [("frames", 6)] + _TAIL,
    "lookahead": _HEAD + [("frames", 4), ("frames", 2)] + _TAIL,
}


def _whole_text_calls(monkeypatch, mod, factory):
    dec, engines, refills = _sched(monkeypatch, mod, factory)
    out = {rid: codes.shape[0] for rid, codes, _t in dec.run([_req(0, 150), _req(1, 70), _req(2, 92), _req(3, 20, eos_after=13)])}
    assert out == {0: 150, 1: 70, 2: 92, 3: 13}
    return list(dec.batch.calls)


@pytest.mark.parametrize("kind,factory", [("sync", HoldBatch), ("lookahead", HoldLookAhead)])
def test_whole_text_runs_make_the_same_calls_as_before(monkeypatch, kind, factory):
    """Four whole-text requests over three lanes (lane reuse, an early EOS, two ring boundaries): the ``_refill`` / ``frames`` calls,
    in order, are those of the scheduler before it knew text lanes."""
    assert _whole_text_calls(monkeypatch, Bt, factory) == WHOLE_TEXT_CALLS[kind]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_entry_point():
    from fq3hip import _lib
    lib_path = os.path.join(ROOT, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fq3hip.h")).read(), flags=re.S)
    assert re.search(r"\bfq3_batch_text_append\s*\(", hdr)
    assert hasattr(lib, "fq3_batch_text_append") and "fq3_batch_text_append" in _lib.SIGNATURES
    lib.fq3_abi_version.restype = ctypes.c_int
    assert lib.fq3_abi_version() == 5
    fn = lib.fq3_batch_text_append
    fn.restype = ctypes.c_int
    fn.argtypes = _lib.SIGNATURES["fq3_batch_text_append"][1]
    one = (ctypes.c_int32 * 1)(0)
    assert fn(None, 1, one, one, one, None, None) == -1                        # FQ3_EINVAL: null batch, before any device call
    from fq3hip.engine import Fq3Batch
    assert callable(getattr(Fq3Batch, "text_append", None))


# ---- server: text sessions against a stub worker ------------------------------------------------------------------------------------
class _StubWorker:
    """Stands in for ``BatchWorker``: a session's audio is one chunk per piece of text it was fed (sample k of the chunk = k-th byte)."""

    def __init__(self):
        import queue
        self.queue, self.sessions = queue, []

    def submit_text(self, cfg, feeder):
        import threading
        import numpy as np
        from fq3hip.server import BatchWorker
        out = self.queue.Queue()
        self.sessions.append((cfg, feeder, out))

        def run():
            while True:
                ids, closed = feeder.take(block=True, timeout=5.0)
                if ids:
                    out.put(np.asarray(ids, dtype=np.float32) / 32768.0)
                if closed or not ids:
                    out.put(BatchWorker.DONE)
                    return
        threading.Thread(target=run, daemon=True).start()
        return out


def test_server_sessions():
    import numpy as np
    from starlette.testclient import TestClient
    from fq3hip.server import create_app
    icl_only = SimpleNamespace(icl_mode=True)
    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "ignored by sessions", "language": "English"},
              "icl": {"voice_clone_prompt": [icl_only], "language": "English"}}
    model = SimpleNamespace(sample_rate=24000, _text_tokenize=lambda: (lambda s: list(s.encode())))
    worker = _StubWorker()
    client = TestClient(create_app(model, voices, default_voice="alloy", scheduler="batch", worker=worker))
    base = "/v1/audio/speech/sessions"
    r = client.post(base, json={"voice": "icl"})
    assert r.status_code == 400 and "x-vector-only" in r.json()["detail"]                 # says why
    assert client.post(base, json={"voice": "alloy", "response_format": "mp3"}).status_code == 400
    assert client.post(base + "/nope/text", json={"text": "a"}).status_code == 404
    assert client.get(base + "/nope/audio").status_code == 404
    a = client.post(base, json={"voice": "alloy", "response_format": "pcm"}).json()["id"]
    b = client.post(base, json={"voice": "alloy", "response_format": "wav"}).json()["id"]
    assert a != b and len(worker.sessions) == 2 and worker.sessions[0][0] is voices["alloy"]
    # whole words are released at the next whitespace (TextFeeder), the tail at `final`
    assert client.post(f"{base}/{a}/text", json={"text": "ab cd"}).json() == {"id": a, "final": False}
    assert client.post(f"{base}/{b}/text", json={"text": "xyz", "final": True}).json() == {"id": b, "final": True}
    assert client.post(f"{base}/{a}/text", json={"text": " ef", "final": True}).status_code == 200
    assert client.post(f"{base}/{a}/text", json={"text": "late"}).status_code == 409        # text after final
    ra = client.get(f"{base}/{a}/audio")
    assert ra.status_code == 200 and ra.headers["content-type"].startswith("audio/pcm")
    got = np.frombuffer(ra.content, dtype="<i2").tolist()
    assert got == list(b"ab cd ef")                                                        # audio bytes in order
    rb = client.get(f"{base}/{b}/audio")
    assert rb.status_code == 200 and rb.content[:4] == b"RIFF" and np.frombuffer(rb.content[44:], dtype="<i2").tolist() == list(b"xyz")
    # dropped at the end
    assert client.get(f"{base}/{a}/audio").status_code == 404 and client.post(f"{base}/{b}/text", json={"text": "x"}).status_code == 404
    # the lock scheduler has no lanes to put sessions in
    lock_client = TestClient(create_app(model, voices, default_voice="alloy", scheduler="lock"))
    assert lock_client.post(base, json={"voice": "alloy"}).status_code == 400
