"""CPU: the host side of seeded sampling -- seed validation and expansion, the ``seeded`` context, the refill
switch, the scheduler's one fill per step, the server's ``seed`` field under both schedulers and in text sessions, the CLI flag."""
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fq3hip import cli
from fq3hip.generate import NOISE_RING, _refill, expand_seeds, run_frames, validate_seed


# ---- validation and expansion ----------------------------------------------------------------------------------------------------------
def test_validate_seed():
    assert validate_seed(None) is None
    assert validate_seed(0) == 0 and validate_seed(2 ** 64 - 1) == 2 ** 64 - 1
    assert validate_seed(np.int64(7)) == 7 and type(validate_seed(np.uint64(2 ** 63))) is int
    for bad in (-1, 2 ** 64, 1.0, "7", True, [1], 1 + 0j):
        with pytest.raises(ValueError):
            validate_seed(bad)


def test_seeds_int_expands_to_s_plus_i_modulo_2_64():
    assert expand_seeds(None, 3) == [None, None, None]
    assert expand_seeds(5, 3) == [5, 6, 7]
    assert expand_seeds(2 ** 64 - 2, 4) == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    assert expand_seeds([9, None, 2 ** 64 - 1], 3) == [9, None, 2 ** 64 - 1]
    assert expand_seeds((1, 2), 2) == [1, 2]
    for bad, n in (([1, 2], 3), (-1, 2), (2 ** 64, 1), ([1, -1], 2), ([1, "x"], 2), (1.5, 2)):
        with pytest.raises(ValueError):
            expand_seeds(bad, n)


# ---- the seeded() context --------------------------------------------------------------------------------------------------------------
def _bare_model():
    from fq3hip.model import FasterQwen3TTS
    inner = SimpleNamespace(tts_model_type="base", tts_model_size="0b6", speech_tokenizer=None)
    return FasterQwen3TTS(SimpleNamespace(model=inner, sample_rate=24000), None, None, device="cpu")


def test_seeded_restores_the_previous_state():
    m = _bare_model()
    assert m._seed is None and m._seed_kw() == {}
    with m.seeded(11) as s:
        assert s == 11 and m._seed_kw() == {"seed": 11}
        with m.seeded(2 ** 64 - 1):
            assert m._seed_kw() == {"seed": 2 ** 64 - 1}
        assert m._seed_kw() == {"seed": 11}
        with m.seeded(None):                                   # an unseeded stretch inside a seeded one
            assert m._seed_kw() == {}
        assert m._seed_kw() == {"seed": 11}
    assert m._seed is None
    with pytest.raises(RuntimeError):
        with m.seeded(3):
            raise RuntimeError("inside")
    assert m._seed is None
    for bad in (-1, 2 ** 64, "1", 2.0):
        with pytest.raises(ValueError):
            with m.seeded(bad):
                pass
        assert m._seed is None


def test_seeded_reaches_the_decode_loop(monkeypatch):
    """Inside ``seeded`` the one-shot back half passes ``seed=`` to ``fast_generate``; outside it the call has no such keyword."""
    import fq3hip.generate as G
    seen = []

    def fake(**kw):
        seen.append(kw.get("seed", "absent"))
        return None, {"steps": 0, "prefill_ms": 0.0, "decode_s": 0.0, "ms_per_step": 0.0}
    monkeypatch.setattr(G, "fast_generate", fake)
    m = _bare_model()
    m._run_full(None, None, None, None, None, None, None, None, {})
    with m.seeded(42):
        m._run_full(None, None, None, None, None, None, None, None, {})
    assert seen == ["absent", 42]


def test_seeded_reaches_the_streaming_loops_parity_mode_included(monkeypatch):
    """``_run_streaming`` under ``seeded``: the graph path and the parity path (direct launches, ``parity_generate_streaming``, which
    forwards to ``fast_generate_streaming``) both receive the seed; outside the context neither receives the keyword."""
    import fq3hip.streaming as S
    seen = []

    def fake(*a, **kw):
        seen.append((kw.get("use_graph", True), kw.get("seed", "absent")))
        return iter(())
    monkeypatch.setattr(S, "fast_generate_streaming", fake)
    m = _bare_model()
    m._vocoder_stream = lambda tok: None
    m.predictor_graph = m.talker_graph = object()          # (the parity path insists on graph objects; the fake loop reads neither)
    inner = SimpleNamespace(speech_tokenizer=SimpleNamespace())

    def run(parity):
        assert list(m._run_streaming(inner, None, None, None, None, None, None, None, {}, 12, parity_mode=parity)) == []
    run(False), run(True)
    with m.seeded(2 ** 64 - 1):
        run(False), run(True)
    assert seen == [(True, "absent"), (False, None), (True, 2 ** 64 - 1), (False, 2 ** 64 - 1)]


def test_seeds_are_expanded_in_one_place_and_refused_beside_rounds():
    m = _bare_model()
    with pytest.raises(ValueError, match="rounds"):
        next(m._run_batch_streaming(None, {}, 12, 2, rounds=lambda dec, meta: [], seeds=5))
    with pytest.raises(ValueError, match="count"):
        next(m._run_batch_streaming(iter(()), {}, 12, 2, seeds=[1]))
    with pytest.raises(ValueError):
        next(m._run_batch_streaming(iter(()), {}, 12, 2, seeds=[1], count=2))
    with pytest.raises(ValueError):
        m._run_batch_full(iter(()), {}, 2, 2, seeds=2 ** 64)


# ---- the refill switch -----------------------------------------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self):
        self.fills, self.frames = [], []

    def noise_fill(self, tn, pn, seed, first_frame=0, n_frames=None, ring_frames=None):
        self.fills.append((tn, pn, seed, first_frame))

    def decode_frames(self, n):
        self.frames.append(n)


class _Ring:
    def __init__(self):
        self.draws = 0

    def exponential_(self, lam):
        self.draws += 1
        return self


def test_refill_unseeded_draws_and_seeded_fills():
    eng, tn, pn = _StubEngine(), _Ring(), _Ring()
    _refill(eng, tn, pn)
    _refill(eng, tn, pn, seed=None)
    assert (tn.draws, pn.draws) == (2, 2) and eng.fills == []
    _refill(eng, tn, None, seed=9, first_frame=128)
    assert (tn.draws, pn.draws) == (2, 2) and eng.fills == [(tn, None, 9, 128)]
    _refill(eng, None, None, seed=9)                         # greedy everywhere: nothing to fill
    assert len(eng.fills) == 1


def test_run_frames_refills_with_the_frame_index():
    eng, tn, pn = _StubEngine(), _Ring(), _Ring()
    issued = run_frames(eng, tn, pn, 0, 60, seed=5)
    issued = run_frames(eng, tn, pn, issued, 80, seed=5)     # crosses 64 and 128
    assert issued == 140 and [f[3] for f in eng.fills] == [0, NOISE_RING, 2 * NOISE_RING] and tn.draws == 0
    assert eng.frames == [60, 4, 64, 12]
    eng2 = _StubEngine()
    run_frames(eng2, tn, pn, 0, 70)
    assert eng2.fills == [] and tn.draws == 2 and pn.draws == 2


def test_text_session_refills_with_its_emitted_count():
    from fq3hip.text_stream import TextFeeder, TextSession
    calls = []
    eng = SimpleNamespace(decode_frames=lambda n: None, decode_text_append=lambda ids, final: None)
    f = TextFeeder()
    f.feed_ids(range(100))
    f.close()
    s = TextSession(eng, f, 1, 200, "tn", "pn", refill=lambda *a: calls.append(a), seed=77)
    s.pump(70, block=True)
    assert calls == [(eng, "tn", "pn", 77, 0), (eng, "tn", "pn", 77, 64)]
    calls.clear()
    f2 = TextFeeder()
    f2.feed_ids(range(10))
    f2.close()
    TextSession(eng, f2, 1, 200, "tn", "pn", refill=lambda *a: calls.append(a)).pump(5, block=True)
    assert calls == [(eng, "tn", "pn")]                      # unseeded: the call is what it was


# ---- the scheduler: seeded lanes at a ring boundary are filled together --------------------------------------------------------------
def test_scheduler_fills_seeded_lanes_in_one_call(monkeypatch):
    import fq3hip.batching as Bt
    fills, draws = [], []

    class Eng:
        device = SimpleNamespace(type="cpu")
        cfg = SimpleNamespace(num_code_groups=16)

        def __init__(self, i):
            self.i, self.n, self.max = i, 0, 0

        @staticmethod
        def noise_fill_many(items, ring_frames=None):
            fills.append([(it[0].i, it[3], it[4]) for it in items])
            assert ring_frames == NOISE_RING

        def decode_poll(self):
            return self.n, self.n >= self.max

        def decode_codes(self, start, count):
            return torch.zeros(count, 16, dtype=torch.long)

    class Batch:
        def __init__(self, engines):
            self.engines = engines

        def frames(self, n):
            for e in self.engines:
                e.n = min(e.n + n, e.max)

        def graph_capture(self):
            pass

    def arm(talker, tie, tam, tth, tpe, config, pg, tg, max_new, *a, use_graph=False, seed=None, **kw):
        tg.engine.n, tg.engine.max = 0, max_new
        arm.seeds.append(seed)
        return tg.engine, "tn%d" % tg.engine.i, "pn%d" % tg.engine.i, max_new
    arm.seeds = []
    monkeypatch.setattr(Bt, "_prefill_and_arm", arm)
    monkeypatch.setattr(Bt, "_refill", lambda eng, tn, pn: draws.append(eng.i))
    monkeypatch.setattr(Bt, "TalkerGraph", lambda e: SimpleNamespace(engine=e))
    monkeypatch.setattr(Bt, "PredictorGraph", lambda e, **kw: SimpleNamespace(engine=e, **kw))
    engines = [Eng(i) for i in range(3)]
    dec = Bt.BatchDecoder(engines, batch_factory=Batch, use_graph=False)
    reqs = [Bt.BatchRequest(rid, None, None, None, None, None, None, dict(max_new_tokens=n), seed=sd)
            for rid, n, sd in (("a", 70, 100), ("u", 70, None), ("b", 70, 2 ** 64 - 1), ("late", 8, 5))]
    done = [rid for rid, _codes, _t in dec.run(reqs)]
    assert sorted(done) == ["a", "b", "late", "u"]
    assert arm.seeds[:3] == [100, None, 2 ** 64 - 1] and arm.seeds[3] == 5
    # frame 0 and frame 64: lanes 0 and 2 in ONE call each time, the unseeded lane drawn as ever; the re-armed lane starts at frame 0
    assert fills[0] == [(0, 100, 0), (2, 2 ** 64 - 1, 0)] and fills[1] == [(0, 100, 64), (2, 2 ** 64 - 1, 64)]
    assert len(fills) == 3 and len(fills[2]) == 1 and fills[2][0][1:] == (5, 0)
    assert draws == [1, 1]
    with pytest.raises(ValueError):
        list(dec.run([Bt.BatchRequest("x", None, None, None, None, None, None, dict(max_new_tokens=4), seed=-3)]))


# ---- the server ------------------------------------------------------------------------------------------------------------------------
class _LockModel:
    sample_rate = 24000

    def __init__(self):
        self.calls, self._seed = [], None

    def seeded(self, seed):
        import contextlib

        @contextlib.contextmanager
        def ctx():
            prev, self._seed = self._seed, seed
            try:
                yield seed
            finally:
                self._seed = prev
        return ctx()

    def generate_voice_clone_streaming(self, text, chunk_size=12, **kw):
        self.calls.append((text, self._seed))
        yield np.full(240 * len(text), 0.25, np.float32), 24000, {"chunk_index": 0}


VOICES = {"alloy": {"voice_clone_prompt": {"x": 1}, "ref_text": "t", "language": "English"}}


def test_server_lock_scheduler_seed_field():
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app
    m = _LockModel()
    client = TestClient(create_app(m, VOICES, default_voice="alloy", scheduler="lock"))
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "response_format": "pcm", "seed": 2 ** 64 - 1})
    assert r.status_code == 200 and r.headers["x-seed"] == str(2 ** 64 - 1) and len(r.content) == 2 * 240 * 5
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and "x-seed" not in r.headers
    assert m.calls == [("hello", 2 ** 64 - 1), ("hello", None)] and m._seed is None
    for bad in (-1, 2 ** 64):
        r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "seed": bad})
        assert r.status_code == 400 and "seed" in r.text
    assert client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "seed": "soon"}).status_code == 422
    assert len(m.calls) == 2


class _BatchModel:
    """What BatchWorker needs from a model (as the scripted model of tests/test_serving_cpu.py), recording each request's seed."""
    sample_rate = 24000

    class _Voc:
        def push(self, codes, ready_event=None):
            return np.full(100 * int(codes.shape[0]), 0.5, np.float32), 24000

    class _Dec:
        lanes = ()

        def __init__(self, owner):
            self.owner = owner

        def run(self, requests, on_error="raise", source=None, chunk_frames=None):
            pending = list(requests)
            while True:
                while source is not None:                    # as the scheduler: the source is asked at every boundary, an empty start included
                    r = source()
                    if r is None:
                        break
                    pending.append(r)
                if not pending:
                    return
                req = pending.pop(0)
                self.owner.seeds.append((req.rid, req.seed))
                yield req.rid, torch.zeros(3, 16, dtype=torch.long), {"is_final": True, "total_steps_so_far": 3, "steps": 3}

    def __init__(self):
        self.seeds = []

    def _prepare_generation(self, text, **kw):
        return None, None, None, text, None, None, None, None

    @staticmethod
    def _gen_kwargs(*a):
        return {}

    def streaming_vocoder(self, rc, chunk):
        return self._Voc()

    def _batch_decoder(self, lanes):
        return self._Dec(self)

    # text sessions
    def _text_tokenize(self):
        return lambda s: list(s.encode())

    def _bind_lane_prompt_weights(self, dec):
        pass

    def text_batch_request(self, rid, feeder, prepare, gen_kwargs, seed=None):
        feeder.take(block=False)
        return SimpleNamespace(rid=rid, seed=seed)


def test_server_batch_scheduler_and_sessions_seed_field(monkeypatch):
    from fastapi.testclient import TestClient
    import fq3hip.batching as Bt
    from fq3hip.server import create_app

    class Req:
        def __init__(self, rid, talker, tie, tam, tth, tpe, config, kw, seed=None):
            self.rid, self.seed = rid, seed

    monkeypatch.setattr(Bt, "BatchRequest", Req)
    m = _BatchModel()
    client = TestClient(create_app(m, VOICES, default_voice="alloy", scheduler="batch", lanes=2, chunk_size=4))
    r = client.post("/v1/audio/speech", json={"input": "abc", "voice": "alloy", "response_format": "pcm", "seed": 12345})
    assert r.status_code == 200 and r.headers["x-seed"] == "12345" and len(r.content) == 2 * 100 * 3
    r = client.post("/v1/audio/speech", json={"input": "abc", "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and "x-seed" not in r.headers
    assert [s for _rid, s in m.seeds] == [12345, None]
    assert client.post("/v1/audio/speech", json={"input": "abc", "voice": "alloy", "seed": 2 ** 64}).status_code == 400
    assert client.post("/v1/audio/speech", json={"input": "abc", "voice": "alloy", "seed": -5}).status_code == 400
    # a text session
    assert client.post("/v1/audio/speech/sessions", json={"voice": "alloy", "seed": -1}).status_code == 400
    sid = client.post("/v1/audio/speech/sessions", json={"voice": "alloy", "response_format": "pcm", "seed": 2 ** 63})
    assert sid.status_code == 200 and sid.json()["seed"] == 2 ** 63
    sid = sid.json()["id"]
    assert client.post(f"/v1/audio/speech/sessions/{sid}/text", json={"text": "hello there", "final": True}).status_code == 200
    r = client.get(f"/v1/audio/speech/sessions/{sid}/audio")
    assert r.status_code == 200 and r.headers["x-seed"] == str(2 ** 63) and len(r.content) == 2 * 100 * 3
    assert m.seeds[-1][1] == 2 ** 63
    plain = client.post("/v1/audio/speech/sessions", json={"voice": "alloy", "response_format": "pcm"}).json()
    assert "seed" not in plain
    assert len(m.seeds) == 3


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_seed_flag(tmp_path):
    m = _LockModel()
    m.generate_voice_design = lambda text, instruct, **kw: (m.calls.append((text, m._seed)), ([np.zeros(240, np.float32)], 24000))[1]
    m.generate_custom_voice = lambda text, speaker, **kw: (m.calls.append((text, m._seed)), ([np.zeros(240, np.float32)], 24000))[1]
    m.generate_voice_clone = lambda text, **kw: (m.calls.append((text, m._seed)), ([np.zeros(240, np.float32)], 24000))[1]
    p = cli.build_parser()
    out = str(tmp_path / "o.wav")
    cli.cmd_once(p.parse_args(["design", "--text", "abc", "--output", out, "--instruct", "calm", "--seed", "77"]), model=m)
    cli.cmd_once(p.parse_args(["custom", "--text", "abc", "--output", out, "--speaker", "bob", "--seed", str(2 ** 64 - 1)]), model=m)
    cli.cmd_once(p.parse_args(["clone", "--text", "abc", "--output", out, "--ref-audio", "r.wav", "--ref-text", "t", "--seed", "0"]), model=m)
    cli.cmd_once(p.parse_args(["design", "--text", "abc", "--output", out, "--instruct", "calm"]), model=m)
    assert [c[1] for c in m.calls] == [77, 2 ** 64 - 1, 0, None] and m._seed is None
    assert p.parse_args(["design", "--text", "x", "--output", out, "--instruct", "i"]).seed is None
