"""CPU: the host side of the time-scale stage (fq3_tsm_design / fq3_tsm_count, argument checks that precede every HIP call), the
``speed`` field of ``AudioOutSpec``, and how the server and the CLI hand it on (stand-in worker and model, no GPU).  DESIGN.md
section 4.9."""
import contextlib
import ctypes as C
import queue
from types import SimpleNamespace

import numpy as np
import pytest

import _tsm_ref as R
from fq3hip import _lib, audio_io
from fq3hip import audio_out as ao

SPEEDS = (250, 500, 999, 1001, 1250, 2000, 4000)


def test_design():
    for P in SPEEDS:
        N, Hs, D, w = ao.tsm_design(24000, P)
        assert (N, Hs, D) == (480, 240, 240)
        assert w.dtype == np.float32 and w.shape == (480,)
        ref = R.hann(480)
        assert np.all(np.abs(w.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)).astype(np.float64))     # within 1 ulp
        assert np.abs(w[:240].astype(np.float64) + w[240:].astype(np.float64) - 1.0).max() <= 2.0 ** -23
    assert ao.tsm_design(16000, 1500, window=False) == (320, 160, 160, None)
    assert ao.tsm_design(8000, 1500, window=False)[:3] == (160, 80, 80)


@pytest.mark.parametrize("P", SPEEDS)
def test_count_rules(P):
    Hs = 240
    prev = 0
    for n in list(range(0, 3000)) + [15360, 1 << 40]:
        T = R.total(n, P)
        c = ao.tsm_count(24000, P, n, False)
        assert c >= prev, (P, n)                              # non-decreasing
        prev = c
        assert c <= T and c % Hs == 0, (P, n, c, T)
        assert ao.tsm_count(24000, P, n, True) == T
        S = c // Hs
        if S > 0:
            assert R.need(S - 1, P) <= n, (P, n, S)           # every counted segment has all its candidates' samples
        assert R.need(S, P) > n or (S + 1) * Hs > T, (P, n, S)   # the next one lacks samples, or would pass the cap
    assert ao.tsm_count(24000, P, 1 << 40, True) == R.total(1 << 40, P)


def test_cap_binds_at_four_times():
    """at 4x the plain need rule would hand out more than a stream ending there has: the cap is what keeps the count below T"""
    hit = 0
    for n in range(0, 3000):
        S = ao.tsm_count(24000, 4000, n, False) // 240
        if R.need(S, 4000) <= n:
            hit += 1
            assert (S + 1) * 240 > R.total(n, 4000)
    assert hit > 0


@pytest.mark.parametrize("rate", [8000, 24000, 48000])
def test_history_reaches_the_next_segment(rate):
    """The object keeps a fixed history (plan_ in csrc/fq3_tsm.hip; ``R.history_bound`` restates its size).  Whatever the cumulative
    length n, the first segment the count has NOT handed out must find everything it can read, from ``R.reach`` on, inside it -- at the
    extremes too (0.25x: the need rule binds; 4x: the cap does), which no GPU test streams.  A change of the need rule or of the cap
    that breaks this fails here and not as FQ3_ESTATE in a running stream."""
    hs = rate // 100
    for P in (250, 251, 333, 500, 999, 1000, 1001, 1250, 1999, 2000, 3001, 3999, 4000):
        bound, worst = R.history_bound(P, hs), 0
        for n in list(range(0, 12 * hs, 1)) + list(range(1000 * hs, 1000 * hs + 5 * hs)):
            c = ao.tsm_count(rate, P, n, False)
            assert c % hs == 0
            worst = max(worst, n - R.reach(c // hs, P, hs))
        assert worst <= bound, (rate, P, worst, bound)
        assert worst >= bound - 8, (rate, P, worst, bound)      # the bound is tight: the test would see it move


def test_errors_are_codes_not_crashes():
    lib = _lib.load()
    N, Hs, D = C.c_int(), C.c_int(), C.c_int()
    assert lib.fq3_tsm_design(24000, 1250, None, Hs, D, None, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_tsm_design(24000, 1250, N, None, D, None, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_tsm_design(24000, 1250, N, Hs, None, None, 0) == _lib.FQ3_EINVAL
    for P in (249, 4001, 0, -1000):
        assert lib.fq3_tsm_design(24000, P, N, Hs, D, None, 0) == _lib.FQ3_EINVAL
        assert b"[0.25, 4.0]" in lib.fq3_last_error()
        assert lib.fq3_tsm_count(24000, P, 100, 0) == _lib.FQ3_EINVAL
    for rate in (0, -24000, 44100, 96000, 500):                # no hop / a hop that is no multiple of 16 / above 480 / below 16
        assert lib.fq3_tsm_design(rate, 1250, N, Hs, D, None, 0) == _lib.FQ3_EINVAL
    small = (C.c_float * 479)()
    assert lib.fq3_tsm_design(24000, 1250, N, Hs, D, small, 479) == _lib.FQ3_EINVAL          # window capacity below N
    assert lib.fq3_tsm_design(24000, 250, N, Hs, D, None, 0) == 0 and lib.fq3_tsm_design(24000, 4000, N, Hs, D, None, 0) == 0
    assert lib.fq3_tsm_count(24000, 1250, -1, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_tsm_count(24000, 1250, -1, 1) == _lib.FQ3_EINVAL
    h = C.c_void_p()
    assert lib.fq3_tsm_create(None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_tsm_create(None, C.byref(h)) == _lib.FQ3_EINVAL
    good = _lib.TsmConfig(24000, 1250)
    assert lib.fq3_tsm_create(C.byref(good), None) == _lib.FQ3_EINVAL
    for bad in (_lib.TsmConfig(24000, 100), _lib.TsmConfig(24000, 5000), _lib.TsmConfig(44100, 1250)):      # before any HIP call
        assert lib.fq3_tsm_create(C.byref(bad), C.byref(h)) == _lib.FQ3_EINVAL and not h.value
    n = C.c_int64()
    assert lib.fq3_tsm_push(None, None, 0, 0, None, 0, C.byref(n), None, 0, None) == _lib.FQ3_EINVAL
    assert lib.fq3_tsm_reset(None, None) == _lib.FQ3_EINVAL and lib.fq3_tsm_destroy(None) == 0


def test_spec_speed_validation():
    for bad in (0.2, 4.5, float("nan"), float("inf"), "1.5", None, True, 0.2494, 4.0006):
        with pytest.raises(ValueError):
            ao.AudioOutSpec(speed=bad)
    for ok, P in ((0.25, 250), (4.0, 4000), (1.5, 1500), (2, 2000), (np.float32(1.25), 1250), (0.2496, 250), (1.0004, 1000)):
        assert ao.AudioOutSpec(8000, "mulaw", ok).validate(24000).permille == P
    # 1.0 is today's spec: the same fields first, equal, no time-scale stage
    assert ao.AudioOutSpec(8000, "mulaw") == ao.AudioOutSpec(8000, "mulaw", 1.0) == ao.AudioOutSpec(8000, "mulaw", speed=1.0)
    assert ao.AudioOutSpec(8000, "mulaw").speed == 1.0 and ao.AudioOutSpec().permille == 1000
    assert ao.AudioOutSpec(None, "s16", 1.5).out_rate(24000) == 24000
    with pytest.raises(ValueError):
        ao.AudioOutSpec(None, "f32", 1.5).validate(44100)      # the time-scale stage refuses the rate, with the library's reason
    ao.AudioOutSpec(None, "f32", 1.0).validate(44100)          # ... and is not asked without a speed


# ---- server: `speed` reaches the worker / the model; 1.0 alone is today's path ----------------------------------------------------
class _Worker:
    """Stand-in for ``BatchWorker``: fixed chunks; a request with a spec gets bytes 'encoded' to its dtype."""

    def __init__(self):
        self.seen, self.sessions = [], []
        self.chunks = [np.linspace(-1.2, 1.2, 700).astype(np.float32), np.full(300, 0.25, np.float32)]

    def _box(self, cfg):
        from fq3hip.server import BatchWorker
        box = queue.Queue()
        spec = cfg.get("audio_output")
        for c in self.chunks:
            box.put(c if spec is None else np.arange(len(c) // 3, dtype=ao.NUMPY_DTYPES[spec.encoding]))
        box.put(BatchWorker.DONE)
        return box

    def submit(self, cfg, text):
        self.seen.append(cfg)
        return self._box(cfg)

    def submit_text(self, cfg, feeder):
        self.sessions.append(cfg)
        return self._box(cfg)


def _client(model, worker=None, scheduler="batch"):
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app
    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "t", "language": "English"}}
    return TestClient(create_app(model, voices, default_voice="alloy", scheduler=scheduler, worker=worker)), voices


def test_server_batch_scheduler_applies_speed():
    w = _Worker()
    model = SimpleNamespace(sample_rate=24000, _text_tokenize=lambda: (lambda s: list(s.encode())))
    client, voices = _client(model, w)
    req = {"input": "hello", "voice": "alloy", "response_format": "wav"}
    r = client.post("/v1/audio/speech", json=dict(req, speed=1.5))
    assert r.status_code == 200
    spec = w.seen[-1]["audio_output"]
    assert spec.speed == 1.5 and spec == ao.AudioOutSpec(None, "s16", 1.5) and "audio_output" not in voices["alloy"]
    # speed alone: the container and sample format of a request without it
    assert r.content[:44] == audio_io.wav_header(24000)
    assert r.content[44:] == b"".join(np.arange(len(c) // 3, dtype="<i2").tobytes() for c in w.chunks)
    r = client.post("/v1/audio/speech", json=dict(req, speed=0.5, sample_rate=8000, encoding="mulaw"))
    assert r.status_code == 200 and w.seen[-1]["audio_output"] == ao.AudioOutSpec(8000, "mulaw", 0.5)
    assert r.content[:58] == audio_io.wav_header_for(8000, "mulaw")
    # 1.0 alone is no spec at all: today's path, today's bytes
    plain = client.post("/v1/audio/speech", json=req)
    for body in (dict(req, speed=1.0), dict(req, speed=1)):
        r = client.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and w.seen[-1] is voices["alloy"] and r.content == plain.content
    n = len(w.seen)
    for bad in (9, 0.1, -1):
        r = client.post("/v1/audio/speech", json=dict(req, speed=bad))
        assert r.status_code == 400 and "[0.25, 4.0]" in r.json()["detail"], r.text
    assert len(w.seen) == n                                     # refused before anything was submitted
    # text sessions take the field too
    base = "/v1/audio/speech/sessions"
    assert client.post(base, json={"voice": "alloy", "speed": 1.25}).status_code == 200
    assert w.sessions[-1]["audio_output"] == ao.AudioOutSpec(None, "s16", 1.25)
    assert client.post(base, json={"voice": "alloy", "speed": 1.0}).status_code == 200
    assert w.sessions[-1] is voices["alloy"]
    assert client.post(base, json={"voice": "alloy", "speed": 9}).status_code == 400
    assert len(w.sessions) == 2


class _Model:
    """Stand-in for ``FasterQwen3TTS`` under the lock scheduler: notes the arguments of ``audio_output``"""
    sample_rate = 24000

    def __init__(self):
        self.contexts, self.open = [], None

    @contextlib.contextmanager
    def audio_output(self, sample_rate=None, encoding="f32", speed=1.0):
        self.contexts.append((sample_rate, encoding, speed))
        self.open = ao.AudioOutSpec(sample_rate, encoding, speed)
        try:
            yield self.open
        finally:
            self.open = None

    def generate_voice_clone_streaming(self, **kw):
        dt = np.float32 if self.open is None else ao.NUMPY_DTYPES[self.open.encoding]
        for n in (500, 200):
            yield np.ones(n, dtype=dt), 24000, {}


def test_server_lock_scheduler_applies_speed():
    m = _Model()
    client, _voices = _client(m, scheduler="lock")
    req = {"input": "hello", "voice": "alloy", "response_format": "pcm"}
    r = client.post("/v1/audio/speech", json=dict(req, speed=1.5))
    assert r.status_code == 200 and m.contexts == [(None, "s16", 1.5)]
    assert r.content == np.ones(700, dtype="<i2").tobytes()
    r = client.post("/v1/audio/speech", json=dict(req, speed=1.0))
    assert r.status_code == 200 and len(m.contexts) == 1       # no context at all
    assert r.content == audio_io.to_pcm16(np.ones(700, dtype=np.float32))
    assert client.post("/v1/audio/speech", json=dict(req, speed=9)).status_code == 400 and len(m.contexts) == 1


def test_cli_speed_flag():
    from fq3hip import cli
    base = ["custom", "--text", "x", "--output", "o.wav", "--speaker", "s"]
    a = cli.build_parser().parse_args(base + ["--speed", "1.25"])
    assert a.speed == 1.25 and a.out_rate is None and a.encoding is None
    assert cli.build_parser().parse_args(base).speed is None
    m = _Model()
    with cli._output_stage(m, a):
        pass
    assert m.contexts == [(None, "f32", 1.25)]
    with cli._output_stage(m, cli.build_parser().parse_args(base)):
        pass
    assert len(m.contexts) == 1                                 # no flag: no context
    with cli._output_stage(m, cli.build_parser().parse_args(base + ["--out-rate", "8000", "--encoding", "mulaw", "--speed", "2"])):
        pass
    assert m.contexts[-1] == (8000, "mulaw", 2.0)
