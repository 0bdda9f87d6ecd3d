"""CPU: the leveller's contract (include/fq3hip.h, "Leveller") as tests/_level_ref.py restates it -- cut
independence, the last target against the one-shot gain, leading silence, convergence to the target level, the bound on the gain's
step -- and everything of the stage that needs no GPU: the spec, the bindings, the model's context, the command line and the server."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import _level_ref as R
import _loud_ref as LR
from fq3hip import _lib
from fq3hip import leveller as M

RATES = (8000, 24000)


def _noise(rate):
    H = rate // 10
    return (0.03 * np.random.default_rng(1).standard_normal(40 * H + 37)).astype(np.float32)


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_reference_is_cut_independent(rate):
    H = rate // 10
    x = R.signals(rate)["lead"]
    for spec in (M.LevelSpec(), M.LevelSpec(initial_gain_db=6.0, smooth_hops=3, min_blocks=2)):
        whole = R.level(x, rate, spec)
        for sizes in ([1, H - 1, H, H + 1, 2 * H + 3, 0], [H], [4097]):
            ref, pos, k, ys = R.RefLeveller(rate, spec), 0, 0, []
            while pos < len(x):
                step = sizes[k % len(sizes)]
                k += 1
                ys.append(ref.push(x[pos:pos + step]))
                pos += step
            ys.append(ref.push(x[:0]))                                 # an empty push at the end
            assert np.concatenate(ys).tobytes() == whole["y"].tobytes(), sizes
            assert np.array(ref.T, dtype=np.float32).tobytes() == whole["T"].tobytes()


@pytest.mark.parametrize("rate", RATES)
def test_last_target_of_a_whole_hop_stream_is_the_one_shot_gain(rate):
    H = rate // 10
    for name, spec in (("bursts", M.LevelSpec()), ("lead", M.LevelSpec(min_blocks=3)), ("bursts", M.LevelSpec(initial_gain_db=-6.0, min_blocks=27))):
        x = R.signals(rate)[name][:30 * H]
        r = R.level(x, rate, spec)
        d = r["design"]
        one = LR.gate(LR.emulate_hops(x, d.coef32, H), LR.peak_and_bad(x)[0], 0, d)
        assert one["valid"] == 1 and one["n_abs"] >= spec.min_blocks
        assert r["T"][-1].tobytes() == np.float32(one["gain"]).tobytes() and len(r["T"]) == 31
        assert (r["stats"]["n_abs"], r["stats"]["n_rel"], r["stats"]["mean_power"]) == (one["n_abs"], one["n_rel"], one["mean_power"])
    # one block fewer than min_blocks: the prefix is measured, and the target still is the initial gain
    r = R.level(x, rate, M.LevelSpec(initial_gain_db=-6.0, min_blocks=28))
    assert r["stats"]["n_abs"] == 27 and r["stats"]["valid"] == 0 and (r["T"] == M.LevelSpec(initial_gain_db=-6.0).g0).all()


@pytest.mark.parametrize("rate", RATES)
def test_leading_zeros_leave_the_initial_gain_and_zeros(rate):
    H = rate // 10
    x = R.signals(rate)["lead"]
    for spec in (M.LevelSpec(), M.LevelSpec(initial_gain_db=6.0)):
        r = R.level(x, rate, spec)
        d = r["design"]
        n_abs = [LR.gate(r["energy"][:h], np.float32(0), 0, d)["n_abs"] for h in range(len(r["T"]))]
        few = np.array(n_abs) < spec.min_blocks
        assert few[:19].all() and not few[-1]
        assert (r["T"][few] == spec.g0).all() and (r["T"][~few] != spec.g0).all()
        # g = g0 exactly while every target that enters the smoothing is g0: up to the end of the last such hop
        last = int(np.flatnonzero(few)[-1])
        assert (r["g"][:(last + 1) * H] == spec.g0).all() and not r["y"][:10 * H].any()
        assert (r["y"][10 * H:(last + 1) * H] == x[10 * H:(last + 1) * H] * spec.g0).all()


def test_convergence_to_the_target():
    """Stationary noise at about -28 LUFS: behind hop m + 3 + k the levelled tail reads the target by the float64 measure.
    Measured with the float32 reference at the defaults (m = 8, k = 10, tail from hop 21): -16.084 LUFS at 8 kHz (0.084 LU under the
    target of -16), -15.978 LUFS at 24 kHz (0.022 LU over).  The margin is twice the larger offset: 0.17 LU (< 0.5 LU)."""
    margin = 0.17
    assert margin == round(2 * 0.084, 2) and margin < 0.5
    spec = M.LevelSpec()
    for rate in RATES:
        H = rate // 10
        x = _noise(rate)
        assert -29.0 < LR.measure64(x, rate) < -27.0                    # the input reads about -28 LUFS: 12 dB under the target
        r = R.level(x, rate, spec)
        tail = r["y"][(spec.min_blocks + 3 + spec.smooth_hops) * H:]
        got = LR.measure64(tail, rate)
        print(f"{rate} Hz: levelled tail reads {got:.3f} LUFS (target {spec.target_lufs})")
        assert abs(got - spec.target_lufs) <= margin, (rate, got)


@pytest.mark.parametrize("rate", RATES)
def test_gain_step_between_neighbouring_samples_is_bounded(rate):
    H = rate // 10
    for name in ("bursts", "lead", "noise"):
        for spec in (M.LevelSpec(), M.LevelSpec(initial_gain_db=6.0, smooth_hops=3, min_blocks=2), M.LevelSpec(smooth_hops=1, min_blocks=1)):
            x = _noise(rate) if name == "noise" else R.signals(rate)[name]
            r = R.level(x, rate, spec)
            d = r["design"]
            lo = min(float(spec.g0), float(r["T"].min()))
            bound = (d.max_gain - lo) / (spec.smooth_hops * H)
            # float rounding: the ramp's value is rounded to float32 at both ends of a step (half an ulp of Gmax each), and so are S and
            # the ramp's fraction
            slack = 4 * float(np.spacing(np.float32(d.max_gain)))
            step = float(np.abs(np.diff(r["g"].astype(np.float64))).max())
            assert step <= bound + slack, (name, spec, step, bound)
            assert (r["g"] >= np.float32(lo)).all() and (r["g"] <= np.float32(d.max_gain)).all()


# ---- the spec and the bindings -------------------------------------------------------------------------------------------------------------
def test_spec_validation():
    s = M.LevelSpec()
    assert (s.target_lufs, s.ceiling_db, s.max_gain_db, s.initial_gain_db, s.smooth_hops, s.min_blocks) == (-16.0, -1.0, 20.0, 0.0, 10, 8)
    assert s.g0 == np.float32(1.0) and M.LevelSpec(initial_gain_db=6.0).g0 == np.float32(10.0 ** 0.3)
    assert "NOT been tuned" in M.LevelSpec.__doc__ and "NOT limit" in M.Leveller.__doc__ + M.__doc__
    for kw in (dict(target_lufs=-41.0), dict(target_lufs=-4.0), dict(ceiling_db=0.5), dict(max_gain_db=41.0), dict(initial_gain_db=-61.0),
               dict(initial_gain_db=40.5), dict(initial_gain_db=float("nan")), dict(smooth_hops=0), dict(smooth_hops=65), dict(smooth_hops=2.5),
               dict(min_blocks=0), dict(min_blocks=65), dict(min_blocks=True), dict(target_lufs="-16")):
        with pytest.raises(ValueError):
            M.LevelSpec(**kw)
    for kw in (dict(smooth_hops=1, min_blocks=1), dict(smooth_hops=64, min_blocks=64, initial_gain_db=40.0)):
        M.LevelSpec(**kw)
    with pytest.raises(ValueError):
        M.Leveller(None, 24000, "cpu")
    with pytest.raises(ValueError, match="2\\^20"):
        M.capacity_for((1 << 20) * 2400, 24000)
    assert M.capacity_for(72037, 24000) == 31


def test_range_errors_and_null_arguments_come_without_a_hip_call():
    lib, h = _lib.load(), C.c_void_p()
    for cfg in ((8050, -16.0, -1.0, 20.0, 0.0, 10, 8, 0), (24000, -41.0, -1.0, 20.0, 0.0, 10, 8, 0), (24000, -16.0, -1.0, 20.0, 41.0, 10, 8, 0),
                (24000, -16.0, -1.0, 20.0, 0.0, 0, 8, 0), (24000, -16.0, -1.0, 20.0, 0.0, 10, 65, 0), (24000, -16.0, -1.0, 20.0, 0.0, 10, 8, -1),
                (24000, -16.0, -1.0, 20.0, 0.0, 10, 8, (1 << 20) + 1), (24000, -16.0, -1.0, 20.0, float("nan"), 10, 8, 0)):
        c = _lib.LevelConfig(*cfg)
        assert lib.fq3_level_create(C.byref(c), C.byref(h)) == _lib.FQ3_EINVAL and not h.value, cfg
    assert lib.fq3_level_create(None, C.byref(h)) == _lib.FQ3_EINVAL
    assert lib.fq3_level_destroy(None) == 0
    n = C.c_int64()
    assert lib.fq3_level_reset(None, None) == _lib.FQ3_EINVAL and lib.fq3_level_push(None, None, 0, 0, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_level_stats(None, None, None) == _lib.FQ3_EINVAL and lib.fq3_level_set_initial_gain(None, 0.0) == _lib.FQ3_EINVAL
    assert lib.fq3_level_trace(None, None, None, None, None, 0, C.byref(n), None) == _lib.FQ3_EINVAL
    assert b"fq3_level_trace" in lib.fq3_last_error()


def test_bindings_match_the_header():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fq3hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(fq3_level_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(n for n in _lib.SIGNATURES if n.startswith("fq3_level_")) == [
        "fq3_level_create", "fq3_level_destroy", "fq3_level_push", "fq3_level_reset", "fq3_level_set_initial_gain", "fq3_level_stats",
        "fq3_level_trace"]
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        want = [C.c_void_p if "*" in a and "int64_t* n_hops" not in a and "fq3_level_config" not in a and "fq3_level**" not in a
                else None if "*" in a else ctype[a.split()[0]] for a in args]
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and len(got) == len(want), name
        assert all(w is None or w is g for w, g in zip(want, got)), (name, got)
    assert _lib.SIGNATURES["fq3_level_trace"][1][6]._type_ is C.c_int64 and _lib.SIGNATURES["fq3_level_create"][1][0]._type_ is _lib.LevelConfig
    # the two structs, field for field
    for cname, struct in (("fq3_level_config", _lib.LevelConfig), ("fq3_level_report", _lib.LevelReport)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}" % cname, code, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            parts = decl.replace(",", " ").split()
            fields += [(n, parts[0]) for n in parts[1:]]
        kinds = {"int": C.c_int, "double": C.c_double, "float": C.c_float, "int32_t": C.c_int32}
        assert [(n, kinds[t]) for n, t in fields] == list(struct._fields_), cname
    assert C.sizeof(_lib.LevelReport) == 40 and M.STATS_BYTES == 40
    assert _lib.load().fq3_abi_version() == 5                         # additive: the version stays


# ---- the model's context, the command line and the server (no GPU) ---------------------------------------------------------------------
def test_model_context_validates_and_composes():
    from fq3hip.model import FasterQwen3TTS
    m = FasterQwen3TTS.__new__(FasterQwen3TTS)
    m.sample_rate, m.device, m._audio_spec, m._loud, m._gain, m._limit = 24000, "cuda:0", None, None, None, None
    assert not m._levelling() and m._gain_kw() == {} and m.last_level_gain_db is None
    for kw in (dict(target_lufs=-4.0), dict(ceiling_db=1.0), dict(max_gain_db=50.0), dict(initial_gain_db=41.0), dict(smooth_hops=0), dict(min_blocks=65)):
        with pytest.raises(ValueError):
            with m.leveller(**kw):
                pass
    with m.leveller(-20.0) as spec:
        assert spec == M.LevelSpec(-20.0) and m._lvl is spec and m._levelling()
        assert m._gain_kw() == dict(leveller=spec, leveller_pool=[], leveller_hops=4096) and m._gain_kw()["leveller_pool"] is m._leveller_pools[spec]
        with pytest.raises(ValueError, match="same question"):       # leveller() together with loudness() raises, either way round
            with m.loudness():
                pass
        with m.limiter(-2.0):
            assert set(m._gain_kw()) == {"limiter", "limiter_pool", "leveller", "leveller_pool", "leveller_hops"}
        with m.fixed_gain(6.0), m.limiter(-2.0) as lim:              # composes with fixed_gain and limiter
            assert m._gain is not None and m._limit is lim and m._lvl is spec
        with m.leveller(initial_gain_db=3.0) as inner:
            assert m._lvl is inner
        assert m._lvl is spec
        # the initial gain is a per-stream value: contexts that differ in it alone share ONE pool, and no request adds a key
        pool = m._gain_kw()["leveller_pool"]
        for g in (-3.25, 1.5, 7.125):
            with m.leveller(-20.0, initial_gain_db=g) as warm:
                kw = m._gain_kw()
                assert kw["leveller"] is warm and warm.initial_gain_db == g and warm.pooled == spec and kw["leveller_pool"] is pool
        assert list(m._leveller_pools) == [spec]
        m.max_seq_len = 8192                                          # the capacity follows the frame limit: 8192 frames of 80 ms
        assert m._gain_kw()["leveller_hops"] == 8192 * 1920 // 2400 + 2 > 4096
    assert m._lvl is None and not m._levelling()
    with m.loudness():
        with pytest.raises(ValueError, match="same question"):
            with m.leveller():
                pass
        with pytest.raises(ValueError, match="fixed_gain"):          # loudness() still refuses a stream, in its own words
            m.streaming_vocoder(None, 12)
    assert "NOT limit" in FasterQwen3TTS.leveller.__doc__ and "NOT tuned" in FasterQwen3TTS.leveller.__doc__


def test_cli_flag():
    from fq3hip import cli
    p = cli.build_parser()
    base = ["custom", "--speaker", "bob", "--output", "o.wav", "--text", "hi"]
    for extra in ([], ["--streaming"], ["--long"], ["--gain-db", "12"], ["--limiter-db", "-2"], ["--streaming", "--exact-streaming"]):
        a = p.parse_args(base + extra + ["--level", "-18"])
        assert a.level == -18.0
        cli.check_level_args(p, a)
    assert p.parse_args(["serve", "--level", "-16"]).level == -16.0 and p.parse_args(base).level is None
    a = p.parse_args(["custom", "--speaker", "bob", "--output", "o.wav", "--text-stdin", "--level", "-16"])
    cli.check_level_args(p, a)                                         # the text-stream mode too
    for bad in (["--level", "-4"], ["--level", "-41"], ["--level", "nan"], ["--level", "-16", "--loudness", "-16"]):
        with pytest.raises(SystemExit):
            cli.check_level_args(p, p.parse_args(base + bad))

    class Fake:
        def __init__(self):
            self.seen = []

        def _ctx(self, *what):
            import contextlib
            self.seen.append(what)
            return contextlib.nullcontext()

        def fixed_gain(self, g):
            return self._ctx("fixed_gain", g)

        def leveller(self, **kw):
            return self._ctx("leveller", kw)

        def limiter(self, **kw):
            return self._ctx("limiter", kw)

    f = Fake()
    with cli._levelled(f, p.parse_args(base + ["--gain-db", "4", "--level", "-18", "--limiter-db", "-2"])):
        pass
    with cli._levelled(f, p.parse_args(base + ["--level", "-20"])):
        pass
    with cli._levelled(f, p.parse_args(base)):
        pass
    assert f.seen == [("fixed_gain", 4.0), ("leveller", dict(target_lufs=-18.0)), ("limiter", dict(ceiling_db=-2.0)),
                      ("leveller", dict(target_lufs=-20.0))]


def test_server_flag_and_voice_memory(caplog):
    import contextlib
    from fastapi.testclient import TestClient
    from fq3hip.server import build_parser, create_app, main, voice_key

    class Model:
        sample_rate = 24000

        def __init__(self, learn=(-3.25, None, -4.5)):
            self.entered, self.open, self.learn, self.last_level_gain_db = [], 0, list(learn), None

        @contextlib.contextmanager
        def leveller(self, target_lufs=-16.0, ceiling_db=-1.0, max_gain_db=20.0, initial_gain_db=0.0, smooth_hops=10, min_blocks=8):
            spec = M.LevelSpec(target_lufs, ceiling_db, max_gain_db, initial_gain_db, smooth_hops, min_blocks)
            self.entered.append(spec)
            self.open += 1
            try:
                yield spec
            finally:
                self.open -= 1

        @contextlib.contextmanager
        def limiter(self, ceiling_db=-1.0):
            from fq3hip.limiter import LimiterSpec
            yield LimiterSpec(ceiling_db)

        def generate_voice_clone_streaming(self, **kw):
            self.last_level_gain_db = self.learn.pop(0)              # what the stream's leveller ended with (None: no valid measure)
            yield np.zeros(240, dtype=np.float32), 24000, {}

    voices = {"v": {"ref_audio": "v.wav", "ref_text": "hello"}, "same": {"ref_audio": "v.wav", "ref_text": "hello", "language": "English"},
              "w": {"ref_audio": "w.wav"}, "bob": {"speaker": "bob"}}
    assert voice_key(voices["v"], "v") == voice_key(voices["same"], "same") == ("v.wav", "hello") != voice_key(voices["w"], "w")
    assert voice_key(voices["bob"], "x") == ("speaker", "bob") and voice_key({}, "n") == ("voice", "n")
    m = Model()
    with caplog.at_level("WARNING"):
        client = TestClient(create_app(m, voices, "v", scheduler="lock", level=-18.0))
    assert sum("does not limit" in r.getMessage() for r in caplog.records) == 1       # --level without --limiter-db: one warning
    assert m.entered == [M.LevelSpec(-18.0)] and m.open == 1              # entered once, for the life of the app
    h = client.get("/health").json()["level"]
    assert h == dict(target_lufs=-18.0, ceiling_db=-1.0, max_gain_db=20.0, smooth_hops=10, min_blocks=8, learned_gains_db={})
    post = lambda voice: client.post("/v1/audio/speech", json={"input": "hello", "voice": voice, "response_format": "pcm"})  # noqa: E731
    r = post("v")
    assert r.status_code == 200 and len(r.content) == 480 and "x-initial-gain-db" not in r.headers       # nothing learned yet
    assert client.get("/health").json()["level"]["learned_gains_db"] == {"('v.wav', 'hello')": -3.25}
    r = post("same")                                                    # the same clip under another name starts from what was learned ...
    assert r.headers["x-initial-gain-db"] == "-3.250" and m.entered[-1] == M.LevelSpec(-18.0, initial_gain_db=-3.25) and m.open == 1
    assert client.get("/health").json()["level"]["learned_gains_db"] == {"('v.wav', 'hello')": -3.25}     # ... an invalid measure teaches nothing
    r = post("w")
    assert "x-initial-gain-db" not in r.headers
    assert client.get("/health").json()["level"]["learned_gains_db"] == {"('v.wav', 'hello')": -3.25, "('w.wav', '')": -4.5}
    caplog.clear()
    with caplog.at_level("WARNING"):
        create_app(Model(), voices, "v", scheduler="lock", level=-18.0, limiter_db=-1.0)
    assert not any("does not limit" in r.getMessage() for r in caplog.records)
    m2 = Model()
    assert "level" not in TestClient(create_app(m2, voices, "v", scheduler="lock")).get("/health").json() and m2.entered == []
    with pytest.raises(ValueError):
        create_app(Model(), voices, "v", scheduler="lock", level=-3.0)

    # the batch scheduler: the request's entry carries the initial gain and the hook to the worker
    class Worker:
        def __init__(self):
            self.seen = []

        def submit(self, cfg, text):
            import queue
            from fq3hip.server import BatchWorker
            self.seen.append(cfg)
            cfg["on_level"](-7.0 if len(self.seen) == 1 else float("nan"))
            q = queue.Queue()
            q.put(np.zeros(240, dtype=np.float32))
            q.put(BatchWorker.DONE)
            return q

    w = Worker()
    client = TestClient(create_app(Model(), voices, "v", scheduler="batch", worker=w, level=-16.0, limiter_db=-1.0))
    assert client.post("/v1/audio/speech", json={"input": "hi", "voice": "bob", "response_format": "pcm"}).status_code == 200
    r = client.post("/v1/audio/speech", json={"input": "hi", "voice": "bob", "response_format": "pcm"})
    assert "initial_gain_db" not in w.seen[0] and w.seen[1]["initial_gain_db"] == -7.0 and r.headers["x-initial-gain-db"] == "-7.000"
    assert client.get("/health").json()["level"]["learned_gains_db"] == {"('speaker', 'bob')": -7.0}
    a = build_parser().parse_args(["--ref-audio", "x.wav", "--level", "-18", "--scheduler", "batch"])
    assert a.level == -18.0 and build_parser().parse_args(["--ref-audio", "x.wav"]).level is None
    assert build_parser().parse_args(["--ref-audio", "x.wav", "--level", "-18", "--scheduler", "lock"]).scheduler == "lock"
    for bad in (["--level", "-3"], ["--level", "-18", "--loudness", "-18", "--scheduler", "lock"]):
        with pytest.raises(SystemExit):
            main(["--ref-audio", "x.wav"] + bad)
