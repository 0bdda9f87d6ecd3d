"""CPU: the limiter's host side (fq3_limit_design / _count, the argument checks of the C ABI, fq3hip.limiter's validation) and the
properties of the float32 reference tests/_limit_ref.py that the GPU test compares the device against: the peak guarantee, the
untouched stretches, the attack / hold / release sample counts, and the two measured figures -- the detector's under-read and the
reference's own true-peak overshoot -- from which the GPU test's true-peak bound is derived."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _limit_ref as R
from fq3hip import _lib
from fq3hip import limiter as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = R.ONE


# ---- design and count ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,A,H", [(24000, 120, 480), (8000, 40, 160), (44100, 221, 882), (48000, 240, 960)])
def test_design_constants(rate, A, H):
    """5 ms at 44 100 Hz is 220.5 samples: the round goes away from zero, to 221"""
    for db in (-1.0, -6.0, 0.0, -20.0):
        d = M.design(rate, M.LimiterSpec(ceiling_db=db))
        assert (d.A, d.H, d.latency, d.history) == (A, H, A + 6, 2 * A + H + 11)
        assert type(d.c) is np.float32 and abs(float(d.c) - 10.0 ** (db / 20.0)) <= 2.0 ** -24
        assert d.tile % 256 == 0 and 256 <= d.tile <= 4096
    rows = np.array(d.rows, dtype=np.float64)
    assert rows.shape == (3, 12)
    assert np.abs(rows.sum(axis=1) - 1.0).max() <= 12 * 2.0 ** -25          # each row sums to 1 up to the float32 rounding of its taps
    assert np.array_equal(rows[0], rows[2][::-1])                           # phase 1/4 mirrors phase 3/4
    assert np.array_equal(rows[1], rows[1][::-1]) and rows[1][5] == rows[1][6] and rows[0][5] > 0.85
    assert np.array_equal(rows, np.array(M.design(8000).rows, dtype=np.float64))      # the rows do not depend on the rate


def test_design_range_errors_come_without_a_hip_call():
    lib = _lib.load()
    for args in ((7999, -1.0, 5.0, 20.0), (48001, -1.0, 5.0, 20.0), (24000, 0.1, 5.0, 20.0), (24000, -20.1, 5.0, 20.0),
                 (24000, float("nan"), 5.0, 20.0), (24000, -1.0, 0.3, 20.0), (24000, -1.0, 20.1, 20.0), (24000, -1.0, float("nan"), 20.0),
                 (24000, -1.0, 5.0, 80.1), (24000, -1.0, 5.0, -1.0), (8000, -1.0, 0.9, 20.0), (48000, -1.0, 10.1, 20.0)):
        assert lib.fq3_limit_design(*args, None, None, None, None, None) == _lib.FQ3_EINVAL, args
        cfg, h = _lib.LimitConfig(args[0], args[1], args[2], args[3], 0), C.c_void_p()
        assert lib.fq3_limit_create(C.byref(cfg), C.byref(h)) == _lib.FQ3_EINVAL and not h.value, args
        assert lib.fq3_last_error().startswith(b"limit: ")
    for tile in (-256, 128, 300, 4352):
        cfg, h = _lib.LimitConfig(24000, -1.0, 5.0, 20.0, tile), C.c_void_p()
        assert lib.fq3_limit_create(C.byref(cfg), C.byref(h)) == _lib.FQ3_EINVAL and not h.value, tile
    assert lib.fq3_limit_design(24000, -1.0, 5.0, 20.0, None, None, None, None, None) == 0       # every output may be NULL
    assert lib.fq3_limit_count(24000, 5.0, -1, 0) == _lib.FQ3_EINVAL and lib.fq3_limit_count(24000, 5.0, (1 << 31) + 1, 1) == _lib.FQ3_EINVAL
    assert lib.fq3_limit_count(7000, 5.0, 10, 0) == _lib.FQ3_EINVAL
    with pytest.raises(ValueError, match="attack"):
        M.design(8000, M.LimiterSpec(lookahead_ms=0.5))
    with pytest.raises(ValueError, match="outside"):
        M.count(24000, None, -5, False)


def test_null_arguments_through_the_c_abi():
    """answered before any HIP call, so this runs without a GPU; the state error (FQ3_ESTATE after a final push) needs an object and
    is checked on the GPU"""
    lib = _lib.load()
    h, n = C.c_void_p(), C.c_int64()
    cfg = _lib.LimitConfig(24000, -1.0, 5.0, 20.0, 0)
    assert lib.fq3_limit_create(None, C.byref(h)) == _lib.FQ3_EINVAL and lib.fq3_limit_create(C.byref(cfg), None) == _lib.FQ3_EINVAL
    assert lib.fq3_limit_destroy(None) == 0
    assert lib.fq3_limit_reset(None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_limit_push(None, None, 0, 0, None, 0, C.byref(n), None) == _lib.FQ3_EINVAL
    assert lib.fq3_limit_stats(None, None, None) == _lib.FQ3_EINVAL
    assert b"null" in lib.fq3_last_error()


@pytest.mark.parametrize("rate", R.RATES)
def test_count_is_a_non_decreasing_function_of_the_cumulative_length(rate):
    d = M.design(rate)
    ns = list(range(0, d.latency + 40)) + [10 ** 4, 10 ** 6, 1 << 31]
    got = [M.count(rate, None, n, False) for n in ns]
    assert got == [max(0, n - d.A - 6) for n in ns]
    assert all(b >= a for a, b in zip(got, got[1:]))
    assert [M.count(rate, None, n, True) for n in ns] == ns
    assert M.count(rate, M.LimiterSpec(lookahead_ms=10.0), 1000, False) == 1000 - round(rate / 100) - 6


def test_spec_validation():
    for kw in (dict(ceiling_db=0.5), dict(ceiling_db=-21), dict(ceiling_db=None), dict(ceiling_db=True), dict(lookahead_ms=-1),
               dict(hold_ms=float("inf")), dict(hold_ms="20"), dict(lookahead_ms=float("nan"))):
        with pytest.raises(ValueError):
            M.LimiterSpec(**kw)
    s = M.LimiterSpec()
    assert (s.ceiling_db, s.lookahead_ms, s.hold_ms) == (-1.0, 5.0, 20.0)
    with pytest.raises(ValueError, match="GPU"):
        M.Limiter(None, 24000, "cpu")
    with pytest.raises(ValueError, match="LimiterSpec"):
        M.Limiter(-1.0, 24000, "cpu")


# ---- the reference's own properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ceiling_db", R.CEILINGS)
@pytest.mark.parametrize("rate", R.RATES)
def test_reference_keeps_every_sample_under_the_ceiling(rate, ceiling_db):
    d, sig, emu = R.case(rate, ceiling_db)
    lim = float(d.c) * (1.0 + 2.0 ** -22)
    for k, e in emu.items():
        assert np.isfinite(e.y).all() and float(np.abs(e.y).max()) <= lim, k
        assert (e.g <= e.q).all() and (e.g >= 0).all() and (e.g <= ONE).all(), k
    assert float(np.abs(sig["bursts"]).max()) > 3.9 * float(d.c) and emu["bursts"].n_limited > 0        # +12 dB over the ceiling
    assert emu["bad"].n_bad == 3 and emu["bursts"].n_bad == 0
    if ceiling_db == -1.0:
        # the sine's samples never reach the ceiling, its true peak does: a sample-peak limiter would pass it unchanged
        assert float(np.abs(sig["sine"]).max()) < float(d.c) < 1.2 and emu["sine"].n_limited > 0
        assert abs(float(emu["sine"].true_peak) / 1.2 - 1.0) < 0.02


@pytest.mark.parametrize("rate", R.RATES)
def test_reference_passes_untouched_stretches_bit_for_bit(rate):
    d, sig, emu = R.case(rate, -1.0)
    q = emu["quiet"]
    assert q.n_limited == 0 and q.min_gain_q23 == ONE and q.y.tobytes() == sig["quiet"].tobytes()
    assert float(q.true_peak) < float(d.c)
    x, e = sig["bursts"], emu["bursts"]
    over = np.concatenate([np.zeros(d.A + d.H, bool), e.q < ONE, np.zeros(d.A, bool)])
    touched = np.lib.stride_tricks.sliding_window_view(over, 2 * d.A + d.H + 1).any(axis=1)      # some over in [i - A - H, i + A]
    assert len(touched) == len(x) and 0 < (~touched).sum() < len(x)
    assert np.array_equal(e.g < ONE, touched)
    assert x[~touched].tobytes() == e.y[~touched].tobytes()


@pytest.mark.parametrize("rate", R.RATES)
def test_reference_attack_hold_and_release_counts(rate):
    """one sample 5 % over the ceiling at k, nothing else: the gain is 1 up to k - A - 1, falls strictly over the A samples in front
    of k, sits at q[k] on [k, k + H], climbs strictly over the next A samples and is 1 from k + A + H + 1 on"""
    d = M.design(rate)
    A, H, k = d.A, d.H, 3000
    x = np.zeros(k + 2 * (A + H) + 500, np.float32)
    x[k] = np.float32(1.05) * d.c
    e = R.emulate(x, d)
    assert (e.q < ONE).sum() == 1 and e.q[k] < ONE
    g = e.g
    assert (g[:k - A] == ONE).all() and (g[k + A + H + 1:] == ONE).all()
    assert (np.diff(g[k - A - 1:k + 1]) < 0).all() and g[k - A] < ONE
    assert (g[k:k + H + 1] == e.q[k]).all()
    assert (np.diff(g[k + H:k + A + H + 2]) > 0).all() and g[k + A + H] < ONE
    assert e.n_limited == 2 * A + H + 1
    assert abs(float(e.y[k])) <= float(d.c) * (1 + 2.0 ** -22)


# ---- the measured figures --------------------------------------------------------------------------------------------------------------
def test_yardstick_reads_a_known_true_peak():
    i = np.arange(4000)
    for amp, f in ((1.2, 0.25), (0.7, 0.11), (1.0, 0.37)):
        x = amp * np.sin(2 * np.pi * f * i + np.pi / 4) * np.minimum(1.0, np.minimum(i, i[::-1]) / 500.0)      # faded in and out
        assert abs(R.true_peak64(x) / amp - 1.0) < 2e-3


def test_under_read_and_overshoot_are_the_recorded_ones():
    """The detector reads a waveform's peak at four points per sample, so it reads low; the reference's output therefore overshoots c
    a little when read by the yardstick, and gain modulation can add to that.  Neither figure is fixed in advance: they are measured
    here, recorded in profiles/limiter_stage.json and quoted in DESIGN.md section 4.16, and the GPU test's true-peak bound is
    c (1 + 1.05 (worst overshoot - 1))."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "limiter_stage.json")))["detector"]
    worst_u = worst_o = 0.0
    for rate in R.RATES:
        for db in R.CEILINGS:
            for k, v in R.measured(rate, db).items():
                print(f"{rate} Hz {db:+.0f} dB {k}: under-read {v['under_read']:.4f}, output overshoot {v['overshoot']:.4f}")
                worst_u, worst_o = max(worst_u, v["under_read"]), max(worst_o, v["overshoot"])
                assert np.isfinite(v["under_read"]) and np.isfinite(v["overshoot"])
            assert R.true_peak_bound(rate, db) >= float(R.case(rate, db)[0].c)
    print(f"worst under-read {worst_u:.4f}, worst overshoot {worst_o:.4f}")
    assert abs(worst_u / rec["worst_under_read"] - 1.0) < 1e-4 and abs(worst_o / rec["worst_overshoot"] - 1.0) < 1e-4
    # the sine (in_rate / 4, true peak 1.2 between its samples) is read to within 0.1 %; full-band noise bursts are the hard case
    assert all(abs(R.measured(rate, -1.0)["sine"]["under_read"] - 1.0) < 2e-3 for rate in R.RATES)


# ---- the model's context, the command line and the server (no GPU) ---------------------------------------------------------------------
def test_model_context_validates_and_composes():
    from fq3hip.model import FasterQwen3TTS
    m = FasterQwen3TTS.__new__(FasterQwen3TTS)
    m.sample_rate, m.device, m._audio_spec, m._loud, m._gain = 24000, "cuda:0", None, None, None
    assert not m._levelling() and m._gain_kw() == {}
    for kw in (dict(ceiling_db=1.0), dict(ceiling_db=-25.0), dict(lookahead_ms=0.1), dict(lookahead_ms=25.0), dict(hold_ms=100.0)):
        with pytest.raises(ValueError):
            with m.limiter(**kw):
                pass
    with m.limiter(-3.0) as spec:
        assert spec == M.LimiterSpec(-3.0, 5.0, 20.0) and m._limit is spec and m._levelling()
        assert m._gain_kw() == dict(limiter=spec, limiter_pool=[]) and m._gain_kw()["limiter_pool"] is m._limiter_pools[spec]
        with m.fixed_gain(6.0):                                      # composes with fixed_gain, either way round
            assert m._gain is not None and m._limit is spec
        with m.loudness(-20.0):                                      # and with loudness(), where loudness() is allowed ...
            with pytest.raises(ValueError, match="fixed_gain"):      # ... which still is not on a stream
                m.streaming_vocoder(None, 12)
        with m.limiter(-9.0) as inner:
            assert m._limit is inner
        assert m._limit is spec
    assert m._limit is None and not m._levelling()
    with m.fixed_gain(6.0), m.limiter():
        assert m._limit == M.LimiterSpec() and m._gain is not None
    assert "limiter()" in FasterQwen3TTS.fixed_gain.__doc__ and "There is no limiter" not in FasterQwen3TTS.fixed_gain.__doc__


def test_cli_flag():
    from fq3hip import cli
    p = cli.build_parser()
    base = ["custom", "--speaker", "bob", "--output", "o.wav", "--text", "hi"]
    for extra in ([], ["--streaming"], ["--long"], ["--gain-db", "12"], ["--loudness", "-18"]):
        a = p.parse_args(base + extra + ["--limiter-db", "-2"])
        assert a.limiter_db == -2.0
        cli.check_level_args(p, a)
    assert p.parse_args(["serve", "--limiter-db", "-1"]).limiter_db == -1.0
    assert p.parse_args(base).limiter_db is None
    for bad in ("1", "-21", "nan"):
        with pytest.raises(SystemExit):
            cli.check_level_args(p, p.parse_args(base + ["--limiter-db", bad]))

    class Fake:
        def __init__(self):
            self.seen = []

        def _ctx(self, *what):
            import contextlib
            self.seen.append(what)
            return contextlib.nullcontext()

        def loudness(self, **kw):
            return self._ctx("loudness", kw)

        def fixed_gain(self, g):
            return self._ctx("fixed_gain", g)

        def limiter(self, **kw):
            return self._ctx("limiter", kw)

    f = Fake()
    with cli._levelled(f, p.parse_args(base + ["--gain-db", "4", "--limiter-db", "-2"])):
        pass
    with cli._levelled(f, p.parse_args(base + ["--limiter-db", "-6"])):
        pass
    with cli._levelled(f, p.parse_args(base)):
        pass
    assert f.seen == [("fixed_gain", 4.0), ("limiter", dict(ceiling_db=-2.0)), ("limiter", dict(ceiling_db=-6.0))]


def test_server_flag():
    import contextlib
    from fastapi.testclient import TestClient
    from fq3hip.server import build_parser, create_app, main

    class Model:
        sample_rate = 24000

        def __init__(self):
            self.entered, self.open = [], 0

        @contextlib.contextmanager
        def limiter(self, ceiling_db=-1.0):
            spec = M.LimiterSpec(ceiling_db, 4.0, 30.0)            # not the defaults: /health must report what the context yields
            self.entered.append(ceiling_db)
            self.open += 1
            try:
                yield spec
            finally:
                self.open -= 1

        def generate_voice_clone_streaming(self, **kw):
            yield np.zeros(240, dtype=np.float32), 24000, {}

    voices = {"v": {"ref_audio": "v.wav"}}
    m = Model()
    client = TestClient(create_app(m, voices, "v", scheduler="lock", limiter_db=-2.0))
    assert m.entered == [-2.0] and m.open == 1                       # entered once, for the life of the app
    assert client.get("/health").json()["limiter"] == {"ceiling_db": -2.0, "lookahead_ms": 4.0, "hold_ms": 30.0}
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "v", "response_format": "pcm"})
    assert r.status_code == 200 and len(r.content) == 480
    m2 = Model()
    assert "limiter" not in TestClient(create_app(m2, voices, "v", scheduler="lock")).get("/health").json() and m2.entered == []
    with pytest.raises(ValueError):
        create_app(Model(), voices, "v", scheduler="lock", limiter_db=3.0)
    a = build_parser().parse_args(["--ref-audio", "x.wav", "--limiter-db", "-1.5", "--scheduler", "batch"])
    assert a.limiter_db == -1.5 and build_parser().parse_args(["--ref-audio", "x.wav"]).limiter_db is None
    with pytest.raises(SystemExit):
        main(["--ref-audio", "x.wav", "--limiter-db", "2"])
