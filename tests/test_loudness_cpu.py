"""CPU: the loudness stage's host half (fq3_loud_design behind fq3hip/loudness.py) and its reference
(tests/_loud_ref.py): the K-weighting design against the BS.1770-4 table, range errors without a HIP call, a sine anchor for the
float64 measure, the integer gating and the gain on hand-made hop arrays, the GPU tests' signal, and the validation of the spec and
of the model's contexts."""
import ctypes as C
import math

import numpy as np
import pytest

import _loud_ref as R
from fq3hip import _lib
from fq3hip import loudness as L


def test_design_48k_equals_the_standard_table():
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
            1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    d = L.design(48000)
    assert d.H == 4800
    assert np.abs(np.array(d.coef64) - want).max() <= 1e-12
    sb, sa, hb, ha = R.design64(48000)
    assert np.abs(np.array(sb + sa[1:] + hb + ha[1:]) - want).max() <= 1e-12
    assert all(np.float32(a) == b for a, b in zip(d.coef64, d.coef32)) and all(isinstance(v, np.float32) for v in d.coef32)


@pytest.mark.parametrize("rate", [8000, 16000, 24000, 44100])
def test_design_constants(rate):
    spec = L.LoudnessSpec(-23.0, -2.0, 12.0)
    d = L.design(rate, spec)
    H = rate // 10
    assert d.H == H
    sb, sa, hb, ha = R.design64(rate)
    assert np.abs(np.array(d.coef64) - np.array(sb + sa[1:] + hb + ha[1:])).max() <= 1e-14      # libm against Python: an ulp or two
    gate = 10.0 ** ((-70 + 0.691) / 10) * 4 * H * 2.0 ** 40
    assert abs(d.abs_gate - gate) <= 1 + 1e-12 * gate
    assert d.target_power == pytest.approx(10 ** ((-23 + 0.691) / 10), rel=1e-14)
    assert d.ceiling == pytest.approx(10 ** (-2 / 20), rel=1e-14) and d.max_gain == pytest.approx(10 ** (12 / 20), rel=1e-14)


def test_design_range_errors_come_without_a_hip_call():
    lib = _lib.load()
    ok = (24000, -16.0, -1.0, 20.0)
    bad = [(7900, -16.0, -1.0, 20.0), (48100, -16.0, -1.0, 20.0), (24050, -16.0, -1.0, 20.0), (24000, -40.5, -1.0, 20.0),
           (24000, -4.0, -1.0, 20.0), (24000, -16.0, 0.5, 20.0), (24000, -16.0, -21.0, 20.0), (24000, -16.0, -1.0, -1.0),
           (24000, -16.0, -1.0, 41.0), (24000, float("nan"), -1.0, 20.0)]
    none = [None] * 7
    assert lib.fq3_loud_design(*ok, *none) == 0                    # every output pointer may be NULL
    for args in bad:
        assert lib.fq3_loud_design(*args, *none) == _lib.FQ3_EINVAL, args
        assert b"loud" in lib.fq3_last_error()
    # the object calls: NULL and range errors before any HIP call (no GPU here)
    h = C.c_void_p()
    assert lib.fq3_loud_create(None, C.byref(h)) == _lib.FQ3_EINVAL
    for cfg in (_lib.LoudConfig(22050, -16.0, -1.0, 20.0, 0), _lib.LoudConfig(24000, -50.0, -1.0, 20.0, 0),
                _lib.LoudConfig(24000, -16.0, -1.0, 20.0, -1), _lib.LoudConfig(24000, -16.0, -1.0, 20.0, (1 << 20) + 1)):
        assert lib.fq3_loud_create(C.byref(cfg), C.byref(h)) == _lib.FQ3_EINVAL and not h.value
    assert lib.fq3_loud_destroy(None) == 0
    assert lib.fq3_loud_reset(None, None) == _lib.FQ3_EINVAL and lib.fq3_loud_push(None, None, 0, 0, None) == _lib.FQ3_EINVAL
    assert lib.fq3_loud_finish(None, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_loud_hops(None, None, 0, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_loud_apply(None, None, 0, None, None) == _lib.FQ3_EINVAL
    g = C.c_float(1.0)
    assert lib.fq3_loud_apply(C.byref(g), None, -1, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_loud_apply(C.byref(g), None, 5, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_loud_apply(C.byref(g), None, 0, None, None) == 0          # n = 0 launches nothing
    with pytest.raises(ValueError, match="multiple of 100"):
        L.design(22050)
    assert C.sizeof(_lib.LoudStats) == 40 and _lib.LoudStats.gain.offset == 12 and C.sizeof(_lib.LoudConfig) == 40


@pytest.mark.parametrize("rate,tol", [(48000, 0.001), (24000, 0.05), (8000, 0.05)])
def test_sine_anchor(rate, tol):
    """A 997 Hz sine of amplitude 0.5 reads 20 log10(0.5) - 3.01 LUFS: exact at 48 kHz, where the design is the standard's table; the
    re-designed filters at lower rates are warped by a few hundredths of an LU (a sanity anchor, not a precision claim)."""
    t = np.arange(5 * rate) / rate
    got = R.measure64(0.5 * np.sin(2 * np.pi * 997 * t), rate)
    print(f"{rate} Hz: {got:.5f} LUFS, off by {got - (20 * math.log10(0.5) - 3.01):+.5f}")
    assert abs(got - (20 * math.log10(0.5) - 3.01)) <= tol


def _hops(d, lufs_per_hop):
    """hop integers whose blocks sit at the given loudness"""
    return [int(10 ** ((v + 0.691) / 10) * d.H * R.SCALE) if v is not None else 0 for v in lufs_per_hop]


def test_gating_absolute_gate_alone():
    d = L.design(24000, L.LoudnessSpec(-16.0, 0.0, 40.0))
    E = _hops(d, [-20.0] * 10 + [None] * 6 + [-80.0] * 6)
    g = R.gate(E, np.float32(0.01), 0, d)
    # blocks 0..6 are whole; 7, 8, 9 hold 3, 2, 1 loud hops: -21.2, -23, -26 LUFS, all above the relative gate at about -31
    assert (g["n_hops"], g["n_abs"], g["n_rel"], g["valid"]) == (22, 10, 10, 1)
    B = [sum(E[b:b + 4]) for b in range(len(E) - 3)]
    kept = [v for v in B if v > d.abs_gate]
    assert len(kept) == 10
    assert g["mean_power"] == pytest.approx(sum(kept) / (10 * 4 * d.H * R.SCALE), rel=1e-15)
    assert float(g["gain"]) == pytest.approx(math.sqrt(d.target_power / g["mean_power"]), rel=1e-7)
    # the two-half sum is the correctly rounded double of the exact integer
    assert R._split_sum(kept) == float(sum(kept))
    big = [(1 << 60) + 12345, (1 << 60) + 99999, (1 << 59) + 7] * 1000
    assert R._split_sum(big) == float(sum(big))


def test_gating_relative_gate_drops_a_block():
    d = L.design(24000, L.LoudnessSpec(-16.0, 0.0, 40.0))
    E = _hops(d, [-20.0] * 12 + [None] * 4 + [-45.0] * 8)
    g = R.gate(E, np.float32(0.01), 0, d)
    B = [sum(E[b:b + 4]) for b in range(len(E) - 3)]
    g1 = [v for v in B if v > d.abs_gate]
    thr = sum(g1) / len(g1) / 10
    g2 = [v for v in g1 if v > thr]
    assert 0 < len(g2) < len(g1) == g["n_abs"] and g["n_rel"] == len(g2)
    assert g["mean_power"] == pytest.approx(sum(g2) / (len(g2) * 4 * d.H * R.SCALE), rel=1e-15)
    assert R.lufs_of(g["mean_power"]) > R.lufs_of(sum(g1) / (len(g1) * 4 * d.H * R.SCALE))


def test_gating_invalid_results():
    d = L.design(24000)
    for E in ([], _hops(d, [-20.0] * 3)):
        g = R.gate(E, np.float32(0.5), 0, d)
        assert (g["valid"], float(g["gain"]), g["n_abs"], g["n_hops"]) == (0, 1.0, 0, len(E))
    g = R.gate(_hops(d, [-90.0] * 8), np.float32(0.5), 0, d)        # nothing above the absolute gate
    assert (g["valid"], float(g["gain"]), g["n_abs"]) == (0, 1.0, 0)
    g = R.gate(_hops(d, [-20.0] * 8), np.float32(0.5), 1, d)        # a non-finite sample
    assert (g["valid"], float(g["gain"]), g["n_bad"]) == (0, 1.0, 1)


def test_gain_clamps():
    E = _hops(L.design(24000), [-30.0] * 8)
    free = R.gate(E, np.float32(0.05), 0, L.design(24000, L.LoudnessSpec(-16.0, 0.0, 40.0)))
    assert 20 * math.log10(float(free["gain"])) == pytest.approx(14.0, abs=1e-3)
    d = L.design(24000, L.LoudnessSpec(-16.0, -1.0, 40.0))
    ceil = R.gate(E, np.float32(0.5), 0, d)                          # +14 dB would put the peak at +8 dBFS
    assert ceil["gain"] == np.float32(d.ceiling / 0.5) and ceil["valid"] == 1
    d = L.design(24000, L.LoudnessSpec(-16.0, 0.0, 6.0))
    capped = R.gate(E, np.float32(0.05), 0, d)
    assert capped["gain"] == np.float32(d.max_gain)
    zero_peak = R.gate(E, np.float32(0.0), 0, d)                     # (a peak of 0 does not divide)
    assert zero_peak["gain"] == np.float32(d.max_gain)


def test_emulation_follows_the_float64_measure():
    """The float32 emulation of the contract (per-hop restart, integer energies) against the true recursive float64 filter, on the GPU
    tests' signal: the restart and float32 together stay within 1e-3 of every sounding hop's energy."""
    rate = 8000
    d = L.design(rate)
    x = R.burst_signal(rate)
    e32 = R.emulate_hops(x, d.coef32, d.H).astype(np.float64) / R.SCALE
    e64 = R.hop_energies64(x, rate)
    assert len(e32) == len(e64) == 70
    loud = e64 >= R.ABS_GATE_POWER * d.H
    assert loud.sum() >= 0.75 * len(e64)
    assert (np.abs(e32 - e64)[loud] / e64[loud]).max() <= 1e-3
    assert np.abs(e32 - e64)[~loud].max() <= 1e-3 * R.ABS_GATE_POWER * d.H
    # the emulation's gating reads what the float64 measure reads
    pk, nb = R.peak_and_bad(x)
    g = R.gate(R.emulate_hops(x, d.coef32, d.H), pk, nb, d)
    assert g["valid"] == 1 and abs(R.lufs_of(g["mean_power"]) - R.measure64(x, rate)) <= 0.001


@pytest.mark.parametrize("rate", [24000, 8000])
def test_burst_signal_keeps_its_gate_sets_under_a_uniform_gain(rate):
    """What the GPU tests rely on.  A uniform gain moves every block and the relative threshold alike, so only the ABSOLUTE gate can
    change hands: no block of the signal lies within 20 dB of it (the range of gains the tests apply).  The relative gate drops the
    quiet burst by more than 3 dB and keeps every other block by more than 3 dB -- thousands of times what float32 moves a block."""
    x = R.burst_signal(rate)
    z = R.block_levels64(x, rate)
    db = 10 * np.log10(np.maximum(z, 1e-40) / R.ABS_GATE_POWER)
    assert np.abs(db).min() > 20.0
    g1 = z[z > R.ABS_GATE_POWER]
    rel = 10 * np.log10(g1 / (0.1 * g1.mean()))
    assert np.abs(rel).min() > 3.0
    assert 0 < (rel > 0).sum() < len(g1) < len(z)                   # both gates drop blocks
    H = rate // 10
    for h0, n, _rel in R.BURSTS[:-1]:                               # exact zeros, at least 5 hops, between the bursts
        nxt = min(b[0] for b in R.BURSTS if b[0] > h0)
        assert nxt - (h0 + n) >= 5 and not x[(h0 + n) * H: nxt * H].any()
    assert len(x) % H != 0 and len(x) // H == 70


def test_spec_validation():
    assert L.LoudnessSpec() == L.LoudnessSpec(-16.0, -1.0, 20.0)
    for kw in (dict(target_lufs=-41), dict(target_lufs=-4.9), dict(ceiling_db=0.1), dict(ceiling_db=-20.5), dict(max_gain_db=-0.1),
               dict(max_gain_db=40.5), dict(target_lufs="loud"), dict(target_lufs=True), dict(ceiling_db=float("nan")),
               dict(max_gain_db=None)):
        with pytest.raises(ValueError):
            L.LoudnessSpec(**kw)
    assert L.gain_factor(-6.0) == 10 ** (-6.0 / 20) and L.gain_factor(0) == 1.0
    for bad in (41, -61, float("inf"), "3", None, True):
        with pytest.raises(ValueError):
            L.gain_factor(bad)
    st = L.LoudnessStats.from_bytes(bytes(_lib.LoudStats(0.01, 0.5, 2.0, 50, 40, 30, 0, 1, 0)))
    assert st.lufs == pytest.approx(-20.691) and st.peak_db == pytest.approx(-6.0206, abs=1e-4) and st.gain_db == pytest.approx(6.0206, abs=1e-4)
    assert (st.valid, st.n_hops, st.n_abs, st.n_rel, st.n_bad) == (True, 50, 40, 30, 0)
    assert L.LoudnessStats.from_bytes(bytes(_lib.LoudStats(0.0, 0.0, 1.0, 2, 0, 0, 0, 0, 0))).lufs == float("-inf")


def test_model_contexts_validate_and_refuse_streaming():
    """The contexts on a model that has no GPU behind it: argument errors on entry, the two do not nest, every streaming path refuses
    inside ``loudness`` with a pointer to ``fixed_gain``, and leaving a context restores what was there."""
    from fq3hip.model import FasterQwen3TTS
    m = FasterQwen3TTS.__new__(FasterQwen3TTS)
    m.sample_rate, m.device, m._audio_spec, m._loud, m._gain = 24000, "cuda:0", None, None, None
    with pytest.raises(ValueError):
        with m.loudness(target_lufs=-3.0):
            pass
    with pytest.raises(ValueError):
        with m.fixed_gain(90.0):
            pass
    with m.loudness(-20.0) as sess:
        assert sess.spec == L.LoudnessSpec(-20.0, -1.0, 20.0) and m._loud is sess and sess.stats == []
        with pytest.raises(ValueError, match="loudness"):
            with m.fixed_gain(-6.0):
                pass
        for make in (lambda: m._run_streaming(*[None] * 9, 12), lambda: m._run_text_streaming(["x"], None, {}, 12),
                     lambda: m._run_batch_streaming([], {}, 12, 2), lambda: m._run_long_streaming([], [], None, {}, 12, 2)):
            with pytest.raises(ValueError, match="fixed_gain"):
                next(make())
        with pytest.raises(ValueError, match="fixed_gain"):
            m.streaming_vocoder(None, 12)
    assert m._loud is None
    with m.fixed_gain(-6.0) as factor:
        assert factor == float(np.float32(10 ** (-6.0 / 20))) and m._gain["gain_db"] == -6.0
        with pytest.raises(ValueError, match="fixed_gain"):
            with m.loudness():
                pass
    assert m._gain is None and m._gain_kw() == {} and not m._levelling()
    m.sample_rate = 22050                                        # a rate the meter refuses: said on entry
    with pytest.raises(ValueError, match="multiple of 100"):
        with m.loudness():
            pass


# ---- the command line and the server (no GPU: a stand-in model) ----------------------------------------------------------------------
def test_cli_flags():
    from fq3hip import cli
    p = cli.build_parser()
    base = ["custom", "--speaker", "bob", "--output", "o.wav"]
    a = p.parse_args(base + ["--text", "hi", "--loudness", "-18", "--long"])
    assert a.loudness == -18.0 and a.gain_db is None
    cli.check_level_args(p, a)
    a = p.parse_args(base + ["--text", "hi", "--gain-db", "-3.5", "--streaming"])
    assert a.gain_db == -3.5 and a.loudness is None
    cli.check_level_args(p, a)
    assert p.parse_args(["serve", "--gain-db", "2"]).gain_db == 2.0
    for extra in (["--text", "hi", "--loudness", "-18", "--streaming"], ["--text-stdin", "--loudness", "-18"],
                  ["--text", "hi", "--loudness", "-18", "--gain-db", "1"]):
        with pytest.raises(SystemExit):
            cli.check_level_args(p, p.parse_args(base + extra))
    for extra in (["--text", "hi", "--loudness", "-2"], ["--text", "hi", "--gain-db", "55"], ["--text", "hi", "--gain-db", "nan"]):
        with pytest.raises(SystemExit):                         # out of range: an argparse error, not a traceback behind the model load
            cli.check_level_args(p, p.parse_args(base + extra))
    with pytest.raises(SystemExit):
        cli.check_level_args(p, p.parse_args(["serve", "--gain-db", "-70"]))
    with pytest.raises(SystemExit):
        p.parse_args(["serve", "--loudness", "-18"])             # `serve` writes line by line; it takes --gain-db only

    class Fake:
        def __init__(self):
            self.seen = []

        def loudness(self, **kw):
            self.seen.append(("loudness", kw))
            import contextlib
            return contextlib.nullcontext()

        def fixed_gain(self, g):
            self.seen.append(("fixed_gain", g))
            import contextlib
            return contextlib.nullcontext()

    f = Fake()
    cli._levelled(f, p.parse_args(base + ["--text", "hi", "--loudness", "-18"]))
    cli._levelled(f, p.parse_args(base + ["--text", "hi", "--gain-db", "4"]))
    cli._levelled(f, p.parse_args(base + ["--text", "hi"]))
    assert f.seen == [("loudness", dict(target_lufs=-18.0)), ("fixed_gain", 4.0)]


class _FakeServerModel:
    """what the lock scheduler touches, with a voice "quiet" whose calibration reads -36 LUFS and a voice "mute" that cannot be measured"""
    sample_rate = 24000

    def __init__(self):
        import contextlib
        self.ctx, self.gains, self.seeds = contextlib, [], []

    def seeded(self, seed):
        self.seeds.append(seed)
        return self.ctx.nullcontext()

    def fixed_gain(self, g):
        self.gains.append(g)
        return self.ctx.nullcontext()

    def generate_voice_clone(self, text, ref_audio=None, **kw):
        self.cal_text = text
        return [np.full(4, 1.0 if ref_audio == "quiet.wav" else 0.0, dtype=np.float32)], 24000

    def measure_loudness(self, wav, spec):
        ok = bool(wav[0])
        raw = bytes(_lib.LoudStats(10 ** ((-36 + 0.691) / 10) if ok else 0.0, 0.1, 10 ** ((spec.target_lufs + 36) / 20) if ok else 1.0,
                                   30, 27 if ok else 0, 27 if ok else 0, 0, int(ok), 0))
        return L.LoudnessStats.from_bytes(raw)

    def generate_voice_clone_streaming(self, **kw):
        yield np.zeros(240, dtype=np.float32), 24000, {}


def test_server_calibrates_voices_and_streams_with_their_gain():
    from fastapi.testclient import TestClient
    from fq3hip.server import build_parser, create_app, main
    voices = {"quiet": {"ref_audio": "quiet.wav"}, "mute": {"ref_audio": "mute.wav"}}
    m = _FakeServerModel()
    with pytest.raises(ValueError, match="lock scheduler"):
        create_app(m, voices, "quiet", scheduler="batch", worker=object(), loudness=-20.0)
    with pytest.raises(ValueError):
        create_app(m, voices, "quiet", scheduler="lock", loudness=-2.0)           # the spec's range
    app = create_app(m, voices, "quiet", scheduler="lock", loudness=-20.0, loudness_text="calibrate me")
    assert m.seeds == [0, 0] and m.cal_text == "calibrate me"
    client = TestClient(app)
    h = client.get("/health").json()["loudness"]
    assert h["target_lufs"] == -20.0
    assert h["voices"]["quiet"] == {"gain_db": 16.0, "lufs": -36.0, "calibrated": True}
    assert h["voices"]["mute"] == {"gain_db": 0.0, "lufs": None, "calibrated": False}
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "quiet", "response_format": "pcm"})
    assert r.status_code == 200 and r.headers["X-Gain-Db"] == "16.000" and m.gains == [16.0] and len(r.content) == 480
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "mute", "response_format": "pcm"})
    assert r.headers["X-Gain-Db"] == "0.000" and m.gains == [16.0, 0.0]
    # without the flag: no calibration, no header, no context
    m2 = _FakeServerModel()
    c2 = TestClient(create_app(m2, voices, "quiet", scheduler="lock"))
    r = c2.post("/v1/audio/speech", json={"input": "hello", "voice": "quiet", "response_format": "pcm"})
    assert "X-Gain-Db" not in r.headers and m2.gains == [] and m2.seeds == [] and "loudness" not in c2.get("/health").json()
    a = build_parser().parse_args(["--ref-audio", "x.wav", "--loudness", "-18", "--scheduler", "lock"])
    assert a.loudness == -18.0 and "fox" in a.loudness_text
    with pytest.raises(SystemExit):
        main(["--ref-audio", "x.wav", "--loudness", "-18", "--scheduler", "batch"])
