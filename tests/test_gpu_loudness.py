"""GPU: the loudness stage (csrc/loud_kernels.cuh behind fq3_loud_*) against tests/_loud_ref.py: hop energies
against the float64 measure, independence of the cuts bit for bit, the gating and the gain teacher-forced with the device's own
integers, the gain multiply, the whole chain end to end, and the model's ``loudness`` / ``fixed_gain`` contexts."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _join_ref as J
import _loud_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao
from fq3hip import loudness as L

RATES = (24000, 8000)
# (a) and (b) also at 44.1 kHz: H = 4410 is no multiple of the kernel's 32-step tile, so every phase ends in a short tile
RATES_TILES = RATES + (44100,)


@functools.lru_cache(maxsize=None)
def _sig(rate):
    """the burst signal (70 hops and a partial one: two workgroups of the push kernel, the second one partly filled), read-only"""
    x = R.burst_signal(rate)
    x.setflags(write=False)
    return x


def _raw(meter):
    """(hop integers, the 40 stats bytes) of a finished meter"""
    return meter.hops(), meter.finish().cpu().numpy().tobytes()


def _measure(x, rate, spec=None, cuts=None):
    """a fresh meter over ``x`` pushed in the pieces ``cuts`` (ascending positions) delimit -> (hops, stats bytes)"""
    m = L.LoudnessMeter(spec, rate, "cuda")
    xd = torch.from_numpy(np.array(x)).cuda()
    edges = [0] + list(cuts or []) + [len(x)]
    for i in range(len(edges) - 1):
        m.push(xd[edges[i]:edges[i + 1]], final=i == len(edges) - 2)
    return _raw(m)


# ---- (a) hop energies against the float64 reference --------------------------------------------------------------------------------
def _hop_errors(e, e64, floor):
    """per hop: relative error where the reference is at or above ``floor``, else the absolute error as a fraction of ``floor``"""
    loud = e64 >= floor
    return np.where(loud, np.abs(e - e64) / np.maximum(e64, floor), np.abs(e - e64) / floor), loud


@pytest.mark.parametrize("rate", RATES_TILES)
def test_hop_energies_against_float64(rate):
    x, d = _sig(rate), L.design(rate)
    e64 = R.hop_energies64(x, rate)
    floor = R.ABS_GATE_POWER * d.H
    emu, loud = _hop_errors(R.emulate_hops(x, d.coef32, d.H).astype(np.float64) / R.SCALE, e64, floor)
    assert loud.mean() >= 0.75                                      # a condition on the signal
    hops, _ = _measure(x, rate)
    assert len(hops) == len(e64) == 70
    dev, _ = _hop_errors(hops.astype(np.float64) / R.SCALE, e64, floor)
    print(f"{rate} Hz: worst hop error device {dev.max():.3e}, float32 emulation {emu.max():.3e}, bound {4 * emu.max():.3e}")
    assert emu.max() > 0 and dev.max() <= 4 * emu.max()


# ---- (b) cut independence, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES_TILES)
def test_cut_independence(rate):
    x, H = _sig(rate), rate // 10
    n = len(x)
    want = _measure(x, rate)
    rng = np.random.default_rng(11)
    rnd = sorted(int(v) for v in rng.integers(0, n + 1, 36))
    rnd = sorted(rnd + [rnd[5], rnd[5], rnd[20], 3 * H + 17, 3 * H + 18, 0, n])       # empty pushes (also first and last), a 1-sample push
    plans = {"hops": list(range(H, n, H)), "hops+1": list(range(H + 1, n, H)), "hops-1": list(range(H - 1, n, H)),
             "two hops and a half": list(range(5 * H // 2, n, 5 * H // 2)), "random": rnd}
    assert len(rnd) >= 40
    for name, cuts in plans.items():
        hops, raw = _measure(x, rate, cuts=cuts)
        assert np.array_equal(hops, want[0]), name
        assert raw == want[1], name
    st = L.LoudnessStats.from_bytes(want[1])
    assert st.valid and np.float32(st.peak) == R.peak_and_bad(x)[0] and st.n_hops == 70


# ---- (c) teacher-forced gating -----------------------------------------------------------------------------------------------------
def _cases(rate):
    x = _sig(rate)
    nan = x.copy()
    nan[len(x) // 3] = np.nan
    return {"burst": (x, L.LoudnessSpec()), "ceiling": (x, L.LoudnessSpec(-5.0, -6.0, 40.0)),
            "max gain": (x * np.float32(0.01), L.LoudnessSpec()), "short": (x[:3 * rate // 10 + 5], L.LoudnessSpec()),
            "nan": (nan, L.LoudnessSpec())}


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("case", ["burst", "ceiling", "max gain", "short", "nan"])
def test_gating_teacher_forced(rate, case):
    x, spec = _cases(rate)[case]
    d = L.design(rate, spec)
    hops, raw = _measure(x, rate, spec)
    s = _lib.LoudStats.from_buffer_copy(raw)
    pk, nb = R.peak_and_bad(x)
    assert np.float32(s.peak) == pk and s.n_bad == nb
    g = R.gate(hops, np.float32(s.peak), s.n_bad, d)
    got = dict(mean_power=s.mean_power, gain=np.float32(s.gain), n_hops=s.n_hops, n_abs=s.n_abs, n_rel=s.n_rel, n_bad=s.n_bad, valid=s.valid)
    for k, v in got.items():                                       # bit for bit: the double, the float and every count
        assert type(v) is type(g[k]) and np.asarray(v).tobytes() == np.asarray(g[k]).tobytes(), (k, v, g[k])
    if case == "burst":
        assert s.valid and 0 < s.n_rel < s.n_abs < s.n_hops - 3 and s.gain < d.max_gain and s.gain * pk < d.ceiling
    elif case == "ceiling":
        assert s.valid and np.float32(s.gain) == np.float32(d.ceiling / float(pk))
    elif case == "max gain":
        assert s.valid and np.float32(s.gain) == np.float32(d.max_gain)
    elif case == "short":
        assert not s.valid and s.n_hops == 3 and s.gain == 1.0
    else:
        assert not s.valid and s.n_bad == 1 and s.gain == 1.0


def test_state_errors():
    lib = _lib.load()
    m = L.LoudnessMeter(None, 24000, "cuda", capacity_hops=2)
    x = torch.zeros(2400 * 3, device="cuda")
    buf = torch.empty(L.STATS_BYTES, dtype=torch.uint8, device="cuda")
    assert lib.fq3_loud_finish(m._h, C.c_void_p(buf.data_ptr()), None) == _lib.FQ3_ESTATE          # no final push yet
    with pytest.raises(RuntimeError):                               # three hops into room for two: FQ3_ETOOLONG, nothing changed
        m.push(x)
    m.push(x[:4800 + 7], final=True)
    assert m.n_in == 4807 and len(m.hops()) == 2
    with pytest.raises(_lib.Fq3Error) as e:
        m.push(x[:10])
    assert e.value.code == _lib.FQ3_ESTATE
    assert not m.stats().valid and m.stats().n_hops == 2
    m.reset()
    m.push(x[:100], final=True)
    assert m.stats().n_hops == 0 and m.stats().gain == 1.0


# ---- (d) fq3_loud_apply --------------------------------------------------------------------------------------------------------------
def test_apply_is_numpy_float32_multiply():
    rng = np.random.default_rng(3)
    g = np.float32(0.7345678)
    gd = torch.tensor([float(g)], dtype=torch.float32, device="cuda")
    base = rng.standard_normal(20011).astype(np.float32)
    for n in (0, 1, 2, 7, 1023, 10007):
        for so, do in ((0, 0), (1, 1), (1, 5), (1, 2), (3, 0)):     # element offsets: aligned, odd and equal modulo 4, unequal
            src = torch.from_numpy(base).cuda()
            dst = torch.full((n + 16,), -7.0, dtype=torch.float32, device="cuda")
            out = L.apply_gain(src[so:so + n], gd, out=dst[do:do + n])
            got = dst.cpu().numpy()
            want = base[so:so + n] * g
            assert out.data_ptr() == dst[do:do + n].data_ptr()
            assert got[do:do + n].tobytes() == want.tobytes(), (n, so, do)
            assert (got[:do] == -7.0).all() and (got[do + n:] == -7.0).all(), (n, so, do)       # nothing outside the range
        for so in (0, 1):                                           # in place
            buf = torch.from_numpy(base).cuda()
            L.apply_gain(buf[so:so + n], gd, out=buf[so:so + n])
            got = buf.cpu().numpy()
            assert got[so:so + n].tobytes() == (base[so:so + n] * g).tobytes()
            assert got[:so].tobytes() == base[:so].tobytes() and got[so + n:].tobytes() == base[so + n:].tobytes()
    fresh = L.apply_gain(torch.from_numpy(base).cuda(), gd)
    assert fresh.cpu().numpy().tobytes() == (base * g).tobytes()


# ---- (e) end to end on the burst signal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_normalise_end_to_end(rate):
    x = _sig(rate)
    xd = torch.from_numpy(np.array(x)).cuda()
    m = L.LoudnessMeter(L.LoudnessSpec(-16.0, -1.0, 20.0), rate, "cuda")
    y = m.normalise(xd).cpu().numpy()
    st = m.stats()
    assert st.valid and np.float32(st.gain) < np.float32(m.design.max_gain) and st.gain * st.peak < m.design.ceiling      # no clamp binds
    assert y.tobytes() == (x * np.float32(st.gain)).tobytes()
    got = R.measure64(y, rate)
    print(f"{rate} Hz: measured {st.lufs:.4f} LUFS, gain {st.gain_db:+.4f} dB, float64 reads the output at {got:.5f} LUFS")
    assert abs(got - (-16.0)) <= 0.01
    assert abs(st.lufs - R.measure64(x, rate)) <= 0.01
    # the ceiling binds: the peak lands on it, the loudness stays below the target
    m = L.LoudnessMeter(L.LoudnessSpec(-5.0, -6.0, 40.0), rate, "cuda")
    y = m.normalise(xd).cpu().numpy()
    pk = R.peak_and_bad(x)[0]
    assert np.abs(y).max() == np.float32(m.design.ceiling / float(pk)) * pk
    assert R.measure64(y, rate) < -5.0


# ---- (f) model level -------------------------------------------------------------------------------------------------------------------
TEXT = "The quick brown fox jumps. Over the lazy dog it goes! And then it sleeps for a while?"
_state = {}


def _model():
    if "m" not in _state:
        from fq3hip.config import tiny_test_config
        from fq3hip.model import FasterQwen3TTS
        from fq3hip.weights import synth_weights
        cfg = copy.deepcopy(tiny_test_config())
        cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "1b7"
        cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
        W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "text", "codec"))
        m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, max_frames=48, codec_max_frames=64)
        m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
        _state["m"] = m
        _state["kw"] = dict(do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0, max_new_tokens=22, min_new_tokens=22)
    return _state["m"], _state["kw"]


def _texts():
    from fq3hip.long_form import split_text
    return [s.text for s in split_text(TEXT, 40)]


def _plain_batch():
    """the unscaled waveforms of the three texts, computed once"""
    if "plain" not in _state:
        m, kw = _model()
        with m.seeded(0):
            _state["plain"] = [w[0].copy() for w, _sr in m.generate_custom_voice_batch(_texts(), "bob", "English", lanes=3, **kw)]
    return _state["plain"]


def test_model_one_shot_and_batch():
    m, kw = _model()
    texts = _texts()
    with m.seeded(0):
        plain, sr = m.generate_custom_voice(texts[0], "bob", "English", **kw)
        with m.loudness(-20.0) as sess:
            got, sr2 = m.generate_custom_voice(texts[0], "bob", "English", **kw)
            st = sess.stats
    assert sr == sr2 == 24000 and len(st) == 1 and st[0].valid and st[0].gain != 1.0 and st[0].n_hops == len(plain[0]) // 2400
    assert got[0].dtype == np.float32 and got[0].tobytes() == (plain[0] * np.float32(st[0].gain)).tobytes()
    assert m.measure_loudness(plain[0], L.LoudnessSpec(-20.0)) == st[0]
    assert m.measure_loudness(torch.from_numpy(plain[0]).cuda(), L.LoudnessSpec(-20.0)) == st[0]
    # in front of an open audio_output stage: the scaled float waveform is what the stage encodes
    with m.seeded(0), m.loudness(-20.0), m.audio_output(8000, "s16"):
        enc, sr3 = m.generate_custom_voice(texts[0], "bob", "English", **kw)
    stage = ao.AudioOut(ao.AudioOutSpec(8000, "s16"), 24000, "cuda")
    assert sr3 == 8000 and np.array_equal(enc[0], stage.push_host(torch.from_numpy(got[0]).cuda(), final=True))
    # batch: every utterance by its own gain
    base = _plain_batch()
    with m.loudness(-20.0) as sess:
        with m.seeded(0):
            outs = m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, **kw)
        st = sess.stats
    assert len(outs) == len(st) == 3 and len({s.gain for s in st}) > 1
    for (w, _sr), s, b in zip(outs, st, base):
        assert s.valid and w[0].tobytes() == (b * np.float32(s.gain)).tobytes()
    assert m._loud is None
    kept = len(m._meters)                                          # one meter per (device, stream), whatever targets are asked for
    for target in (-18.0, -19.0, -21.0):
        m.measure_loudness(plain[0], L.LoudnessSpec(target))
    assert len(m._meters) == kept
    again, _ = m.generate_custom_voice_batch(texts[:1], "bob", "English", lanes=3, **kw)[0]      # outside: unchanged
    assert again[0].tobytes() == base[0].tobytes()


def test_model_long_form_levels_each_segment():
    from fq3hip.long_form import LongFormSpec, split_text
    m, kw = _model()
    base = _plain_batch()
    segs = split_text(TEXT, 40)
    peaks = [float(np.abs(base[0][h: h + 240]).max()) for h in range(0, len(base[0]), 240)]
    spec = LongFormSpec(max_chars=40, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=float(np.median(peaks)),
                        lead_hops=1, tail_hops=2, hold_hops=4)
    args = (spec.threshold, spec.lead_hops, spec.tail_hops, spec.hold_hops)
    pieces = [J.join([(w, spec.pause_samples(s.pause, 24000))], 24000, *args, last_pause=k + 1 < len(segs))
              for k, (w, s) in enumerate(zip(base, segs))]
    with m.seeded(0):
        plain, _ = m.generate_long_custom_voice(TEXT, "bob", "English", lanes=3, long_form=spec, **kw)
        with m.loudness(-20.0) as sess:
            got, sr = m.generate_long_custom_voice(TEXT, "bob", "English", lanes=3, long_form=spec, **kw)
            st = sess.stats
    assert np.array_equal(plain[0], np.concatenate(pieces)) and 0 < plain[0].size < sum(len(w) for w in base) + 2400
    assert len(st) == 3 and all(s.valid for s in st) and len({s.gain for s in st}) > 1
    for s, w in zip(st, base):                                      # each segment's RAW waveform was measured
        assert s == m.measure_loudness(w, L.LoudnessSpec(-20.0))
    want = np.concatenate([p * np.float32(s.gain) for p, s in zip(pieces, st)])
    assert sr == 24000 and got[0].tobytes() == want.tobytes()
    assert any((p[-10:] == 0).all() for p in pieces[:-1])           # the pauses are there, and zeros stay zeros


def test_model_streaming_refuses_loudness_and_takes_a_fixed_gain():
    m, kw = _model()
    text = _texts()[0]
    skw = dict(kw, chunk_size=4, non_streaming_mode=False)
    with m.loudness(-20.0):
        for gen in (lambda: m.generate_custom_voice_streaming(text, "bob", "English", **skw),
                    lambda: m.generate_custom_voice_batch_streaming([text], "bob", "English", lanes=2, **skw),
                    lambda: m.generate_long_custom_voice_streaming(TEXT, "bob", "English", lanes=3, **skw),
                    lambda: m.stream_custom_voice([text], "bob", "English", **dict(kw, chunk_size=4))):
            with pytest.raises(ValueError, match="fixed_gain"):
                next(gen())

    def run(**ctx):
        with m.seeded(0):
            if ctx:
                with m.audio_output(**ctx):
                    return [np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(text, "bob", "English", **skw)]
            return [np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(text, "bob", "English", **skw)]

    plain = run()
    with m.fixed_gain(-6.0) as factor:
        got = run()
        mulaw = run(sample_rate=8000, encoding="mulaw")
        with m.seeded(0):
            lanes = {}
            for i, a, _sr, _tm in m.generate_custom_voice_batch_streaming([text, text], "bob", "English", lanes=2, **skw):
                lanes.setdefault(i, []).append(np.asarray(a).copy())
            one, _ = m.generate_custom_voice(text, "bob", "English", **dict(kw, non_streaming_mode=False))
    f = np.float32(10.0 ** (-6.0 / 20.0))
    assert factor == float(f) and len(got) == len(plain) > 1
    for a, b in zip(got, plain):
        assert a.dtype == np.float32 and a.tobytes() == (b * f).tobytes()
    # through the output stage: the existing encoder, fed with the scaled float chunks
    stage = ao.AudioOut(ao.AudioOutSpec(8000, "mulaw"), 24000, "cuda")
    want = stage.push_host(torch.from_numpy(np.concatenate(got)).cuda(), final=True)
    assert np.concatenate(mulaw).dtype == np.uint8 and np.array_equal(np.concatenate(mulaw), want)
    # the batched streaming path and the one-shot path multiply too
    with m.seeded(0):
        lanes_plain = {}
        for i, a, _sr, _tm in m.generate_custom_voice_batch_streaming([text, text], "bob", "English", lanes=2, **skw):
            lanes_plain.setdefault(i, []).append(np.asarray(a).copy())
        one_plain, _ = m.generate_custom_voice(text, "bob", "English", **dict(kw, non_streaming_mode=False))
    for i in (0, 1):
        assert np.concatenate(lanes[i]).tobytes() == (np.concatenate(lanes_plain[i]) * f).tobytes()
    assert one[0].tobytes() == (one_plain[0] * f).tobytes()
    assert m._gain is None
