"""GPU: the limiter stage (limit_push_kernel and limit_stats_kernel of csrc/limit_kernels.cuh, behind fq3_limit_*; DESIGN.md
section 4.16) against tests/_limit_ref.py: output,
stats and counts bit for bit against the float32 emulation, independence of the cuts and of the tile bit for bit, the true peak of
the output under the bound measured on the CPU, the chain gain -> limiter -> time-scale -> s16, and the model's ``limiter`` context."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _limit_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao
from fq3hip import limiter as M
from fq3hip import loudness as L

ONE = R.ONE


def _spec(db):
    return M.LimiterSpec(ceiling_db=db)


def _run(x, rate, db=-1.0, sizes=None, tile=0, final_empty=False):
    """a fresh limiter over ``x`` pushed in pieces of the lengths ``sizes`` cycles through (None: one push); ``final_empty``: the stream
    ends with a push of no samples -> (output, stats tuple, the length of every push's output)"""
    lim = M.Limiter(_spec(db), rate, "cuda", tile=tile)
    xd = torch.from_numpy(np.array(x)).cuda()
    n, pos, k, outs, counts = len(x), 0, 0, [], []
    if sizes is None:
        sizes = [n]
    while pos < n:
        step = min(sizes[k % len(sizes)], n - pos)
        k += 1
        last = pos + step == n and not final_empty
        outs.append(lim.push(xd[pos:pos + step] if step else None, final=last))
        pos += step
        counts.append(len(outs[-1]))
        assert lim.n_out == M.count(rate, lim.spec, pos, last)
    if final_empty or n == 0:
        outs.append(lim.push(None, final=True))
        counts.append(len(outs[-1]))
    st = lim.stats()
    y = torch.cat(outs).cpu().numpy() if outs else np.zeros(0, np.float32)
    return y, (np.float32(st.true_peak).tobytes(), st.min_gain_q23, st.n_limited, st.n_bad), counts


# ---- (a) bit for bit against the float32 emulation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bursts", "sine", "bad", "quiet"])
@pytest.mark.parametrize("db", R.CEILINGS)
@pytest.mark.parametrize("rate", R.RATES)
def test_device_equals_the_reference_bit_for_bit(rate, db, name):
    d, sig, emu = R.case(rate, db)
    x, e = sig[name], emu[name]
    y, st, counts = _run(x, rate, db)
    assert counts == [len(x)] and y.dtype == np.float32
    assert st == R.stats_tuple(e), (st, R.stats_tuple(e))
    diff = np.flatnonzero(y.view(np.uint32) != e.y.view(np.uint32))
    assert diff.size == 0, (diff[:8], y[diff[:8]], e.y[diff[:8]])
    assert float(np.abs(y).max()) <= float(d.c) * (1.0 + 2.0 ** -22)
    if name == "quiet":
        assert y.tobytes() == x.tobytes() and st[1] == ONE and st[2] == 0       # the delayed input, bit for bit
    if name == "bad":
        assert st[3] == 3 and np.isfinite(y).all()
    if name in ("bursts", "sine") and (db == -1.0 or name == "bursts"):
        assert st[2] > 0 and st[1] < ONE


# ---- (b) cut and tile independence, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", R.RATES)
def test_cut_independence(rate):
    d, sig, emu = R.case(rate, -1.0)
    x, e = sig["bad"], emu["bad"]
    want = (e.y.tobytes(), R.stats_tuple(e))
    T, lat = d.tile, d.latency
    plans = {"1": [1], "7": [7], "latency": [lat], "latency + 1": [lat + 1], "tile - 1": [T - 1], "tile": [T], "tile + 1": [T + 1],
             "mixed": [1, 0, 7, lat, 0, 0, lat + 1, T - 1, 1, 1, 1, T, 0, T + 1, 3]}
    for name, sizes in plans.items():
        y, st, counts = _run(x, rate, sizes=sizes, final_empty=name in ("mixed", "tile"))
        assert (y.tobytes(), st) == want, name
        assert sum(counts) == len(x), name
    for tile in (256, 4096):                                        # the tile changes the speed, never the result
        y, st, _ = _run(x, rate, tile=tile, sizes=[3 * tile + 5])
        assert (y.tobytes(), st) == want, tile


@pytest.mark.parametrize("rate", R.RATES)
def test_stream_shorter_than_the_latency(rate):
    d, sig, _ = R.case(rate, -6.0)
    for n in (0, 1, d.A, d.latency - 1, d.latency, d.latency + 1):
        x = np.array(sig["bursts"][d.A:d.A + n]) * np.float32(3.0)
        e = R.emulate(x, d)
        for sizes, final_empty in (([max(n, 1)], True), ([max(n, 1)], False), ([1], True), ([2, 0, 1], False)):
            y, st, counts = _run(x, rate, -6.0, sizes=sizes, final_empty=final_empty)
            assert y.tobytes() == e.y.tobytes() and len(y) == n, (n, sizes)
            if n:
                assert st == R.stats_tuple(e), (n, sizes)
            if final_empty and n < d.latency:
                assert sum(counts[:-1]) == 0 and counts[-1] == n        # nothing before the end, everything with it


def test_state_errors_and_reset():
    d, sig, emu = R.case(24000, -1.0)
    x = torch.from_numpy(np.array(sig["bursts"])).cuda()
    lim = M.Limiter(None, 24000, "cuda")
    lib, got = _lib.load(), C.c_int64()
    out = torch.empty(len(x), device="cuda")
    # too little room: refused before anything is launched or changed
    assert lib.fq3_limit_push(lim._h, C.c_void_p(x.data_ptr()), 1000, 0, C.c_void_p(out.data_ptr()), 1000 - d.latency - 1, C.byref(got),
                              None) == _lib.FQ3_EINVAL
    assert lib.fq3_limit_push(lim._h, None, 5, 0, C.c_void_p(out.data_ptr()), 100, C.byref(got), None) == _lib.FQ3_EINVAL
    first = lim.push(x[:5000])
    rest = lim.push(x[5000:], final=True)
    assert len(first) == 5000 - d.latency and len(rest) == len(x) - len(first)
    with pytest.raises(_lib.Fq3Error) as err:
        lim.push(x[:10])
    assert err.value.code == _lib.FQ3_ESTATE
    with pytest.raises(_lib.Fq3Error) as err:
        lim.push(None, final=True)
    assert err.value.code == _lib.FQ3_ESTATE
    st = lim.stats()
    assert (np.float32(st.true_peak).tobytes(), st.min_gain_q23, st.n_limited, st.n_bad) == R.stats_tuple(emu["bursts"])
    lim.reset()                                                      # a new stream: the accumulators start over
    q = torch.from_numpy(np.array(sig["quiet"])).cuda()
    assert lim.push(q, final=True).cpu().numpy().tobytes() == sig["quiet"].tobytes()
    st = lim.stats()
    assert st.n_limited == 0 and st.min_gain_q23 == ONE and np.float32(st.true_peak) == emu["quiet"].true_peak
    assert lim.push_host is not None and M.Limiter(None, 24000, "cuda").push_host(sig["quiet"], final=True).tobytes() == sig["quiet"].tobytes()


# ---- (c) the true peak of the device's output ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("db", R.CEILINGS)
@pytest.mark.parametrize("rate", R.RATES)
def test_true_peak_of_the_output_stays_under_the_measured_bound(rate, db):
    d, sig, _ = R.case(rate, db)
    bound = R.true_peak_bound(rate, db)
    for name in ("bursts", "sine", "bad"):
        y, _, _ = _run(sig[name], rate, db)
        tp = R.true_peak64(y)
        print(f"{rate} Hz {db:+.0f} dB {name}: output true peak {tp / float(d.c):.4f} c, bound {bound / float(d.c):.4f} c")
        assert tp <= bound, name
    if db == -1.0:
        assert R.true_peak64(sig["sine"]) > 1.19 and R.true_peak64(_run(sig["sine"], rate, db)[0]) < 1.01 * float(d.c)


# ---- (d) gain -> limiter -> time-scale -> s16 ---------------------------------------------------------------------------------------------
def test_chain_gain_limiter_timescale_s16():
    rate, db = 24000, -1.0
    d, sig, _ = R.case(rate, db)
    x = np.array(sig["bursts"]) * np.float32(0.25)                  # the gain brings it back to +12 dB over the ceiling
    g = np.float32(4.0)
    xd = torch.from_numpy(x).cuda()
    gained = L.apply_gain(xd, torch.tensor([float(g)], device="cuda"))
    assert gained.cpu().numpy().tobytes() == sig["bursts"].tobytes()

    def tail(wav):
        """the existing stages, fed by hand: time-scale at speed 1.25 and s16 at the same rate (one AudioOut holds both)"""
        stage = ao.AudioOut(ao.AudioOutSpec(rate, "s16", speed=1.25), rate, "cuda")
        return stage.push(wav, final=True).cpu().numpy()

    lim = M.Limiter(_spec(db), rate, "cuda")
    limited = lim.push(gained, final=True)
    by_hand = tail(torch.from_numpy(R.emulate(sig["bursts"], d).y).cuda())
    got = tail(limited)
    assert got.dtype == np.int16 and np.array_equal(got, by_hand)
    assert int(np.abs(got.astype(np.int32)).max()) < 32767          # WSOLA is a convex combination: the sample peak cannot rise
    assert int(np.abs(got.astype(np.int32)).max()) <= int(np.ceil(float(d.c) * (1 + 2.0 ** -22) * 32767)) + 1
    clipped = tail(gained)                                          # the same chain without the limiter clamps
    assert int(np.abs(clipped.astype(np.int32)).max()) >= 32767 and (np.abs(clipped.astype(np.int32)) >= 32767).sum() > 10


# ---- (e) the model's context ------------------------------------------------------------------------------------------------------------
TEXT = "The quick brown fox jumps. Over the lazy dog it goes!"
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


def _stream(m, kw, chunk, **ctx):
    skw = dict(kw, chunk_size=chunk, non_streaming_mode=False)
    with m.seeded(0):
        if ctx:
            with m.audio_output(**ctx):
                return [np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(TEXT, "bob", "English", **skw)]
        return [np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(TEXT, "bob", "English", **skw)]


def test_model_limiter_context_streaming():
    m, kw = _model()
    d = M.design(24000)
    lim_c = float(d.c) * (1.0 + 2.0 ** -22)
    with m.exact_streaming():
        plain = np.concatenate(_stream(m, kw, 4))
        with m.fixed_gain(18.0) as f:
            hot = np.concatenate(_stream(m, kw, 4))
            with m.limiter() as spec:
                a = _stream(m, kw, 4)
                b = _stream(m, kw, 7)
                s16 = np.concatenate(_stream(m, kw, 4, sample_rate=24000, encoding="s16"))
    assert spec == M.LimiterSpec() and m._limit is None
    assert len(m._limiter_pools[spec]) == 1                          # three streams one after another: one object, reset and reused
    a, b = np.concatenate(a), np.concatenate(b)
    assert hot.tobytes() == (plain * np.float32(f)).tobytes() and float(np.abs(hot).max()) > lim_c     # the limiter has work to do
    assert a.dtype == np.float32 and len(a) == len(plain) and float(np.abs(a).max()) <= lim_c
    assert a.tobytes() == b.tobytes()                                # one stream, whatever the chunk size
    assert a.tobytes() == R.emulate(hot, d).y.tobytes()              # and it is the contract's output for the gained stream
    stage = ao.AudioOut(ao.AudioOutSpec(24000, "s16"), 24000, "cuda")
    assert np.array_equal(s16, stage.push_host(torch.from_numpy(a).cuda(), final=True)) and int(np.abs(s16.astype(np.int32)).max()) < 32767
    # the reference's windowing (no exact_streaming): the held-back samples still come out, the length stays
    base = np.concatenate(_stream(m, kw, 4))
    with m.limiter(-6.0):
        lim = np.concatenate(_stream(m, kw, 4))
    d6 = M.design(24000, M.LimiterSpec(-6.0))
    assert len(lim) == len(base) and lim.tobytes() == R.emulate(base, d6).y.tobytes()
    # outside the context: bit-identical to what it was
    assert np.concatenate(_stream(m, kw, 4)).tobytes() == base.tobytes()


def test_model_limiter_context_one_shot_and_batch():
    m, kw = _model()
    d = M.design(24000)
    with m.seeded(0):
        plain, sr = m.generate_custom_voice(TEXT, "bob", "English", **kw)
        with m.fixed_gain(18.0) as f, m.limiter():
            got, sr2 = m.generate_custom_voice(TEXT, "bob", "English", **kw)
            with m.audio_output(8000, "mulaw"):
                enc, sr3 = m.generate_custom_voice(TEXT, "bob", "English", **kw)
        with m.limiter(-12.0):
            alone, _ = m.generate_custom_voice(TEXT, "bob", "English", **kw)
    want = R.emulate(plain[0] * np.float32(f), d).y
    assert sr == sr2 == 24000 and got[0].tobytes() == want.tobytes() and float(np.abs(got[0]).max()) <= float(d.c) * (1 + 2.0 ** -22)
    stage = ao.AudioOut(ao.AudioOutSpec(8000, "mulaw"), 24000, "cuda")
    assert sr3 == 8000 and np.array_equal(enc[0], stage.push_host(torch.from_numpy(got[0]).cuda(), final=True))
    assert alone[0].tobytes() == R.emulate(plain[0], M.design(24000, M.LimiterSpec(-12.0))).y.tobytes()
    with m.seeded(0):
        base = [w[0].copy() for w, _sr in m.generate_custom_voice_batch([TEXT, TEXT[:26]], "bob", "English", lanes=2, **kw)]
        with m.fixed_gain(18.0) as f, m.limiter():
            outs = [w[0].copy() for w, _sr in m.generate_custom_voice_batch([TEXT, TEXT[:26]], "bob", "English", lanes=2, **kw)]
    for o, bse in zip(outs, base):
        assert o.tobytes() == R.emulate(bse * np.float32(f), d).y.tobytes()
    again, _ = m.generate_custom_voice(TEXT, "bob", "English", **kw)
    with m.seeded(0):
        again, _ = m.generate_custom_voice(TEXT, "bob", "English", **kw)
    assert again[0].tobytes() == plain[0].tobytes()                  # outside: unchanged


def test_model_limiter_context_batch_streaming_and_long_form():
    from fq3hip.long_form import LongFormSpec
    m, kw = _model()
    d = M.design(24000)
    texts = [TEXT, TEXT[:26]]
    skw = dict(kw, chunk_size=4, non_streaming_mode=False)

    def lanes():
        out = {}
        with m.seeded(0):
            for i, a, _sr, _tm in m.generate_custom_voice_batch_streaming(texts, "bob", "English", lanes=2, **skw):
                out.setdefault(i, []).append(np.asarray(a, dtype=np.float32).copy())
        return {i: np.concatenate(v) for i, v in out.items()}

    # every lane's utterance through its own limiter, the rows of a group launch handed to them one by one
    for exact in (True, False):
        with (m.exact_streaming() if exact else contextlib.nullcontext()):
            plain = lanes()
            with m.fixed_gain(18.0) as f, m.limiter():
                got = lanes()
        assert sorted(got) == sorted(plain) == [0, 1]
        assert len(m._limiter_pools[M.LimiterSpec()]) == 2           # two lanes at once: two objects, kept for the next utterances
        for i in plain:
            want = R.emulate(plain[i] * np.float32(f), d).y
            assert len(got[i]) == len(plain[i]) and got[i].tobytes() == want.tobytes(), (exact, i)
            assert float(np.abs(plain[i]).max()) * f > float(d.c) >= float(np.abs(got[i]).max()) / (1 + 2.0 ** -22)
    # long form: ONE limiter behind the join and the gains, in front of the output chain
    spec = LongFormSpec(max_chars=40, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=1e-4, lead_hops=1, tail_hops=2,
                        hold_hops=4)
    long_text = TEXT + " And then it sleeps for a while?"
    lkw = dict(lanes=3, long_form=spec, **kw)

    def streamed(**ctx):
        with m.seeded(0), (m.audio_output(**ctx) if ctx else contextlib.nullcontext()):
            return np.concatenate([np.asarray(a).copy() for a, _sr, _tm in
                                   m.generate_long_custom_voice_streaming(long_text, "bob", "English", chunk_size=4, **lkw)])
    with m.seeded(0):
        plain, _ = m.generate_long_custom_voice(long_text, "bob", "English", **lkw)
    plain_stream = streamed()
    with m.fixed_gain(18.0) as f, m.limiter():
        with m.seeded(0):
            got, sr = m.generate_long_custom_voice(long_text, "bob", "English", **lkw)
        got_stream = streamed()
        got_s16 = streamed(sample_rate=24000, encoding="s16")
    assert sr == 24000 and got[0].tobytes() == R.emulate(plain[0] * np.float32(f), d).y.tobytes()
    assert got_stream.tobytes() == R.emulate(plain_stream * np.float32(f), d).y.tobytes() and len(got_stream) == len(plain_stream)
    stage = ao.AudioOut(ao.AudioOutSpec(24000, "s16"), 24000, "cuda")
    assert np.array_equal(got_s16, stage.push_host(torch.from_numpy(got_stream).cuda(), final=True))
