"""GPU: the leveller stage (level_target_kernel, level_apply_kernel and level_stats_kernel of csrc/level_kernels.cuh, behind
fq3_level_*) against tests/_level_ref.py: output, hop integers, target trace and stats bit for bit against
the float32 reference, independence of the cuts bit for bit, the hop integers against a separate LoudnessMeter, short streams, state
and capacity errors, in-place and odd alignment, the chain fixed gain -> leveller -> limiter -> s16, and the model's ``leveller``
context in its four families."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _level_ref as R
import _limit_ref as LR
from fq3hip import _lib
from fq3hip import audio_out as ao
from fq3hip import leveller as M
from fq3hip import limiter as LM
from fq3hip import loudness as L

RATES = (8000, 24000)
_cache = {}


def _case(rate, name, gain_db):
    """(signal, spec, reference) -- computed once and shared"""
    key = (rate, name, gain_db)
    if key not in _cache:
        if ("sig", rate) not in _cache:
            _cache[("sig", rate)] = R.signals(rate)
        spec = M.LevelSpec(initial_gain_db=gain_db)
        x = _cache[("sig", rate)][name]
        with np.errstate(invalid="ignore"):                           # (the NaN case: the reference's energies of the two hops it reaches)
            _cache[key] = (x, spec, R.level(x, rate, spec))
    return _cache[key]


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32)


def _run(x, rate, spec, sizes=None, final_empty=False, capacity=0):
    """a fresh leveller over ``x`` pushed in pieces of the lengths ``sizes`` cycles through (None: one push) -> (y, trace, stats)"""
    lev = M.Leveller(spec, rate, "cuda", capacity_hops=capacity)
    xd = torch.from_numpy(np.array(x)).cuda()
    n, pos, k, outs = len(x), 0, 0, []
    sizes = [n] if sizes is None else sizes
    while pos < n:
        step = min(sizes[k % len(sizes)], n - pos)
        k += 1
        last = pos + step == n and not final_empty
        y = lev.push(xd[pos:pos + step] if step else None, final=last)
        assert len(y) == step                                          # a push emits exactly what it took
        outs.append(y)
        pos += step
    if final_empty or n == 0:
        assert len(lev.push(None, final=True)) == 0
    y = torch.cat(outs).cpu().numpy() if outs else np.zeros(0, np.float32)
    return y, lev.trace(), lev.stats(), lev


def _same(got, want):
    """bit for bit (a NaN equals the same NaN)"""
    return torch.equal(_bits(got), _bits(want))


def _check(x, rate, spec, ref, got, name=""):
    y, tr, st, _lev = got
    assert y.dtype == np.float32 and _same(y, ref["y"]), name
    bad_hops = set(np.flatnonzero(ref["bad"]).tolist())
    clean = np.array([h not in bad_hops and h - 1 not in bad_hops for h in range(len(ref["energy"]))], dtype=bool)
    # with a non-finite sample the energies of the hops it reaches are unspecified (include/fq3hip.h, "Loudness"): hop h and h + 1
    assert torch.equal(torch.from_numpy(tr["energy"][clean].view(np.int64)), torch.from_numpy(ref["energy"][clean].view(np.int64))), name
    assert len(tr["energy"]) == len(ref["energy"])
    assert _same(tr["peak"], ref["peak"]) and torch.equal(torch.from_numpy(tr["bad"].astype(np.int64)), torch.from_numpy(ref["bad"])), name
    assert _same(tr["target"], ref["T"]), (name, tr["target"], ref["T"])
    s = ref["stats"]
    assert _same(np.float32(st.target_gain), np.float32(s["target_gain"])) and _same(np.float32(st.smooth_gain), np.float32(s["smooth_gain"])), name
    assert (st.n_hops, st.n_bad, int(st.valid)) == (s["n_hops"], s["n_bad"], s["valid"]), name
    if not bad_hops:
        assert (st.n_abs, st.n_rel, st.mean_power) == (s["n_abs"], s["n_rel"], s["mean_power"]), name


# ---- (a) bit for bit against the float32 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain_db", [0.0, 6.0])
@pytest.mark.parametrize("name", ["bursts", "quiet", "nan", "lead"])
@pytest.mark.parametrize("rate", RATES)
def test_device_equals_the_reference_bit_for_bit(rate, name, gain_db):
    x, spec, ref = _case(rate, name, gain_db)
    assert len(x) == 30 * (rate // 10) + 37
    got = _run(x, rate, spec)
    _check(x, rate, spec, ref, got, name)
    T, g0 = ref["T"], spec.g0
    if name == "bursts":
        assert ref["stats"]["valid"] == 1 and (T[12:] != g0).all() and (T[:11] == g0).all() and got[3].final_gain_db is not None
    if name == "quiet":
        assert (T == g0).all() and ref["stats"]["n_abs"] == 0 and got[3].final_gain_db is None
        assert _same(got[0], x * g0)
    if name == "nan":
        assert (T[13:] == g0).all() and (T[12] != g0) and ref["stats"]["n_bad"] == 1 and np.isnan(got[0][12 * (rate // 10) + 5])
        assert got[3].final_gain_db is None
    if name == "lead":
        H = rate // 10
        assert (T[:19] == g0).all() and T[-1] != g0                   # (at least 8 blocks behind the 10 silent hops come first)
        assert not got[0][:10 * H].any()                              # leading zeros stay zeros


def test_44100_with_a_hop_of_4410():
    for gain_db in (0.0, 6.0):
        x, spec, ref = _case(44100, "bursts", gain_db)
        assert ref["design"].H == 4410 and len(x) == 30 * 4410 + 37
        _check(x, 44100, spec, ref, _run(x, 44100, spec), "44100")
    _check(x, 44100, spec, ref, _run(x, 44100, spec, sizes=[1, 4409, 4410, 4411, 8823, 0]), "44100 cut")


# ---- (b) cut independence, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_cut_independence(rate):
    H = rate // 10
    for name in ("bursts", "nan"):
        x, spec, ref = _case(rate, name, 6.0)
        whole = _run(x, rate, spec)
        plans = {"mixed": ([1, H - 1, H, H + 1, 2 * H + 3, 0], True), "hop": ([H], True), "hop - 1": ([H - 1], False), "4097": ([4097], False),
                 "1 then all": ([1, len(x)], False)}
        for pname, (sizes, final_empty) in plans.items():
            got = _run(x, rate, spec, sizes=sizes, final_empty=final_empty)
            _check(x, rate, spec, ref, got, (name, pname))
            assert _same(got[0], whole[0]) and _same(got[1]["target"], whole[1]["target"]) and got[2] == whole[2], (name, pname)


# ---- (c) the hop integers are the meter's, the last target is its gain --------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_hop_integers_and_last_target_are_the_meters(rate):
    H = rate // 10
    x, spec, ref = _case(rate, "bursts", 0.0)
    x = x[:30 * H]                                                     # a whole-hop stream
    meter = L.LoudnessMeter(spec.loudness, rate, "cuda")
    meter.push(torch.from_numpy(x).cuda(), final=True)
    ms = meter.stats()
    _y, tr, st, _ = _run(x, rate, spec, sizes=[H + 3])
    assert torch.equal(torch.from_numpy(tr["energy"].view(np.int64)), torch.from_numpy(meter.hops().view(np.int64)))
    assert ms.valid and ms.n_abs >= spec.min_blocks
    assert _same(np.float32(tr["target"][-1]), np.float32(ms.gain)) and _same(np.float32(st.target_gain), np.float32(ms.gain))
    assert (st.n_hops, st.n_abs, st.n_rel, st.mean_power) == (ms.n_hops, ms.n_abs, ms.n_rel, ms.mean_power)


@pytest.mark.parametrize("rate", RATES)
def test_stream_shorter_than_four_hops(rate):
    H = rate // 10
    x, spec, _ = _case(rate, "bursts", 6.0)
    for n in (0, 1, H - 1, H, H + 1, 3 * H + 5, 4 * H):
        seg = np.array(x[H:H + n])
        ref = R.level(seg, rate, spec)
        assert (ref["T"] == spec.g0).all()
        for sizes, final_empty in (([max(n, 1)], False), ([7, 0, H], True)):
            got = _run(seg, rate, spec, sizes=sizes, final_empty=final_empty)
            _check(seg, rate, spec, ref, got, (n, sizes))
            assert _same(got[0], seg * spec.g0)


def test_state_errors_capacity_and_reset():
    rate, H = 8000, 800
    x, spec, ref = _case(rate, "bursts", 0.0)
    xd = torch.from_numpy(np.array(x)).cuda()
    lev = M.Leveller(spec, rate, "cuda", capacity_hops=30)
    lib = _lib.load()
    out = torch.empty(len(x) + H, device="cuda")
    assert lib.fq3_level_push(lev._h, None, 5, 0, C.c_void_p(out.data_ptr()), None) == _lib.FQ3_EINVAL
    assert lib.fq3_level_push(lev._h, C.c_void_p(xd.data_ptr()), 5, 0, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_level_push(lev._h, C.c_void_p(xd.data_ptr()), -1, 0, C.c_void_p(out.data_ptr()), None) == _lib.FQ3_EINVAL
    first = lev.push(xd[:5000])
    with pytest.raises(RuntimeError, match="capacity"):               # 31 hops: refused before anything is launched or changed
        lev.push(torch.zeros(len(x) - 5000 + H, device="cuda"))
    rest = lev.push(xd[5000:], final=True)
    assert _same(torch.cat([first, rest]).cpu().numpy(), ref["y"])     # the refused push left the stream where it was
    for args in ((xd[:10], False), (None, True)):
        with pytest.raises(_lib.Fq3Error) as err:
            lev.push(*args)
        assert err.value.code == _lib.FQ3_ESTATE
    assert _same(lev.trace()["target"], ref["T"])
    lev.reset()                                                       # a new stream on the same object
    assert lev.stats().target_gain == float(spec.g0) and lev.stats().n_hops == 0 and len(lev.trace()["energy"]) == 0
    q, _, qref = _case(rate, "lead", 0.0)
    assert _same(lev.push(torch.from_numpy(np.array(q)).cuda(), final=True).cpu().numpy(), qref["y"])
    assert _same(lev.trace()["target"], qref["T"])
    # the initial gain of the NEXT stream on a kept object: between reset and the first sample, and nowhere else
    assert lib.fq3_level_set_initial_gain(lev._h, 3.0) == _lib.FQ3_ESTATE                      # the stream has ended, not reset
    for g_db in (6.0, -4.5):
        lev.reset(g_db)
        assert lev.spec == M.LevelSpec(initial_gain_db=g_db) and lev.stats().target_gain == float(lev.spec.g0)
        assert lib.fq3_level_set_initial_gain(lev._h, 41.0) == _lib.FQ3_EINVAL
        first = lev.push(torch.from_numpy(np.array(q[:5000])).cuda())
        assert lib.fq3_level_set_initial_gain(lev._h, 0.0) == _lib.FQ3_ESTATE                  # the stream has begun
        rest = lev.push(torch.from_numpy(np.array(q[5000:])).cuda(), final=True)
        want = R.level(q, rate, lev.spec)                              # what a fresh object made for that gain gives, bit for bit
        assert _same(torch.cat([first, rest]).cpu().numpy(), want["y"]) and _same(lev.trace()["target"], want["T"])
    with pytest.raises(ValueError):
        lev.reset(41.0)
    lev.reset()                                                       # a reset alone keeps the last gain
    assert lev.spec.initial_gain_db == -4.5 and lev.stats().target_gain == float(lev.spec.g0)
    for kw in (dict(smooth_hops=65), dict(min_blocks=0), dict(initial_gain_db=41.0), dict(target_lufs=-4.0)):
        with pytest.raises(ValueError):
            M.LevelSpec(**kw)
    cfg = _lib.LevelConfig(8000, -16.0, -1.0, 20.0, 0.0, 65, 8, 0)
    h = C.c_void_p()
    assert lib.fq3_level_create(C.byref(cfg), C.byref(h)) == _lib.FQ3_EINVAL and not h.value
    with pytest.raises(ValueError):
        M.Leveller(spec, 8050, "cuda")


@pytest.mark.parametrize("rate", RATES)
def test_in_place_and_odd_alignment(rate):
    x, spec, ref = _case(rate, "bursts", 6.0)
    n = len(x)
    for off_in, off_out in ((0, 0), (1, 1), (3, 3), (1, 2), (0, 3)):
        buf = torch.zeros(n + 8, device="cuda")
        src = buf[off_in:off_in + n]
        src.copy_(torch.from_numpy(np.array(x)))
        dst = torch.full((n + 8,), 7.0, device="cuda")
        lev = M.Leveller(spec, rate, "cuda")
        y = lev.push(src, final=True, out=dst[off_out:off_out + n])
        assert _same(y.cpu().numpy(), ref["y"]), (off_in, off_out)
        assert (dst[:off_out] == 7.0).all() and (dst[off_out + n:] == 7.0).all()      # nothing written outside
    for off in (0, 1):                                                 # out == pcm
        buf = torch.zeros(n + 8, device="cuda")
        src = buf[off:off + n]
        src.copy_(torch.from_numpy(np.array(x)))
        lev = M.Leveller(spec, rate, "cuda")
        H = rate // 10
        for a, b in ((0, H + 5), (H + 5, n)):
            lev.push(src[a:b], final=b == n, out=src[a:b])
        assert _same(src.cpu().numpy(), ref["y"]) and not buf[:off].any() and not buf[off + n:].any()


# ---- (d) fixed gain -> leveller -> limiter -> s16 -----------------------------------------------------------------------------------------
def test_chain_gain_leveller_limiter_s16():
    rate = 24000
    x, _, _ = _case(rate, "bursts", 0.0)
    spec = M.LevelSpec(target_lufs=-8.0, smooth_hops=3, min_blocks=2)       # pushes the bursts over the limiter's ceiling
    g = np.float32(2.0)
    gained = L.apply_gain(torch.from_numpy(np.array(x)).cuda(), torch.tensor([float(g)], device="cuda"))
    lev, lim = M.Leveller(spec, rate, "cuda"), LM.Limiter(None, rate, "cuda")
    stage = ao.AudioOut(ao.AudioOutSpec(rate, "s16"), rate, "cuda")
    outs, H = [], rate // 10
    for a in range(0, len(x), 3 * H + 11):
        last = a + 3 * H + 11 >= len(x)
        outs.append(stage.push(lim.push(lev.push(gained[a:a + 3 * H + 11], final=last), final=last), final=last).cpu().numpy())
    got = np.concatenate(outs)
    levelled = R.level(x * g, rate, spec)
    d = LM.design(rate)
    limited = LR.emulate(levelled["y"], d)
    assert float(np.abs(levelled["y"]).max()) > float(d.c) and limited.n_limited > 0       # the limiter has work: the leveller does not limit
    by_hand = ao.AudioOut(ao.AudioOutSpec(rate, "s16"), rate, "cuda").push(torch.from_numpy(limited.y).cuda(), final=True).cpu().numpy()
    assert got.dtype == np.int16 and np.array_equal(got, by_hand)


# ---- (e) the model's context ----------------------------------------------------------------------------------------------------------------
TEXT = "The quick brown fox jumps. Over the lazy dog it goes!"
SPEC = dict(target_lufs=-20.0, smooth_hops=3, min_blocks=2)           # a 22-frame utterance has 17 hops: the stage must get to work in it
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


def _want(plain, spec, factor=None):
    x = plain if factor is None else plain * np.float32(factor)
    ref = R.level(x, 24000, spec)
    assert ref["stats"]["valid"] == 1 and (ref["T"] != spec.g0).any()      # the stage had work to do
    return ref["y"]


def _stream(m, kw, chunk):
    skw = dict(kw, chunk_size=chunk, non_streaming_mode=False)
    with m.seeded(0):
        return np.concatenate([np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(TEXT, "bob", "English", **skw)])


def test_model_leveller_context_streaming_and_one_shot():
    m, kw = _model()
    with m.exact_streaming():
        plain = _stream(m, kw, 4)
        with m.fixed_gain(12.0) as f, m.leveller(**SPEC) as spec:
            a = _stream(m, kw, 4)
            b = _stream(m, kw, 7)
            learned = m.last_level_gain_db
            with m.limiter():
                c = _stream(m, kw, 4)
    assert spec == M.LevelSpec(**SPEC) and m._lvl is None
    assert len(m._leveller_pools[spec]) == 1                         # three streams one after another: one object, reset and reused
    # requests of a voice whose learned gain differs every time (the server's memory): still that ONE object and no new pool key
    kept = m._leveller_pools[spec][0]
    with m.exact_streaming():
        for g_db in (-3.25, 2.5, 7.125):
            with m.leveller(initial_gain_db=g_db, **SPEC) as warm:
                got_g = _stream(m, kw, 4)
            assert _same(got_g, _want(plain, warm))                  # and each starts from ITS gain, bit for bit
            assert list(m._leveller_pools) == [spec] and len(m._leveller_pools[spec]) == 1 and m._leveller_pools[spec][0] is kept
        # the batch worker's form: the vocoder is made inside the server-wide context and its spec is replaced before the first chunk
        import dataclasses
        with m.leveller(**SPEC):
            for g_db in (1.0, -2.0):
                voc = m.streaming_vocoder(None, 4)
                voc.level_spec = dataclasses.replace(voc.level_spec, initial_gain_db=g_db)
                x = torch.from_numpy(plain.copy()).to("cuda")
                with torch.cuda.stream(voc.side):
                    y = voc.level_push(x, True).cpu().numpy()
                    host, ev = voc.level_report_async()
                ev.synchronize()
                want_g = R.level(plain, 24000, voc.level_spec)
                assert _same(y, want_g["y"]) and m._leveller_pools[spec] == [kept]
                assert abs(voc.level_gain_of(host) - 20.0 * np.log10(float(want_g["T"][-1]))) < 1e-4 and voc.level_gain_db == voc.level_gain_of(host)
    assert kept.capacity_hops == m._stream_level_hops() >= 4096       # sized for the longest stream the model decodes
    want = _want(plain, spec, f)
    assert len(a) == len(plain) and _same(a, want) and _same(b, want)          # the chunk size does not matter
    assert learned is not None and abs(learned - 20.0 * np.log10(float(R.level(plain * np.float32(f), 24000, spec)["T"][-1]))) < 1e-4
    assert _same(c, LR.emulate(want, LM.design(24000)).y)             # the limiter sits behind it
    with m.seeded(0):
        one, sr = m.generate_custom_voice(TEXT, "bob", "English", **kw)
        with m.leveller(**SPEC):
            got, sr2 = m.generate_custom_voice(TEXT, "bob", "English", **kw)
            with pytest.raises(ValueError, match="same question"):
                with m.loudness():
                    pass
    assert sr == sr2 == 24000 and _same(got[0], _want(one[0], spec))
    assert _same(_stream(m, kw, 4), np.concatenate([_stream(m, kw, 4)]))     # outside the context: what it was
    with m.seeded(0):
        again, _ = m.generate_custom_voice(TEXT, "bob", "English", **kw)
    assert _same(again[0], one[0])


def test_model_leveller_context_batch_streaming_and_long_form():
    from fq3hip.long_form import LongFormSpec
    m, kw = _model()
    texts = [TEXT, TEXT[:26]]
    skw = dict(kw, chunk_size=4, non_streaming_mode=False)

    def lanes():
        out = {}
        with m.seeded(0):
            for i, a, _sr, _tm in m.generate_custom_voice_batch_streaming(texts, "bob", "English", lanes=2, **skw):
                out.setdefault(i, []).append(np.asarray(a, dtype=np.float32).copy())
        return {i: np.concatenate(v) for i, v in out.items()}

    with m.exact_streaming():
        plain = lanes()
        with m.leveller(**SPEC) as spec:
            got = lanes()
    assert sorted(got) == sorted(plain) == [0, 1] and len(m._leveller_pools[spec]) == 2      # two lanes at once: two objects, kept
    for i in plain:
        assert len(got[i]) == len(plain[i]) and _same(got[i], _want(plain[i], spec)), i
    # long form: ONE leveller behind the join, on the joined stream
    lspec = LongFormSpec(max_chars=40, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=1e-4, lead_hops=1, tail_hops=2,
                         hold_hops=4)
    long_text = TEXT + " And then it sleeps for a while?"
    lkw = dict(lanes=3, long_form=lspec, **kw)

    def streamed():
        with m.seeded(0):
            return np.concatenate([np.asarray(a).copy() for a, _sr, _tm in
                                   m.generate_long_custom_voice_streaming(long_text, "bob", "English", chunk_size=4, **lkw)])
    plain_stream = streamed()
    with m.leveller(**SPEC) as spec:
        got_stream = streamed()
        with pytest.raises(ValueError, match="2\\^20"):                # beyond 2^20 hops: refused before anything decodes
            with m.seeded(0):
                m.generate_long_custom_voice(long_text, "bob", "English", **dict(lkw, max_new_tokens=40_000_000))
    assert len(got_stream) == len(plain_stream) and _same(got_stream, _want(plain_stream, spec))
