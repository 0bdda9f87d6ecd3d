"""GPU: the device audio output stage (csrc/audio_kernels.cuh behind fq3_audio_out_*) through ctypes, and
its opt-in through the public API.

The contract has two halves.  Accuracy: the resampler's float32 output against a float64 evaluation of the SAME float32 bank, per
sample, within the bound of a length-K fp32 dot product.  Identity: the result does not depend on how the stream was cut into pushes,
on where the output buffer starts, or on whether the object is fresh -- those comparisons are ``torch.equal``, no tolerance."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip import _lib, audio_io
from fq3hip import audio_out as ao

N_IN = 4801
Z = 16
FORMATS = {"f32": (0, torch.float32), "s16": (1, torch.int16), "mulaw": (2, torch.uint8), "alaw": (3, torch.uint8)}


def _rates(ratio):
    out, inp = ratio
    return 100 * inp, 100 * out


_signal_cache = {}


def _signal():
    """4801 samples: half noise in [-1, 1], half a sine sweep (made once, never modified)"""
    if "x" not in _signal_cache:
        rng = np.random.default_rng(11)
        n1 = N_IN // 2
        t = np.arange(N_IN - n1) / (N_IN - n1)
        sweep = 0.9 * np.sin(2 * np.pi * (20.0 * t + 0.5 * 1100.0 * t * t))
        x = np.concatenate([rng.uniform(-1.0, 1.0, n1), sweep]).astype(np.float32)
        x.setflags(write=False)
        _signal_cache["x"] = x
        _signal_cache["dev"] = torch.from_numpy(x.copy()).cuda()
    return _signal_cache["x"], _signal_cache["dev"]


class _Stage:
    """fq3_audio_out_* through ctypes, on the current stream"""

    def __init__(self, ratio, fmt):
        self.lib = _lib.load()
        self.i, self.o = _rates(ratio)
        self.fmt, self.dtype = FORMATS[fmt]
        cfg = _lib.AudioOutConfig(self.i, self.o, self.fmt, 0)
        self.h = C.c_void_p()
        assert self.lib.fq3_audio_out_create(C.byref(cfg), C.byref(self.h)) == 0, self.lib.fq3_last_error()
        self.n_in = self.n_out = 0

    def __del__(self):
        self.lib.fq3_audio_out_destroy(self.h)

    def count(self, n_in, final):
        return self.lib.fq3_audio_out_count(self.i, self.o, 0, n_in, 1 if final else 0)

    def raw_push(self, x, final, out_ptr, cap):
        n = C.c_int64(-1)
        s = torch.cuda.current_stream().cuda_stream
        rc = self.lib.fq3_audio_out_push(self.h, C.c_void_p(x.data_ptr() if x.numel() else None), x.numel(), 1 if final else 0,
                                         C.c_void_p(out_ptr), cap, C.byref(n), C.c_void_p(s))
        return rc, n.value

    def push(self, x, final=False):
        cap = self.count(self.n_in + x.numel(), final) - self.n_out
        out = torch.empty(cap, dtype=self.dtype, device="cuda")
        rc, n = self.raw_push(x, final, out.data_ptr() if cap else None, cap)
        assert rc == 0 and n == cap, (rc, n, cap, self.lib.fq3_last_error())
        self.n_in += x.numel()
        self.n_out += cap
        return out

    def reset(self):
        assert self.lib.fq3_audio_out_reset(self.h, None) == 0
        self.n_in = self.n_out = 0


def _one_push(ratio, fmt, x):
    return _Stage(ratio, fmt).push(x, final=True)


# ---- 1. float64 reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(1, 3), (2, 3), (147, 160), (147, 80), (2, 1), (80, 147), (147, 320)], ids=lambda r: f"{r[0]}over{r[1]}")
def test_f32_output_against_float64_reference(ratio):
    """|y - y_ref| <= (K + 2) 2^-24 sum_k |h_k x_k| per sample: the standard bound of a length-K fp32 dot product (K roundings of the
    fmaf chain; + 2 of margin for the reference's own evaluation), y_ref in float64 from the library's float32 bank."""
    x, xd = _signal()
    i, o = _rates(ratio)
    L, M, K, bank = ao.design(i, o)
    assert (L, M) == ratio
    st = _Stage(ratio, "f32")
    y = st.push(xd, final=True).cpu().numpy().astype(np.float64)
    n_out = st.count(N_IN, True)
    assert len(y) == n_out == -((-N_IN * L) // M)
    half = Z * max(L, M)
    n = np.arange(n_out, dtype=np.int64)
    idx = ((n * M + half) // L - (K - 1))[:, None] + np.arange(K)[None, :]
    ok = (idx >= 0) & (idx < N_IN)
    xs = np.where(ok, x.astype(np.float64)[np.clip(idx, 0, N_IN - 1)], 0.0)
    prod = bank.astype(np.float64)[(n * M) % L] * xs
    ref, bound = prod.sum(axis=1), (K + 2) * 2.0 ** -24 * np.abs(prod).sum(axis=1)
    err = np.abs(y - ref)
    print(f"{ratio}: K {K}, max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-30)):.3f}")
    assert np.all(err <= bound), (int(np.argmax(err - bound)), float(err.max()))
    assert np.abs(ref).max() > 0.5          # the comparison is not about silence


# ---- 2. the cut does not matter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(1, 3), (147, 80), (1, 1)], ids=lambda r: f"{r[0]}over{r[1]}")
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_result_does_not_depend_on_the_cut(ratio, fmt):
    _x, xd = _signal()
    K = ao.design(*_rates(ratio), bank=False)[2]
    whole = _one_push(ratio, fmt, xd)
    assert whole.numel() == _Stage(ratio, fmt).count(N_IN, True)
    for sizes in ([1, 7, 0, K - 1, K, 1919, 1920], [1] * 300):
        st, at, parts = _Stage(ratio, fmt), 0, []
        for s in sizes:
            parts.append(st.push(xd[at:at + s], final=False))
            at += s
        parts.append(st.push(xd[at:], final=True))
        assert sum(p.numel() for p in parts[:-1]) == st.count(at, False)
        assert torch.equal(torch.cat(parts), whole), (ratio, fmt, len(sizes))


# ---- 3. encoders -------------------------------------------------------------------------------------------------------------------
def _g711_mulaw(s):
    """ITU-T G.711 mu-law from 16-bit linear, the classic 16-bit form: magnitude clipped at 32635, bias 0x84, segment from the table of
    segment ends, 4 mantissa bits below the segment's leading one, all bits complemented."""
    s = np.asarray(s, dtype=np.int64)
    sign = np.where(s < 0, 0x80, 0)
    mag = np.minimum(np.abs(s), 32635) + 0x84
    seg = np.searchsorted(np.array([0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF, 0x3FFF, 0x7FFF]), mag, side="left")
    return (~(sign | (seg << 4) | ((mag >> (seg + 3)) & 0x0F)) & 0xFF).astype(np.uint8)


def _g711_alaw(s):
    """ITU-T G.711 A-law from 16-bit linear: 13-bit magnitude (one's complement for negative values), segment from the table of
    segment ends, 4 mantissa bits, even bits inverted (XOR 0x55; the sign bit is set for non-negative values)."""
    v = np.asarray(s, dtype=np.int64) >> 3
    mask = np.where(v >= 0, 0xD5, 0x55)
    v = np.where(v >= 0, v, -v - 1)
    seg = np.searchsorted(np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]), v, side="left")
    mant = np.where(seg < 2, (v >> 1) & 0x0F, (v >> np.maximum(seg, 1)) & 0x0F)
    return (((seg << 4) | mant) ^ mask).astype(np.uint8)


def _mulaw_decode(u):
    u = ~np.asarray(u, dtype=np.int64) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def _alaw_decode(a):
    a = np.asarray(a, dtype=np.int64) ^ 0x55
    seg, t = (a & 0x70) >> 4, (a & 0x0F) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t)


def test_numpy_g711_reference_is_sound():
    s = np.arange(-32768, 32768)
    assert _g711_mulaw([0, 32767, -32768]).tolist() == [0xFF, 0x80, 0x00]
    assert _g711_alaw([0, 32767, -32768]).tolist() == [0xD5, 0xAA, 0x2A]
    for enc, dec in ((_g711_mulaw, _mulaw_decode), (_g711_alaw, _alaw_decode)):
        d = dec(enc(s))
        assert np.all(np.diff(d) >= 0) and len(np.unique(enc(s))) >= 255
        assert np.abs(d - s).max() <= 1024 + 132          # half the coarsest step (+ mu-law's clip at 32635)


def test_encoders_at_equal_rates():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-1.5, 1.5, 5000), [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.99999, -0.99999, 1e-6, -1e-6, 3.0e4, -3.0e4],
                        (np.arange(-32768, 32768) + rng.uniform(0.01, 0.99, 65536)) / 32768.0]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    assert torch.equal(_one_push((1, 1), "f32", xd), xd)
    s16 = _one_push((1, 1), "s16", xd).cpu().numpy()
    assert s16.tobytes() == audio_io.to_pcm16(x)
    grid = (np.arange(-32768, 32768) / 32768.0).astype(np.float32)
    gd = torch.from_numpy(grid).cuda()
    assert _one_push((1, 1), "s16", gd).cpu().numpy().tolist() == list(range(-32768, 32768))
    for both in (xd, gd):
        lin = _one_push((1, 1), "s16", both).cpu().numpy()
        assert np.array_equal(_one_push((1, 1), "mulaw", both).cpu().numpy(), _g711_mulaw(lin))
        assert np.array_equal(_one_push((1, 1), "alaw", both).cpu().numpy(), _g711_alaw(lin))


# ---- 4. unaligned output -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,offsets", [("s16", (1, 3)), ("mulaw", (1, 2, 3)), ("alaw", (3,))])
def test_unaligned_output(fmt, offsets):
    """written at an odd element offset (s16) / at byte offsets 1, 2, 3 (G.711): the aligned result, and not a byte around it"""
    _x, xd = _signal()
    for ratio in ((1, 3), (147, 80)):
        want = _one_push(ratio, fmt, xd)
        n, esz = want.numel(), want.element_size()
        for off in offsets:
            for cuts in ([], [5, 1234]):
                buf = torch.full(((n + 64) * esz,), 0xA5, dtype=torch.uint8, device="cuda")
                st, at, wrote = _Stage(ratio, fmt), 0, 0
                for s in cuts + [N_IN - sum(cuts)]:
                    final = at + s == N_IN
                    cap = st.count(at + s, final) - wrote
                    rc, k = st.raw_push(xd[at:at + s], final, buf.data_ptr() + (off + wrote) * esz, cap)
                    assert rc == 0 and k == cap
                    at, wrote = at + s, wrote + k
                assert wrote == n
                got = buf.cpu()
                assert torch.equal(got[off * esz:(off + n) * esz], want.cpu().view(torch.uint8)), (fmt, ratio, off, cuts)
                assert bool((got[:off * esz] == 0xA5).all()) and bool((got[(off + n) * esz:] == 0xA5).all())


# ---- 5. reuse ----------------------------------------------------------------------------------------------------------------------
def test_reset_final_and_capacity():
    _x, xd = _signal()
    ratio = (147, 80)
    st = _Stage(ratio, "s16")
    a = torch.cat([st.push(xd[:1000]), st.push(xd[1000:3000], final=True)])
    rc, _ = st.raw_push(xd[:10], False, a.data_ptr(), a.numel())
    assert rc == _lib.FQ3_ESTATE                              # a push after `final`
    st.reset()
    second = torch.flip(xd, [0])[:3001].contiguous()
    b = torch.cat([st.push(second[:77]), st.push(second[77:], final=True)])
    assert torch.equal(b, _one_push(ratio, "s16", second))
    assert torch.equal(a, _one_push(ratio, "s16", xd[:3000]))
    # a capacity below the count: FQ3_EINVAL, nothing launched, the stream goes on as if the call had not been made
    st.reset()
    need = st.count(2000, False)
    buf = torch.full((need + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
    rc, _ = st.raw_push(xd[:2000], False, buf.data_ptr(), need - 1)
    assert rc == _lib.FQ3_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0x5A5A).all())
    c = torch.cat([st.push(xd[:2000]), st.push(xd[2000:], final=True)])
    assert torch.equal(c, _one_push(ratio, "s16", xd))


def test_python_object_and_one_shot():
    x, xd = _signal()
    for rate, enc in ((8000, "mulaw"), (44100, "s16"), (None, "s16"), (48000, "f32")):
        spec = ao.AudioOutSpec(rate, enc)
        whole = ao.AudioOut(spec, 24000, "cuda").push(xd, final=True)
        st = ao.AudioOut(spec, 24000, "cuda", stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        parts = [st.push(xd[:100]), st.push(xd[100:100]), st.push(xd[100:4000]), st.push(xd[4000:]), st.push(None, final=True)]
        assert st.out_rate == (rate or 24000) and whole.dtype == FORMATS[enc][1]
        torch.cuda.synchronize()
        assert torch.equal(torch.cat(parts), whole)
        with pytest.raises(_lib.Fq3Error):
            st.push(xd[:4])
        st.reset()
        again = st.push(xd, final=True)
        torch.cuda.synchronize()          # the stage ran on its own stream
        assert torch.equal(again, whole)
    y = ao.resample_device(x, 24000, 16000, "cuda")
    assert y.dtype == np.float32 and len(y) == -((-N_IN * 2) // 3)
    assert np.array_equal(y, _one_push((2, 3), "f32", xd).cpu().numpy())
    # against the host resampler (another filter, same alignment): where the sweep is below 0.75 of the output Nyquist both are in
    # their passbands -- the host filter deviates by up to 0.018 dB = 0.21 %, this one by 0.01 %, of an amplitude of 0.9
    ref = audio_io.resample(x, 24000, 16000)
    assert np.abs(y[1700:2400] - ref[1700:2400]).max() < 0.9 * 0.0025


# ---- 6. through the public API -----------------------------------------------------------------------------------------------------
def _tiny_model():
    from fq3hip.config import tiny_test_config
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = copy.deepcopy(tiny_test_config())
    cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "1b7"
    cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "text", "codec"))
    return FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, max_frames=48, codec_max_frames=64)


def test_public_api_opt_in():
    m = _tiny_model()
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    text = "the quick brown fox jumps over the lazy dog"
    greedy = dict(do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0, chunk_size=4)

    def run(n_frames, **ctx):
        kw = dict(greedy, max_new_tokens=n_frames, min_new_tokens=n_frames)
        gen = lambda: [(np.asarray(a).copy(), sr, tm) for a, sr, tm in  # noqa: E731
                       m.generate_custom_voice_streaming(text, "bob", "English", non_streaming_mode=False, **kw)]
        if not ctx:
            return gen()
        with m.audio_output(**ctx):
            return gen()

    for n_frames in (30, 32):       # a trailing partial chunk (marked final) / an utterance that ends on a full chunk (the tail follows)
        plain = run(n_frames)
        assert all(sr == 24000 and a.dtype == np.float32 for a, sr, _ in plain)
        pcm = torch.from_numpy(np.concatenate([a for a, _, _ in plain])).cuda()
        for rate, enc in ((8000, "mulaw"), (44100, "s16")):
            got = run(n_frames, sample_rate=rate, encoding=enc)
            assert all(sr == rate for _, sr, _ in got) and got[-1][2]["is_final"]
            assert sum(tm["chunk_steps"] for _, _, tm in got) == n_frames
            want = ao.AudioOut(ao.AudioOutSpec(rate, enc), 24000, "cuda").push(pcm, final=True).cpu().numpy()
            cat = np.concatenate([a for a, _, _ in got])
            assert cat.dtype == want.dtype and np.array_equal(cat, want), (n_frames, rate, enc, len(cat), len(want))
        again = run(n_frames)
        assert len(again) == len(plain) and all(np.array_equal(a, b) and sa == sb for (a, sa, _), (b, sb, _) in zip(again, plain))

    kw = dict(greedy, max_new_tokens=30, min_new_tokens=30)
    # incremental text and the one-shot entry point take the same route
    pieces = [text[i:i + 5] for i in range(0, len(text), 5)]
    plain = np.concatenate([np.asarray(a) for a, _, _ in m.stream_custom_voice(iter(pieces), "bob", "English", **kw)])
    with m.audio_output(8000, "alaw"):
        got = [(np.asarray(a).copy(), sr) for a, sr, _ in m.stream_custom_voice(iter(pieces), "bob", "English", **kw)]
    want = ao.AudioOut(ao.AudioOutSpec(8000, "alaw"), 24000, "cuda").push(torch.from_numpy(plain).cuda(), final=True).cpu().numpy()
    assert all(sr == 8000 for _, sr in got) and np.array_equal(np.concatenate([a for a, _ in got]), want)
    kw.pop("chunk_size")
    full, sr = m.generate_custom_voice(text, "bob", "English", **kw)
    assert sr == 24000 and full[0].dtype == np.float32
    with m.audio_output(16000, "s16"):
        enc, sr = m.generate_custom_voice(text, "bob", "English", **kw)
        with pytest.raises(ValueError):
            m.generate_custom_voice_batch([text, text], "bob", "English", lanes=2, **kw)
    want = ao.AudioOut(ao.AudioOutSpec(16000, "s16"), 24000, "cuda").push(torch.from_numpy(full[0]).cuda(), final=True).cpu().numpy()
    assert sr == 16000 and np.array_equal(enc[0], want)
    with pytest.raises(ValueError):
        with m.audio_output(24001, "s16"):
            pass
    with pytest.raises(ValueError):
        with m.audio_output(8000, "opus"):
            pass
    assert m._audio_spec is None
    full2, sr2 = m.generate_custom_voice(text, "bob", "English", **kw)
    assert sr2 == 24000 and np.array_equal(full2[0], full[0])
