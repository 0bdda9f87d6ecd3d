"""GPU: the time-scale stage (csrc/tsm_kernels.cuh behind fq3_tsm_*) through ctypes, chained in ``AudioOut``,
and through the public API.

Three halves of one contract.  Search: the delta the device chose for every segment is, in a float64 evaluation of all 481 candidates
against the device's own previous position, within the error of two length-N fp32 dot products of the best.  Samples: the overlap-add
against float64, per sample.  Identity: the result (samples AND deltas) does not depend on how the stream was cut into pushes, on
whether the object is fresh, or on where the output buffer starts -- ``torch.equal``, no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _tsm_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao

HS, N, DELTA = R.HS, R.N, R.DELTA
_dev = {}


def _signal():
    x = R.signal()
    if "x" not in _dev:
        _dev["x"] = torch.from_numpy(x.copy()).cuda()
    return x, _dev["x"]


class _Tsm:
    """fq3_tsm_* through ctypes, on the current stream"""

    def __init__(self, P, rate=R.RATE):
        self.lib, self.P, self.rate = _lib.load(), P, rate
        self.h = C.c_void_p()
        cfg = _lib.TsmConfig(rate, P)
        assert self.lib.fq3_tsm_create(C.byref(cfg), C.byref(self.h)) == 0, self.lib.fq3_last_error()
        self.n_in = self.n_out = 0

    def __del__(self):
        self.lib.fq3_tsm_destroy(self.h)

    def count(self, n_in, final):
        return self.lib.fq3_tsm_count(self.rate, self.P, n_in, 1 if final else 0)

    def raw_push(self, x, final, out_ptr, cap, d_ptr=None, d_cap=0):
        n = C.c_int64(-1)
        s = torch.cuda.current_stream().cuda_stream
        rc = self.lib.fq3_tsm_push(self.h, C.c_void_p(x.data_ptr() if x.numel() else None), x.numel(), 1 if final else 0,
                                   C.c_void_p(out_ptr), cap, C.byref(n), C.c_void_p(d_ptr), d_cap, C.c_void_p(s))
        return rc, n.value

    def push(self, x, final=False):
        """-> (samples, deltas) this push emitted"""
        cap = self.count(self.n_in + x.numel(), final) - self.n_out
        n_seg = -(-cap // HS)
        out = torch.empty(cap, dtype=torch.float32, device="cuda")
        d = torch.full((n_seg,), 12345, dtype=torch.int32, device="cuda")
        rc, n = self.raw_push(x, final, out.data_ptr() if cap else None, cap, d.data_ptr() if n_seg else None, n_seg)
        assert rc == 0 and n == cap, (rc, n, cap, self.lib.fq3_last_error())
        self.n_in += x.numel()
        self.n_out += cap
        return out, d

    def reset(self):
        assert self.lib.fq3_tsm_reset(self.h, None) == 0
        self.n_in = self.n_out = 0


_whole = {}


def _one_push(P):
    """(samples, deltas) of the test signal in one final push, as device tensors (made once per speed, never modified)"""
    if P not in _whole:
        _x, xd = _signal()
        _whole[P] = _Tsm(P).push(xd, final=True)
    return _whole[P]


def _pushes(st, xd, sizes, final_empty=False):
    at, ys, ds = 0, [], []
    for s in sizes:
        y, d = st.push(xd[at:at + s])
        at += s
        S = st.n_out // HS                                     # the library's count against the need rule and the cap
        assert st.n_out % HS == 0 and (S == 0 or R.need(S - 1, st.P) <= at)
        assert R.need(S, st.P) > at or (S + 1) * HS > R.total(at, st.P)
        ys.append(y)
        ds.append(d)
    if final_empty:
        y, d = st.push(xd[at:])
        ys.append(y)
        ds.append(d)
        at = xd.numel()
    y, d = st.push(xd[at:], final=True)
    return torch.cat(ys + [y]), torch.cat(ds + [d])


# ---- 1. the search, teacher-forced against float64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [500, 800, 1250, 2000, 4000])
def test_search_against_float64(P):
    """c64(delta_dev) >= max c64 - B with B = 2 (N + 2) 2^-24 max_delta sum_j |x t|: (N + 2) 2^-24 bounds a length-N fp32 dot product,
    winner and runner-up each carry it.  At most one segment may differ from the float64 argmax at all; exact ties (the zeros past the
    end) go to the smallest delta; segment 0 has delta 0."""
    x, _xd = _signal()
    y, d = _one_push(P)
    d = d.cpu().numpy().astype(np.int64)
    T = R.total(len(x), P)
    assert y.numel() == T and len(d) == -(-T // HS)
    assert d[0] == 0 and np.all(np.abs(d) <= DELTA)
    prev, differ, worst, zero_tie = 0, 0, 0.0, 0
    for s in range(1, len(d)):
        c64, a64 = R.correlations(x, s, P, prev)
        best = int(np.argmax(c64))                             # first maximum: the smallest delta among exact ties
        got = int(d[s]) + DELTA
        B = 2 * (N + 2) * 2.0 ** -24 * a64.max()
        assert c64[got] >= c64[best] - B, (P, s, got - DELTA, best - DELTA, c64[best] - c64[got], B)
        if c64[got] == c64[best]:
            assert got == best, (P, s, got - DELTA, best - DELTA)          # a float64 tie resolves to the smallest delta
        differ += got != best
        if B > 0:
            worst = max(worst, (c64[best] - c64[got]) / B)
        if a64.max() == 0.0:
            zero_tie += 1
            assert d[s] == -DELTA
        prev = R.a_of(s, P) + int(d[s])
    print(f"P {P}: {len(d)} segments, {differ} differ from the float64 argmax, worst gap / B {worst:.3f}, all-zero segments {zero_tie}")
    assert differ <= 1


def test_exact_ties_go_to_the_smallest_delta():
    """where every candidate is zero (here: 3000 samples of silence behind the signal, and the zeros past the end) all 481 correlations
    tie exactly, and delta is -DELTA"""
    _x, xd = _signal()
    x = torch.cat([xd[:3000], torch.zeros(3000, device="cuda")])
    _y, d = _Tsm(1250).push(x, final=True)
    d = d.cpu().numpy()
    silent = [s for s in range(1, len(d)) if R.a_of(s, 1250) - DELTA >= 3000]
    assert len(silent) >= 5 and all(d[s] == -DELTA for s in silent), d[-12:]


# ---- 2. the samples against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [500, 800, 1250, 2000, 4000])
def test_samples_against_float64(P):
    """|y - y_ref| <= 3 2^-24 (|w[j] x1| + |w[j + Hs] x0|): two roundings (the product, the fused add) and one for the reference, with
    the device's deltas and the library's float32 window"""
    x, _xd = _signal()
    y, d = _one_push(P)
    w = ao.tsm_design(R.RATE, P)[3].astype(np.float64)
    ref, _ = R.wsola(x, P, w=w, deltas=d.cpu().numpy())
    mag, _ = R.wsola(np.abs(x), P, w=np.abs(w), deltas=d.cpu().numpy())          # |w1 x1| + |w0 x0| at the same positions
    got = y.cpu().numpy().astype(np.float64)
    assert len(got) == len(ref) == R.total(len(x), P)
    err, bound = np.abs(got - ref), 3 * 2.0 ** -24 * mag
    print(f"P {P}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-30)):.3f}")
    assert np.all(err <= bound), (int(np.argmax(err - bound)), float(err.max()))
    assert np.abs(ref).max() > 0.3                             # the comparison is not about silence


# ---- 3. the cut does not matter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [500, 1500])
def test_result_does_not_depend_on_the_cut(P):
    _x, xd = _signal()
    y, d = _one_push(P)
    n = xd.numel()
    cuts = [1, HS - 1, HS, N + DELTA - 1, N + DELTA, N + DELTA + 1, 5000]
    sizes = [b - a for a, b in zip([0] + cuts[:-1], cuts)]
    plans = {"97s": ([97] * (n // 97), False), "edges": (sizes, False), "empty in the middle": ([3000, 0, 4000], False),
             "final without samples": ([7000, 8000], True)}
    st = _Tsm(P)
    for name, (sz, final_empty) in plans.items():
        st.reset()                                             # ... and a reused object is a fresh one
        yy, dd = _pushes(st, xd, sz, final_empty)
        assert torch.equal(yy, y) and torch.equal(dd, d), (P, name)
    fresh = _pushes(_Tsm(P), xd, [97] * 40)
    assert torch.equal(fresh[0], y) and torch.equal(fresh[1], d)
    # many of the 97-sample pushes emit nothing
    st.reset()
    assert [st.push(xd[i * 97:(i + 1) * 97])[0].numel() for i in range(12)].count(0) >= 6
    # an output buffer at an odd element offset
    buf = torch.full((y.numel() + 9,), 7.0, dtype=torch.float32, device="cuda")
    st.reset()
    rc, k = st.raw_push(xd, True, buf.data_ptr() + 4 * 3, y.numel())
    assert rc == 0 and k == y.numel()
    assert torch.equal(buf[3:3 + k], y) and bool((buf[:3] == 7.0).all()) and bool((buf[3 + k:] == 7.0).all())


# ---- 4. the chain -----------------------------------------------------------------------------------------------------------------
def test_chain_with_the_output_stage():
    _x, xd = _signal()
    spec = ao.AudioOutSpec(8000, "mulaw", speed=1.25)
    y, _d = _one_push(1250)
    want = ao.AudioOut(ao.AudioOutSpec(8000, "mulaw"), R.RATE, "cuda").push(y, final=True)
    whole = ao.AudioOut(spec, R.RATE, "cuda")
    got = whole.push(xd, final=True)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert whole.n_in == xd.numel() and whole.n_out == got.numel() and whole.finished
    st = ao.AudioOut(spec, R.RATE, "cuda")
    parts = [st.push(xd[:100]), st.push(xd[100:100]), st.push(xd[100:4000]), st.push(xd[4000:19999]), st.push(xd[19999:]),
             st.push(None, final=True)]
    assert torch.equal(torch.cat(parts), want) and st.n_out == want.numel()
    with pytest.raises(_lib.Fq3Error):
        st.push(xd[:4])
    st.reset()
    assert torch.equal(torch.cat([st.push(xd[:7777]), st.push(xd[7777:], final=True)]), want)
    # speed alone: the time-scale stage's float32, no second launch; and into a caller's buffer
    only = ao.AudioOut(ao.AudioOutSpec(speed=1.25), R.RATE, "cuda")
    buf = torch.zeros(y.numel() + 5, dtype=torch.float32, device="cuda")
    assert torch.equal(only.push_into(xd, True, buf), y) and only.out_rate == R.RATE
    with pytest.raises(_lib.Fq3Error):
        only.push(xd[:4])
    # 1.0 is no stage at all
    for rate, enc in ((8000, "mulaw"), (None, "f32")):
        a = ao.AudioOut(ao.AudioOutSpec(rate, enc, speed=1.0), R.RATE, "cuda")
        b = ao.AudioOut(ao.AudioOutSpec(rate, enc), R.RATE, "cuda")
        assert a._tsm is None and torch.equal(a.push(xd, final=True), b.push(xd, final=True))


# ---- 5. pitch stays, duration scales ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [500, 800, 1250, 1500, 2000])
def test_pitch_stays_and_duration_scales(P):
    t = np.arange(24000) / 24000.0
    x = (0.8 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32)
    y, _d = _Tsm(P).push(torch.from_numpy(x).cuda(), final=True)
    y = y.cpu().numpy().astype(np.float64)
    assert len(y) == R.total(24000, P)
    core = y[1000:-1500]
    spec = np.abs(np.fft.rfft(core * np.hanning(len(core)))) ** 2
    k = int(np.argmax(spec))
    peak = k * 24000.0 / len(core)
    frac = spec[max(k - 3, 0):k + 4].sum() / spec.sum()
    rms = float(np.sqrt(np.mean(core ** 2)))
    print(f"P {P}: peak {peak:.2f} Hz, energy within 3 bins {frac:.6f}, rms {rms:.5f}")
    assert abs(peak - 200.0) <= 2.0                            # plain resampling would put it at 200 * speed
    assert frac >= 0.999
    assert abs(rms - 0.8 / np.sqrt(2.0)) <= 0.01 * 0.8 / np.sqrt(2.0)


# ---- 6. state errors --------------------------------------------------------------------------------------------------------------
def test_state_errors():
    _x, xd = _signal()
    st = _Tsm(1250)
    y, _ = st.push(xd[:5000], final=True)
    rc, _ = st.raw_push(xd[:10], False, y.data_ptr(), y.numel())
    assert rc == _lib.FQ3_ESTATE                               # a push after `final`
    st.reset()
    need = st.count(5000, False)
    assert need > 0
    buf = torch.full((need + 8,), -3.0, dtype=torch.float32, device="cuda")
    rc, _ = st.raw_push(xd[:5000], False, buf.data_ptr(), need - 1)
    assert rc == _lib.FQ3_EINVAL
    d = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc, _ = st.raw_push(xd[:5000], False, buf.data_ptr(), need, d.data_ptr(), need // HS - 1)
    assert rc == _lib.FQ3_EINVAL                               # room for fewer deltas than segments
    torch.cuda.synchronize()
    assert bool((buf == -3.0).all())                           # nothing was launched
    # ... and the stream goes on as if the calls had not been made
    a, da = st.push(xd[:5000])
    b, db = st.push(xd[5000:], final=True)
    want = _one_push(1250)
    assert torch.equal(torch.cat([a, b]), want[0]) and torch.equal(torch.cat([da, db]), want[1])


# ---- 7. through the public API ----------------------------------------------------------------------------------------------------
def test_public_api_speed():
    from fq3hip.config import tiny_test_config
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = tiny_test_config()
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "text", "codec"))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, max_frames=48, codec_max_frames=64)
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    g = torch.Generator().manual_seed(5)
    vcp = dict(ref_code=[None], ref_spk_embedding=[torch.randn(cfg.talker.hidden_size, generator=g).cuda()],
               x_vector_only_mode=[True], icl_mode=[False])
    kw = dict(text="the quick brown fox jumps over the lazy dog", language="English", voice_clone_prompt=vcp, do_sample=False,
              temperature=1.0, top_k=0, repetition_penalty=1.0, max_new_tokens=22, min_new_tokens=22, non_streaming_mode=False)

    def stream():
        return [(np.asarray(a).copy(), sr, tm) for a, sr, tm in m.generate_voice_clone_streaming(chunk_size=4, **kw)]

    full, sr = m.generate_voice_clone(**kw)
    assert sr == 24000 and full[0].dtype == np.float32
    plain = stream()
    with m.audio_output(speed=1.5) as spec:
        assert spec.permille == 1500
        one, sr1 = m.generate_voice_clone(**kw)
        got = stream()
        with pytest.raises(ValueError):
            m.generate_voice_clone_batch([kw["text"]] * 2, language="English", voice_clone_prompt=vcp, lanes=2, non_streaming_mode=False)
    cat = np.concatenate([a for a, _, _ in got])
    assert sr1 == 24000 and all(s == 24000 for _, s, _ in got) and got[-1][2]["is_final"]
    assert one[0].dtype == np.float32 and cat.dtype == np.float32
    assert len(one[0]) == R.total(len(full[0]), 1500)          # T of the unstretched utterance
    assert np.array_equal(cat, one[0])
    want = ao.AudioOut(ao.AudioOutSpec(speed=1.5), 24000, "cuda").push(torch.from_numpy(full[0]).cuda(), final=True).cpu().numpy()
    assert np.array_equal(one[0], want)
    with pytest.raises(ValueError):
        with m.audio_output(speed=5.0):
            pass
    # outside the context nothing changed
    assert m._audio_spec is None
    full2, sr2 = m.generate_voice_clone(**kw)
    again = stream()
    assert sr2 == 24000 and np.array_equal(full2[0], full[0])
    assert len(again) == len(plain) and all(np.array_equal(a, b) and sa == sb for (a, sa, _), (b, sb, _) in zip(again, plain))
