"""GPU: the FLAC output stage (csrc/flac_kernels.cuh behind fq3_flac_*) through ctypes, and through the
public API.

Lossless has one meaning here: the device's bytes ARE the reference encoder's bytes (tests/_flac_ref.py implements the format subset
and the selection rule literally), and the independent decoder turns them back into the input.  Every comparison is exact."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _flac_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao

_cache = {}


def _signal(n):
    """the signal set (every subframe type, several orders, partition orders and Rice parameters), cut or repeated to n samples"""
    if "set" not in _cache:
        s = R.signal_set(1152)
        s.setflags(write=False)
        _cache["set"] = s
    x = np.resize(_cache["set"], n)
    return x, torch.from_numpy(x.copy()).cuda()


def _reference(x, rate, block):
    """the reference encoder's frames, computed once per (signal, rate, block)"""
    key = (x.tobytes(), rate, block)
    if key not in _cache:
        stats = []
        _cache[key] = (R.encode_frames(x, rate, block, stats), stats)
    return _cache[key]


class _Stage:
    """fq3_flac_* through ctypes, on the current stream"""

    def __init__(self, rate, block=0):
        self.lib = _lib.load()
        self.rate = rate
        self.h = C.c_void_p()
        cfg = _lib.FlacConfig(rate, block)
        assert self.lib.fq3_flac_create(C.byref(cfg), C.byref(self.h)) == 0, self.lib.fq3_last_error()
        b, m = C.c_int(), C.c_int()
        assert self.lib.fq3_flac_design(rate, block, C.byref(b), C.byref(m)) == 0
        self.block, self.bound = b.value, m.value
        assert self.bound == 2 * self.block + 18
        self.n_in = 0

    def __del__(self):
        self.lib.fq3_flac_destroy(self.h)

    def frames(self, n_in, final):
        return self.lib.fq3_flac_count(self.rate, self.block, n_in, 1 if final else 0)

    def raw_push(self, x, final, out_ptr, cap, nbytes):
        n = C.c_int64(-1)
        s = torch.cuda.current_stream().cuda_stream
        rc = self.lib.fq3_flac_push(self.h, C.c_void_p(x.data_ptr() if x.numel() else None), x.numel(), 1 if final else 0,
                                    C.c_void_p(out_ptr), cap, C.byref(n), C.c_void_p(nbytes.data_ptr()), C.c_void_p(s))
        return rc, n.value

    def push(self, x, final=False, offset=0):
        """-> the bytes this push completes (host uint8 array); the buffer around them must stay untouched"""
        want = self.frames(self.n_in + x.numel(), final) - self.frames(self.n_in, False)
        cap = want * self.bound
        buf = torch.full((cap + offset + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        nbytes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        rc, n = self.raw_push(x, final, buf.data_ptr() + offset if cap else None, cap, nbytes)
        assert rc == 0 and n == want, (rc, n, want, self.lib.fq3_last_error())
        self.n_in += x.numel()
        got, total = buf.cpu().numpy(), int(nbytes.item())
        assert 0 <= total <= cap
        assert np.all(got[:offset] == 0xA5) and np.all(got[offset + total:] == 0xA5)
        return got[offset:offset + total]

    def reset(self):
        assert self.lib.fq3_flac_reset(self.h, None) == 0
        self.n_in = 0


# ---- 1. the device's bytes are the reference encoder's bytes -----------------------------------------------------------------------
CASES = [(24000, 256, 4801), (24000, 1152, 3000), (24000, 4608, 4801), (24000, 1000, 2500), (11025, 0, 1500), (48000, 0, 1152 * 12)]


@pytest.mark.parametrize("rate,block,n", CASES, ids=lambda v: str(v))
def test_device_bytes_equal_the_reference(rate, block, n):
    """final blocks of 193 (block-size code 0110) and 696 (0111), the largest block, a block size and a rate without a table code, and
    the whole signal set at the default block: every subframe type, several orders, partition orders and Rice parameters"""
    x, xd = _signal(n)
    st = _Stage(rate, block)
    want, stats = _reference(x, rate, st.block)
    got = st.push(xd, final=True).tobytes()
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError(f"{len(got)} bytes, reference {len(want)}; first difference at byte {at}; choices {stats}")
    y, info = R.decode(R.stream_header(rate, st.block, n) + got)
    assert np.array_equal(y, x) and info["rate"] == rate and info["block"] == st.block
    assert len(info["frames"]) == -(-n // st.block) and info["frames"][-1]["n"] == n - (len(info["frames"]) - 1) * st.block
    assert all(f["bytes"] <= 2 * f["n"] + 18 for f in info["frames"])
    if n == 1152 * 12:
        kinds = {f["kind"] for f in info["frames"]}
        assert kinds == {"constant", "verbatim", "fixed"}


def test_two_byte_frame_numbers_and_a_second_launch_pair():
    """more than 128 frames at B = 16: the frame number takes two bytes, and the push takes more than one launch pair of 64 frames"""
    x, xd = _signal(16 * 150 + 5)
    st = _Stage(16000, 16)
    got = st.push(xd, final=True).tobytes()
    assert got == _reference(x, 16000, 16)[0]
    y, info = R.decode(R.stream_header(16000, 16) + got)
    assert np.array_equal(y, x) and len(info["frames"]) == 151


# ---- 2. the cut does not matter ----------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_cut():
    x, xd = _signal(4801)
    for block in (256, 1152):
        whole = _reference(x, 24000, block)[0]
        st = _Stage(24000, block)
        parts = [st.push(xd[:100]), st.push(xd[100:100]), st.push(xd[100:4000]), st.push(xd[4000:]), st.push(xd[:0], final=True)]
        assert len(parts[1]) == 0 and len(parts[0]) == 0
        assert b"".join(p.tobytes() for p in parts) == whole, block
    # a multiple of the block and an empty final push: the final push completes nothing
    x, xd = _signal(1152 * 3)
    st = _Stage(24000)
    a, b = st.push(xd), st.push(xd[:0], final=True)
    assert len(b) == 0 and a.tobytes() == _reference(x, 24000, 1152)[0]


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_output(offset):
    x, xd = _signal(3000)
    st = _Stage(24000, 576)
    got = st.push(xd[:1700], offset=offset).tobytes() + st.push(xd[1700:], final=True, offset=offset).tobytes()
    assert got == _reference(x, 24000, 576)[0]


# ---- 3. reuse ----------------------------------------------------------------------------------------------------------------------
def test_reset_final_and_capacity():
    x, xd = _signal(3000)
    st = _Stage(24000, 576)
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = st.push(xd[:1000]).tobytes() + st.push(xd[1000:], final=True).tobytes()
    buf = torch.empty(4 * st.bound, dtype=torch.uint8, device="cuda")
    rc, _ = st.raw_push(xd[:10], False, buf.data_ptr(), buf.numel(), nbytes)
    assert rc == _lib.FQ3_ESTATE                              # a push after `final`
    st.reset()
    second = np.ascontiguousarray(x[::-1][:2001])
    sd = torch.from_numpy(second).cuda()
    b = st.push(sd[:77]).tobytes() + st.push(sd[77:], final=True).tobytes()
    assert b == R.encode_frames(second, 24000, 576) and a == _reference(x, 24000, 576)[0]
    # a capacity below the bound: FQ3_EINVAL, nothing launched, the stream goes on as if the call had not been made
    st.reset()
    need = st.frames(2000, False) * st.bound
    buf = torch.full((need + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    nbytes.fill_(-3)
    rc, _ = st.raw_push(xd[:2000], False, buf.data_ptr(), need - 1, nbytes)
    assert rc == _lib.FQ3_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all()) and int(nbytes.item()) == -3
    c = st.push(xd[:2000]).tobytes() + st.push(xd[2000:], final=True).tobytes()
    assert c == _reference(x, 24000, 576)[0]
    # null arguments are answered before any launch
    rc = st.lib.fq3_flac_push(st.h, None, 0, 0, None, 0, C.byref(C.c_int64()), None, None)
    assert rc == _lib.FQ3_EINVAL


def test_python_object():
    """AudioOut("flac") = the s16 stage, then the FLAC stage: decodes to what the s16 encoding yields, however the stream is cut"""
    rng = np.random.default_rng(5)
    t = np.arange(9000) / 24000.0
    pcm = (0.4 * np.sin(2 * np.pi * 220.0 * t) * np.hanning(9000) + 0.01 * rng.standard_normal(9000)).astype(np.float32)
    pd = torch.from_numpy(pcm).cuda()
    for rate in (None, 8000):
        s16 = ao.AudioOut(ao.AudioOutSpec(rate, "s16"), 24000, "cuda").push(pd, final=True).cpu().numpy()
        st = ao.AudioOut(ao.AudioOutSpec(rate, "flac"), 24000, "cuda", stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        parts = [st.push(pd[:100]), st.push(pd[100:5000]), st.push(None, final=True)]
        assert all(p.dtype == torch.uint8 and p.is_cuda for p in parts)
        body = b"".join(p.cpu().numpy().tobytes() for p in parts)
        want = ao.AudioOut(ao.AudioOutSpec(rate, "s16"), 24000, "cuda").push(pd[:5000], final=True).cpu().numpy()
        assert st.n_out == len(body) and st.n_samples == len(want)
        y, info = R.decode(st.header() + body)
        assert np.array_equal(y, want) and info["total"] == 0 and info["rate"] == (rate or 24000)
        with pytest.raises(_lib.Fq3Error):
            st.push(pd[:4])
        st.reset()
        whole = st.push_host(pd, final=True)
        y, info = R.decode(st.header(len(s16)) + whole.tobytes())
        assert np.array_equal(y, s16) and info["total"] == len(s16)
        assert len(whole) < 2 * len(s16)                       # a sine under a little noise compresses


# ---- 4. through the public API -----------------------------------------------------------------------------------------------------
def _tiny_model():
    from fq3hip.config import tiny_test_config
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = copy.deepcopy(tiny_test_config())
    cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "1b7"
    cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "text", "codec"))
    return FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, max_frames=48, codec_max_frames=64)


def test_public_api_flac():
    m = _tiny_model()
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    text = "the quick brown fox jumps over the lazy dog"
    greedy = dict(do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0, chunk_size=4)

    def run(n_frames, **ctx):
        kw = dict(greedy, max_new_tokens=n_frames, min_new_tokens=n_frames)
        with m.audio_output(**ctx):
            return [(np.asarray(a).copy(), sr, tm) for a, sr, tm in
                    m.generate_custom_voice_streaming(text, "bob", "English", non_streaming_mode=False, **kw)]

    for n_frames in (30, 32):       # a trailing partial chunk (marked final) / an utterance that ends on a full chunk (the tail follows)
        for ctx in (dict(sample_rate=8000, speed=1.25), dict(sample_rate=None)):
            rate = ctx["sample_rate"] or 24000
            want = np.concatenate([a for a, _, _ in run(n_frames, encoding="s16", **ctx)])
            got = run(n_frames, encoding="flac", **ctx)
            assert all(a.dtype == np.uint8 and sr == rate for a, sr, _ in got) and got[-1][2]["is_final"]
            assert sum(tm["chunk_steps"] for _, _, tm in got) == n_frames
            assert got[0][0][:42].tobytes() == R.stream_header(rate, 0, 0)
            y, info = R.decode(np.concatenate([a for a, _, _ in got]).tobytes())
            assert info["rate"] == rate and info["total"] == 0
            assert y.dtype == want.dtype and np.array_equal(y, want), (n_frames, ctx, len(y), len(want))

    kw = dict(greedy, max_new_tokens=30, min_new_tokens=30)
    kw.pop("chunk_size")
    with m.audio_output(16000, "s16"):
        s16, _ = m.generate_custom_voice(text, "bob", "English", **kw)
    with m.audio_output(16000, "flac"):
        enc, sr = m.generate_custom_voice(text, "bob", "English", **kw)
        with pytest.raises(ValueError):
            m.generate_custom_voice_batch([text, text], "bob", "English", lanes=2, **kw)
    assert sr == 16000 and enc[0].dtype == np.uint8
    y, info = R.decode(enc[0].tobytes())
    assert info["total"] == len(s16[0]) and np.array_equal(y, s16[0])       # the one-shot header carries the total
    assert m._audio_spec is None
