"""CPU: the host-only half of the audio output stage -- the polyphase filter design and the streaming output
count behind ``fq3_audio_out_design`` / ``fq3_audio_out_count`` (no HIP call), the argument errors of the C ABI, the WAV header of
the byte encodings, and the server's opt-in (``sample_rate`` / ``encoding``) over a stand-in worker."""
import ctypes as C
import queue
import struct
from math import ceil

import numpy as np
import pytest

from fq3hip import _lib, audio_io
from fq3hip import audio_out as ao

# out / in as in the issue: 1/3 is 24 kHz -> 8 kHz, 147/80 is 24 kHz -> 44.1 kHz
RATIOS = [(1, 3), (2, 3), (147, 160), (147, 80), (2, 1), (80, 147), (1, 2), (3, 2)]
Z = 16          # default zero crossings a side


def _rates(ratio):
    out, inp = ratio
    return 100 * inp, 100 * out


def _prototype(L, M, K, bank):
    """the phase rows back into the prototype: row p, tap k is prototype index (p + half) mod L + (K - 1 - k) L"""
    half = Z * max(L, M)
    h = np.zeros(K * L + L)
    for p in range(L):
        h[(p + half) % L + (K - 1 - np.arange(K)) * L] = bank[p]
    assert not h[2 * half + 1:].any()
    return h[:2 * half + 1]


def _measures(h, m):
    """(largest passband deviation over [0, 0.8 fN], response at fN, peak response at >= 1.1 fN, at >= 1.2 fN), all in dB against
    the response at 0; fN = 1 / m of the up-sampled Nyquist is the lower of the two Nyquist frequencies"""
    n = 1 << 20
    H = np.abs(np.fft.rfft(h / h.sum(), n))
    f = np.arange(H.size) / (n / 2) * m
    db = 20 * np.log10(np.maximum(H, 1e-12))
    return np.abs(db[f <= 0.8]).max(), db[np.argmin(np.abs(f - 1.0))], db[f >= 1.1].max(), db[f >= 1.2].max()


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}over{r[1]}")
def test_design_is_no_worse_than_the_host_filter(ratio):
    from scipy.signal import firwin
    L, M, K, bank = ao.design(*_rates(ratio))
    assert (L, M) == ratio and K == ceil((2 * Z * max(L, M) + 1) / L) and bank.shape == (L, K) and bank.dtype == np.float32
    m = max(L, M)
    ours = _measures(_prototype(L, M, K, bank.astype(np.float64)), m)
    host = _measures(firwin(2 * 10 * m + 1, 1.0 / m, window=("kaiser", 5.0)), m)          # scipy.signal.resample_poly's default
    print(ratio, "this design", ours, "host filter", host)
    for a, b in zip(ours, host):
        assert a <= b, (ours, host)
    assert np.abs(bank.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-3


@pytest.mark.parametrize("ratio", RATIOS + [(147, 320)], ids=lambda r: f"{r[0]}over{r[1]}")
def test_count_rules(ratio):
    i, o = _rates(ratio)
    L, M, K, _ = ao.design(i, o, bank=False)
    for N in (0, 1, 2, K - 1, K, 4801, 1 << 40):
        assert ao.count(i, o, N, True) == -((-N * L) // M)               # ceil(N L / M): scipy.signal.resample_poly's length
    look = Z * max(L, M) / M                                                # the look-ahead (Z max(1, M / L) inputs) in output samples
    prev = 0
    for n in list(range(0, 700)) + [4801, 1 << 40]:
        c0, c1 = ao.count(i, o, n, False), ao.count(i, o, n, True)
        assert prev <= c0 <= c1 and c1 - c0 <= look + 1, (n, prev, c0, c1)
        prev = c0
    # an output exists exactly when the last input it reads does: e(n) = floor((n M + Z m) / L) < n_in
    for n in (1, 50, 333, 4801):
        c0 = ao.count(i, o, n, False)
        assert c0 == 0 or (M * (c0 - 1) + Z * max(L, M)) // L < n
        assert (M * c0 + Z * max(L, M)) // L >= n


def test_equal_rates_are_the_encoder_alone():
    L, M, K, bank = ao.design(24000, 24000)
    assert (L, M, K) == (1, 1, 1) and bank.tolist() == [[1.0]]
    assert [ao.count(24000, 24000, n, False) for n in (0, 1, 5, 4801)] == [0, 1, 5, 4801]
    assert ao.count(16000, 16000, 77, True) == 77


def test_accepted_rates():
    for r in (8000, 11025, 16000, 22050, 32000, 44100, 48000):
        ao.design(24000, r, bank=False)
        ao.AudioOutSpec(r, "mulaw").validate(24000)
    for r in (44100, 48000, 16000):
        ao.design(r, 24000, bank=False)


def test_errors_are_codes_not_crashes():
    lib = _lib.load()
    L, M, K = C.c_int(), C.c_int(), C.c_int()
    assert lib.fq3_audio_out_design(24000, 24001, 0, L, M, K, None, 0) == _lib.FQ3_EINVAL          # L = 24001
    assert b"320" in lib.fq3_last_error()
    assert lib.fq3_audio_out_design(48000, 100, 0, L, M, K, None, 0) == _lib.FQ3_EINVAL            # M = 480
    assert lib.fq3_audio_out_design(0, 8000, 0, L, M, K, None, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_audio_out_design(24000, -8000, 0, L, M, K, None, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_audio_out_design(24000, 8000, 0, None, M, K, None, 0) == _lib.FQ3_EINVAL
    small = (C.c_float * 4)()
    assert lib.fq3_audio_out_design(24000, 8000, 0, L, M, K, small, 4) == _lib.FQ3_EINVAL          # bank capacity below L K
    assert lib.fq3_audio_out_count(24000, 24001, 0, 10, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_audio_out_count(24000, 8000, 0, -1, 0) == _lib.FQ3_EINVAL
    assert lib.fq3_audio_out_create(None, None) == -1
    h = C.c_void_p()
    assert lib.fq3_audio_out_create(None, C.byref(h)) == -1
    bad = _lib.AudioOutConfig(24000, 8000, 7, 0)                                                   # unknown format: before any HIP call
    assert lib.fq3_audio_out_create(C.byref(bad), C.byref(h)) == -1
    bad = _lib.AudioOutConfig(24000, 24001, 0, 0)
    assert lib.fq3_audio_out_create(C.byref(bad), C.byref(h)) == -1
    n = C.c_int64()
    assert lib.fq3_audio_out_push(None, None, 0, 0, None, 0, C.byref(n), None) == -1
    assert lib.fq3_audio_out_reset(None, None) == -1 and lib.fq3_audio_out_destroy(None) == 0
    with pytest.raises(ValueError):
        ao.AudioOutSpec(8000, "opus")
    with pytest.raises(ValueError):
        ao.AudioOutSpec(24001, "s16").validate(24000)


def test_wav_header_for():
    for r in (8000, 24000, 44100):
        assert audio_io.wav_header_for(r, "s16") == audio_io.wav_header(r)
        assert audio_io.wav_header_for(r, "s16", 1000) == audio_io.wav_header(r, 1000)
    for enc, tag in (("mulaw", 7), ("alaw", 6)):
        h = audio_io.wav_header_for(8000, enc, 4000)
        assert h[:4] == b"RIFF" and h[8:16] == b"WAVEfmt " and struct.unpack("<I", h[4:8])[0] == len(h) - 8 + 4000
        assert struct.unpack("<IHHIIHHH", h[16:38]) == (18, tag, 1, 8000, 8000, 1, 8, 0)
        assert h[38:42] == b"fact" and struct.unpack("<II", h[42:50]) == (4, 4000) and h[50:54] == b"data"
        assert struct.unpack("<I", h[54:58])[0] == 4000 and len(h) == 58
        s = audio_io.wav_header_for(8000, enc)
        assert struct.unpack("<I", s[4:8])[0] == 0xFFFFFFFF and struct.unpack("<I", s[54:58])[0] == 0xFFFFFFFF
    with pytest.raises(ValueError):
        audio_io.wav_header_for(8000, "f32")


# ---- server: both fields absent -> today's bytes; either present -> the spec reaches the worker, the reply is framed for it ----------
class _Worker:
    """Stand-in for ``BatchWorker``: answers with fixed chunks; a request with a spec gets bytes 'encoded' to its dtype."""
    DONE = None

    def __init__(self):
        self.seen = []
        self.chunks = [np.linspace(-1.2, 1.2, 700).astype(np.float32), np.full(300, 0.25, np.float32)]

    def submit(self, cfg, text):
        from fq3hip.server import BatchWorker
        self.seen.append(cfg)
        box = queue.Queue()
        spec = cfg.get("audio_output")
        for c in self.chunks:
            box.put(c if spec is None else np.arange(len(c) // 3, dtype=ao.NUMPY_DTYPES[spec.encoding]))
        box.put(BatchWorker.DONE)
        return box


class _Model:
    sample_rate = 24000


def test_server_default_reply_is_unchanged_and_opt_in_is_framed():
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app
    w = _Worker()
    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "t", "language": "English"}}
    client = TestClient(create_app(_Model(), voices, default_voice="alloy", scheduler="batch", worker=w))
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "response_format": "wav"})
    assert r.status_code == 200
    assert r.content == audio_io.wav_header(24000) + b"".join(audio_io.to_pcm16(c) for c in w.chunks)
    assert "audio_output" not in w.seen[-1] and w.seen[-1] is voices["alloy"]
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "response_format": "pcm"})
    assert r.content == b"".join(audio_io.to_pcm16(c) for c in w.chunks)

    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "response_format": "wav", "sample_rate": 8000,
                                              "encoding": "mulaw"})
    assert r.status_code == 200
    spec = w.seen[-1]["audio_output"]
    assert spec == ao.AudioOutSpec(8000, "mulaw") and "audio_output" not in voices["alloy"]
    body = r.content
    assert struct.unpack("<IHHIIHHH", body[16:38]) == (18, 7, 1, 8000, 8000, 1, 8, 0)
    assert body[:58] == audio_io.wav_header_for(8000, "mulaw")
    assert body[58:] == b"".join(np.arange(len(c) // 3, dtype=np.uint8).tobytes() for c in w.chunks)
    # a rate alone: 16-bit PCM at that rate; f32 is answered as s16
    for extra in ({"sample_rate": 16000}, {"sample_rate": 16000, "encoding": "f32"}):
        r = client.post("/v1/audio/speech", json=dict({"input": "hello", "voice": "alloy", "response_format": "wav"}, **extra))
        assert r.status_code == 200 and w.seen[-1]["audio_output"] == ao.AudioOutSpec(16000, "s16")
        assert r.content[:44] == audio_io.wav_header(16000)
        assert r.content[44:] == b"".join(np.arange(len(c) // 3, dtype="<i2").tobytes() for c in w.chunks)
    n = len(w.seen)
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "encoding": "opus"})
    assert r.status_code == 400 and "opus" in r.json()["detail"]
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "sample_rate": 24001})
    assert r.status_code == 400 and "320" in r.json()["detail"]
    r = client.post("/v1/audio/speech", json={"input": "hello", "voice": "alloy", "sample_rate": 0, "encoding": "alaw"})
    assert r.status_code == 400
    assert len(w.seen) == n                                     # refused before anything was submitted


def test_cli_flags_parse():
    from fq3hip import cli
    a = cli.build_parser().parse_args(["custom", "--text", "x", "--output", "o.wav", "--speaker", "s", "--out-rate", "8000", "--encoding", "mulaw"])
    assert a.out_rate == 8000 and a.encoding == "mulaw"
    a = cli.build_parser().parse_args(["custom", "--text", "x", "--output", "o.wav", "--speaker", "s"])
    assert a.out_rate is None and a.encoding is None
