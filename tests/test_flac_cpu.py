"""CPU: the FLAC reference (tests/_flac_ref.py: a numpy encoder that implements the emitted subset and the selection rule literally, a
pure-Python decoder that checks every CRC, frame number and reserved code), the host-only half of the C ABI (``fq3_flac_header`` /
``_design`` / ``_count``), ``AudioOutSpec("flac")``, and the server's and the CLI's contract over scripted models."""
import contextlib
import ctypes as C
import queue
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import _flac_ref as R
from fq3hip import _lib, audio_io
from fq3hip import audio_out as ao


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_crc_anchors():
    assert R.crc8(b"123456789") == 0xF4 and R.crc16(b"123456789") == 0xFEE8
    assert R.crc8(b"") == 0 and R.crc16(b"") == 0


@pytest.fixture(scope="module")
def encoded_set():
    x = R.signal_set(1152)
    x.setflags(write=False)
    stats = []
    return x, R.encode(x, 24000, stats=stats), stats


def test_signal_set_exercises_the_encoder(encoded_set):
    """a condition on the signal set, not a measurement: the reference alone must take every branch the device has to reproduce"""
    _x, _data, stats = encoded_set
    kinds = [s[0] for s in stats]
    fixed = [s for s in stats if s[0] == "fixed"]
    assert "constant" in kinds and "verbatim" in kinds
    assert len({s[1] for s in fixed}) >= 3, sorted({s[1] for s in fixed})
    porders = {s[2] for s in fixed}
    assert len(porders) >= 2 and max(porders) >= 2, sorted(porders)
    ks = {k for s in fixed for k in s[3]}
    assert 0 in ks and max(ks) >= 10 and max(ks) <= R.MAX_K, sorted(ks)


def test_decode_inverts_encode(encoded_set):
    x, data, stats = encoded_set
    y, info = R.decode(data)
    assert y.dtype == np.int16 and np.array_equal(y, x)
    assert info["rate"] == 24000 and info["block"] == 1152 and info["total"] == len(x) and len(info["frames"]) == len(stats)
    for f, s in zip(info["frames"], stats):                    # the decoder reads back what the encoder chose
        assert f["kind"] == s[0] and f["bytes"] <= 2 * f["n"] + 18
        if s[0] == "fixed":
            assert (f["order"], f["porder"], f["ks"]) == (s[1], s[2], s[3])


@pytest.mark.parametrize("rate,block,n", [(24000, 256, 4801), (24000, 1152, 3000), (8000, 4608, 4801), (16000, 1000, 2500),
                                          (11025, 0, 1500), (16000, 16, 16 * 130 + 5), (44100, 192, 193), (96000, 17, 40)])
def test_round_trip_over_block_sizes_and_rates(encoded_set, rate, block, n):
    """every block-size code (table, 0110, 0111), table rates and a 16-bit rate, two-byte frame numbers, tiny final blocks"""
    x = np.resize(encoded_set[0][2 * 1152:], n)
    data = R.encode(x, rate, block)
    y, info = R.decode(data)
    assert np.array_equal(y, x) and info["rate"] == rate and info["block"] == (block or R.default_block(rate))
    assert info["frames"][-1]["n"] == n - (len(info["frames"]) - 1) * info["block"]
    unknown = R.encode(x, rate, block, total=0)
    assert R.decode(unknown)[1]["total"] == 0 and unknown[42:] == data[42:]


def test_tiny_blocks():
    for x in ([5], [5, 5], [5, -6], [1, 2, 4], [-32768, 32767, -32768, 32767, 0]):
        x = np.array(x, dtype=np.int16)
        y, info = R.decode(R.encode(x, 8000, 16))
        assert np.array_equal(y, x)
    assert R.choose(np.array([5, -6], dtype=np.int16))[0] in ("fixed", "verbatim")


def test_decoder_rejects_what_it_must(encoded_set):
    x, data, _ = encoded_set
    good = bytearray(data[: 42 + 200])                         # header + the start of frame 0; enough for header-level checks

    def broken(at, value, fix_crc8=True, whole=False):
        b = bytearray(data if whole else good)
        b[at] = value
        if fix_crc8:
            b[42 + 5] = R.crc8(bytes(b[42: 42 + 5]))          # frame 0's header is 5 bytes + CRC-8 (table block size and rate)
        return bytes(b)

    assert data[42:44] == b"\xff\xf8" and data[42 + 5] == R.crc8(data[42:47])
    for what, stream in (("marker", b"fLaX" + data[4:]),
                         ("STREAMINFO", data[:4] + b"\x00" + data[5:]),
                         ("block size code 0000", broken(44, 0x07)),
                         ("sample rate code 1111", broken(44, 0x3F)),
                         ("reserved channel assignment", broken(45, 0xB8)),
                         ("reserved sample size", broken(45, 0x06)),
                         ("reserved header bit", broken(45, 0x09)),
                         ("frame number", broken(46, 0x01)),
                         ("CRC-8", broken(44, 0x38, fix_crc8=False)),
                         ("reserved subframe type", broken(48, 0x04)),
                         ("CRC-16", broken(len(data) - 1, data[-1] ^ 1, fix_crc8=False, whole=True)),
                         ("a flipped payload bit", broken(42 + 3 * 1200, data[42 + 3 * 1200] ^ 0x10, fix_crc8=False, whole=True)),
                         ("a truncated stream", data[:-3])):
        with pytest.raises(R.FlacError):
            R.decode(stream)
            pytest.fail(f"accepted: {what}")
    # the total in STREAMINFO must match the frames
    with pytest.raises(R.FlacError):
        R.decode(R.stream_header(24000, 1152, len(x) + 1) + data[42:])


# ---- the host-only half of the C ABI -----------------------------------------------------------------------------------------------
def test_header_design_and_count_against_struct_packed_expectations():
    lib = _lib.load()
    for rate, block, total in ((24000, 0, 0), (8000, 0, 12345), (44100, 4608, (1 << 36) - 1), (11025, 1000, 7), (96000, 16, 1)):
        b = block or (1152 if rate > 16000 else 576)
        want = (b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + struct.pack(">HH", b, b) + b"\0" * 6 +
                ((rate << 44) | (0 << 41) | (15 << 36) | total).to_bytes(8, "big") + b"\0" * 16)
        assert len(want) == 42
        assert ao.flac_header(rate, block, total) == want == audio_io.flac_header(rate, block, total) == R.stream_header(rate, block, total)
        assert ao.flac_design(rate, block) == (b, 2 * b + 18)
        for n in (0, 1, b - 1, b, b + 1, 10 * b, 10 * b + 1):
            assert ao.flac_count(rate, block, n, False) == n // b and ao.flac_count(rate, block, n, True) == -(-n // b)
    buf = (C.c_uint8 * 42)()
    blk, bound = C.c_int(), C.c_int()
    for rc in (lib.fq3_flac_header(24000, 0, 0, None, 42), lib.fq3_flac_header(24000, 0, 0, buf, 41), lib.fq3_flac_header(24000, 0, -1, buf, 42),
               lib.fq3_flac_header(24000, 0, 1 << 36, buf, 42), lib.fq3_flac_header(0, 0, 0, buf, 42), lib.fq3_flac_header(24000, 15, 0, buf, 42),
               lib.fq3_flac_header(24000, 4609, 0, buf, 42), lib.fq3_flac_header(65536, 0, 0, buf, 42),
               lib.fq3_flac_design(24000, 0, None, C.byref(bound)), lib.fq3_flac_design(100000, 0, C.byref(blk), C.byref(bound)),
               lib.fq3_flac_count(24000, 0, -1, 0), lib.fq3_flac_count(24000, 8, 100, 0)):
        assert rc == _lib.FQ3_EINVAL
    assert b"65535" in lib.fq3_last_error() or b"block" in lib.fq3_last_error()
    assert ao.flac_design(88200)[0] == 1152 and ao.flac_design(65535)[0] == 1152       # a table rate above 65535 Hz; the largest 16-bit rate
    # NULL and range errors of the object's entry points are answered before any HIP call
    h = C.c_void_p()
    assert lib.fq3_flac_create(None, C.byref(h)) == _lib.FQ3_EINVAL
    assert lib.fq3_flac_create(C.byref(_lib.FlacConfig(24000, 5000)), C.byref(h)) == _lib.FQ3_EINVAL and not h.value
    assert lib.fq3_flac_destroy(None) == 0 and lib.fq3_flac_reset(None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_flac_push(None, None, 0, 0, None, 0, None, None, None) == _lib.FQ3_EINVAL


def test_spec_validation():
    s = ao.AudioOutSpec(None, "flac")
    assert s.validate(24000) is s and ao.NUMPY_DTYPES["flac"] == np.uint8
    ao.AudioOutSpec(8000, "flac", 1.25).validate(24000)
    ao.AudioOutSpec(44100, "flac").validate(24000)
    with pytest.raises(ValueError):
        ao.AudioOutSpec(None, "flac").validate(100000)         # neither a table rate nor 16 bits of Hz: the FLAC stage's own refusal
    ao.AudioOutSpec(None, "s16").validate(100000)              # ... which the other encodings do not share
    with pytest.raises(ValueError):
        ao.AudioOutSpec(24001, "flac").validate(24000)         # the resampler's refusal comes first, as ever
    with pytest.raises(ValueError):
        ao.AudioOutSpec(None, "mp3")
    with pytest.raises(ValueError):
        audio_io.wav_header_for(24000, "flac")
    with pytest.raises(ValueError):
        ao.AudioOut(ao.AudioOutSpec(None, "flac"), 24000, "cpu")        # no CPU fallback


# ---- server ------------------------------------------------------------------------------------------------------------------------
def _wave(n=5000):
    t = np.arange(n)
    return np.round(9000 * np.sin(t / 17.0) * np.hanning(n)).astype(np.int16)


def _flac_chunks(rate):
    """what a streaming vocoder with a ``flac`` spec hands out: uint8 chunks, the first one starting with the header"""
    data = np.frombuffer(R.encode(_wave(), rate, total=0), dtype=np.uint8)
    return [data[:1000], data[1000:1003], data[1003:]]


class _Model:
    """Stand-in for ``FasterQwen3TTS`` under the lock scheduler"""
    sample_rate = 24000

    def __init__(self):
        self.contexts, self.open = [], None

    def _text_tokenize(self):
        return lambda s: list(s.encode())

    @contextlib.contextmanager
    def audio_output(self, sample_rate=None, encoding="f32", speed=1.0):
        self.contexts.append((sample_rate, encoding, speed))
        self.open = ao.AudioOutSpec(sample_rate, encoding, speed)
        try:
            yield self.open
        finally:
            self.open = None

    def generate_voice_clone_streaming(self, **kw):
        if self.open is not None and self.open.encoding == "flac":
            for c in _flac_chunks(self.open.out_rate(24000)):
                yield c, self.open.out_rate(24000), {}
            return
        for n in (500, 200):
            yield np.ones(n, dtype=np.float32 if self.open is None else ao.NUMPY_DTYPES[self.open.encoding]), 24000, {}


class _Worker:
    """Stand-in for ``BatchWorker``"""

    def __init__(self):
        self.seen, self.sessions = [], []

    def _box(self, cfg):
        from fq3hip.server import BatchWorker
        box = queue.Queue()
        spec = cfg.get("audio_output")
        chunks = _flac_chunks(spec.out_rate(24000)) if spec is not None and spec.encoding == "flac" else [np.zeros(100, np.float32)]
        for c in chunks:
            box.put(c)
        box.put(BatchWorker.DONE)
        return box

    def submit(self, cfg, text):
        self.seen.append(cfg)
        return self._box(cfg)

    def submit_text(self, cfg, feeder):
        self.sessions.append(cfg)
        return self._box(cfg)


def _client(model, worker=None, scheduler="batch"):
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app
    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "t", "language": "English"}}
    return TestClient(create_app(model, voices, default_voice="alloy", scheduler=scheduler, worker=worker)), voices


def _check_flac_body(r, rate):
    assert r.status_code == 200 and r.headers["content-type"].startswith("audio/flac"), r.text
    assert r.content[:4] == b"fLaC"                            # no WAV header in front
    y, info = R.decode(r.content)
    assert np.array_equal(y, _wave()) and info["rate"] == rate and info["total"] == 0


def test_server_lock_scheduler_answers_flac():
    m = _Model()
    client, _ = _client(m, scheduler="lock")
    req = {"input": "hello", "voice": "alloy", "response_format": "flac"}
    _check_flac_body(client.post("/v1/audio/speech", json=req), 24000)
    assert m.contexts == [(None, "flac", 1.0)]
    _check_flac_body(client.post("/v1/audio/speech", json=dict(req, sample_rate=8000, speed=1.25)), 8000)
    assert m.contexts[-1] == (8000, "flac", 1.25)
    n = len(m.contexts)
    for extra in ({"encoding": "s16"}, {"encoding": "flac"}, {"encoding": "mulaw", "sample_rate": 8000}):
        r = client.post("/v1/audio/speech", json=dict(req, **extra))
        assert r.status_code == 400 and "encoding" in r.json()["detail"]
    assert client.post("/v1/audio/speech", json=dict(req, speed=9)).status_code == 400
    assert client.post("/v1/audio/speech", json=dict(req, sample_rate=24001)).status_code == 400
    # `flac` is a response format, not an `encoding` of the others; mp3 is refused as before
    assert client.post("/v1/audio/speech", json=dict(req, response_format="wav", encoding="flac")).status_code == 400
    r = client.post("/v1/audio/speech", json=dict(req, response_format="mp3"))
    assert r.status_code == 400 and "pydub" in r.json()["detail"]
    assert len(m.contexts) == n
    # a model without the device stage keeps its 400
    bare = SimpleNamespace(sample_rate=24000)
    client2, _ = _client(bare, scheduler="lock")
    assert client2.post("/v1/audio/speech", json=req).status_code == 400


def test_server_batch_scheduler_and_sessions_answer_flac():
    w, m = _Worker(), _Model()
    client, voices = _client(m, w)
    req = {"input": "hello", "voice": "alloy", "response_format": "flac"}
    _check_flac_body(client.post("/v1/audio/speech", json=req), 24000)
    assert w.seen[-1]["audio_output"] == ao.AudioOutSpec(None, "flac") and "audio_output" not in voices["alloy"]
    _check_flac_body(client.post("/v1/audio/speech", json=dict(req, sample_rate=16000, speed=0.5)), 16000)
    assert w.seen[-1]["audio_output"] == ao.AudioOutSpec(16000, "flac", 0.5)
    n = len(w.seen)
    assert client.post("/v1/audio/speech", json=dict(req, encoding="s16")).status_code == 400 and len(w.seen) == n
    base = "/v1/audio/speech/sessions"
    r = client.post(base, json={"voice": "alloy", "response_format": "flac", "sample_rate": 8000})
    assert r.status_code == 200 and w.sessions[-1]["audio_output"] == ao.AudioOutSpec(8000, "flac")
    _check_flac_body(client.get(f"{base}/{r.json()['id']}/audio"), 8000)
    assert client.post(base, json={"voice": "alloy", "response_format": "flac", "encoding": "alaw"}).status_code == 400
    assert client.post(base, json={"voice": "alloy", "response_format": "mp3"}).status_code == 400
    assert len(w.sessions) == 1
    # a model without the device stage: sessions refuse the format as well
    bare = SimpleNamespace(sample_rate=24000, _text_tokenize=lambda: (lambda s: list(s.encode())))
    client2, _ = _client(bare, _Worker())
    assert client2.post(base, json={"voice": "alloy", "response_format": "flac"}).status_code == 400
    assert client2.post("/v1/audio/speech", json=req).status_code == 400


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_bytes_as_they_are(tmp_path, capsys):
    from fq3hip import cli
    data = np.frombuffer(R.encode(_wave(), 24000), dtype=np.uint8)
    m = _Model()
    m.generate_custom_voice = lambda **kw: ([data], 24000)
    base = ["custom", "--text", "x", "--speaker", "s", "--encoding", "flac"]
    out = str(tmp_path / "a.flac")
    cli.cmd_once(cli.build_parser().parse_args(base + ["--output", out]), model=m)
    assert m.contexts == [(None, "flac", 1.0)] and open(out, "rb").read() == data.tobytes()
    assert "WARNING" not in capsys.readouterr().out
    out2 = str(tmp_path / "b.wav")
    cli.cmd_once(cli.build_parser().parse_args(base + ["--output", out2, "--out-rate", "8000"]), model=m)
    assert m.contexts[-1] == (8000, "flac", 1.0) and open(out2, "rb").read() == data.tobytes()
    assert "WARNING" in capsys.readouterr().out
