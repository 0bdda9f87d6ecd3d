"""CPU: the host side of exact streaming -- ``StreamingVocoder(exact=True)`` over a toy causal tokenizer, the ``exact_streaming()``
context manager, and the server / CLI flags that enter it."""
import contextlib
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fq3hip import cli
from fq3hip.model import FasterQwen3TTS, StreamingVocoder


class ToyTokenizer:
    """A causal "codec" in numpy: frame value = its first code, held for SPF samples, through a causal FIR; the last TRIM samples of a
    decode are trimmed (as the transposed convs do), so ``num_samples_total(T) = T * SPF - TRIM`` and the ICL cut depends on T."""
    sample_rate, CHUNK_FRAMES, SPF, TRIM = 24000, 300, 4, 3
    FIR = np.array([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125], dtype=np.float32)       # reaches 7 samples = 2 frames back

    def __init__(self):
        self.opened, self.pushes = [], []

    def num_samples_total(self, T: int) -> int:
        return max(0, int(T) * self.SPF - self.TRIM)

    def wave(self, codes) -> np.ndarray:
        v = np.repeat(np.asarray(codes)[:, 0].astype(np.float32), self.SPF)
        y = np.convolve(v, self.FIR)[:len(v)].astype(np.float32)
        return y[:self.num_samples_total(len(codes))]

    def stream_open(self, ref_codes=None, stream=None):
        st = SimpleNamespace(codes=np.zeros((0, 16), np.int64) if ref_codes is None else ref_codes.numpy().copy())
        self.opened.append(st)
        return st

    def stream_push(self, streams, codes):
        rows = []
        for st, c in zip(streams, codes.numpy()):
            F = len(st.codes)
            st.codes = np.concatenate([st.codes, c])
            rows.append(self.wave(st.codes)[self.num_samples_total(F):])
        self.pushes.append((len(streams), int(codes.shape[1])))
        return torch.from_numpy(np.stack(rows))


def _codes(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 100, (n, 16)))


def _stream(voc, gen, chunk):
    out = []
    for i in range(0, len(gen), chunk):
        a, sr = voc.push(gen[i:i + chunk], final=i + chunk >= len(gen))
        assert sr == 24000
        out.append(np.asarray(a))
    return out


@pytest.mark.parametrize("chunk", [1, 8, 12])
def test_exact_chunks_are_slices_of_the_one_pass_decode(chunk):
    tok, gen = ToyTokenizer(), _codes(43, 0)                              # 43 frames: a ragged last chunk at 8 and 12
    voc = StreamingVocoder(tok, None, chunk, "cpu", None, exact=True)
    assert voc.exact and voc.c0 == 0
    parts = _stream(voc, gen, chunk)
    full = tok.wave(gen.numpy())
    assert [len(p) for p in parts[1:]] == [tok.SPF * min(chunk, 43 - i) for i in range(chunk, 43, chunk)]
    assert np.array_equal(np.concatenate(parts), full)
    assert tok.pushes == [(1, min(chunk, 43 - i)) for i in range(0, 43, chunk)]          # one push per chunk, the new frames only
    tail, sr = voc.flush()                                                # a final event without codes, no output stage: nothing left
    assert len(tail) == 0 and sr == 24000


@pytest.mark.parametrize("chunk", [4, 12])
def test_exact_icl_stream_begins_at_the_cut_floor(chunk):
    tok, ref, gen = ToyTokenizer(), _codes(21, 1), _codes(30, 2)
    voc = StreamingVocoder(tok, ref, chunk, "cpu", None, exact=True)
    # c0: the lower bound of the non-streaming cut int(ref_len / T * n(T)) over every one-pass total length T <= CHUNK_FRAMES
    cuts = [int(21 / T * tok.num_samples_total(T)) for T in range(22, 301)]
    assert voc.c0 == min(cuts) and voc.c0 >= tok.num_samples_total(21) and len(set(cuts)) > 1
    assert len(tok.opened) == 1 and len(tok.opened[0].codes) == 21       # the stream began behind the reference
    parts = _stream(voc, gen, chunk)
    full = tok.wave(np.concatenate([ref.numpy(), gen.numpy()]))
    got = np.concatenate(parts)
    assert np.array_equal(got, full[voc.c0:])
    assert len(parts[0]) == tok.SPF * chunk - (voc.c0 - tok.num_samples_total(21))        # the drop comes off the first push only
    cut = int(21 / 51 * tok.num_samples_total(51))                         # what the non-streaming entry point cuts at this length
    assert cut >= voc.c0 and np.array_equal(got[cut - voc.c0:], full[cut:])


def test_exact_needs_a_tokenizer_with_stream_states():
    with pytest.raises(ValueError, match="stream"):
        StreamingVocoder(SimpleNamespace(sample_rate=24000), None, 8, "cpu", None, exact=True)


def _bare_model(tok):
    m = FasterQwen3TTS.__new__(FasterQwen3TTS)
    m.model = SimpleNamespace(model=SimpleNamespace(speech_tokenizer=tok))
    m.device = "cpu"
    return m


def test_context_manager_sets_and_restores_the_mode():
    m = _bare_model(ToyTokenizer())
    assert m._exact_kw() == {} and not m.streaming_vocoder(None, 8).exact
    with m.exact_streaming():
        assert m._exact_kw() == dict(exact=True)
        voc = m.streaming_vocoder(_codes(5, 3), 8)
        assert voc.exact and voc.c0 > 0
        with m.exact_streaming():                                         # nested: the inner exit restores "on"
            pass
        assert m.streaming_vocoder(None, 8).exact
    assert m._exact_kw() == {} and not m.streaming_vocoder(None, 8).exact
    with pytest.raises(RuntimeError, match="boom"):
        with m.exact_streaming():
            raise RuntimeError("boom")
    assert m._exact_kw() == {} and not m.streaming_vocoder(None, 8).exact


# ---- CLI and server flags (stand-in models in the manner of tests/test_serving_cpu.py) ------------------------------------------------
class _ExactAware:
    """keeps the mode like the model does, and notes it wherever a vocoder would be built"""
    sample_rate = 24000

    def __init__(self):
        self.exact, self.seen = False, []

    @contextlib.contextmanager
    def exact_streaming(self):
        prev, self.exact = self.exact, True
        try:
            yield
        finally:
            self.exact = prev


class _CliModel(_ExactAware):
    def generate_voice_clone_streaming(self, text, chunk_size=12, **kw):
        self.seen.append(("stream", self.exact))                          # (as streaming_vocoder would read it, at the first chunk)
        for _ in range(2):
            yield np.full(480, 0.25, np.float32), 24000, {}

    def generate_voice_clone(self, text, **kw):
        self.seen.append(("once", self.exact))
        return [np.full(480, 0.25, np.float32)], 24000


def test_cli_flag_enters_the_context(tmp_path):
    p = cli.build_parser()
    base = ["clone", "--text", "hi", "--output", str(tmp_path / "o.wav"), "--ref-audio", "r.wav", "--ref-text", "t", "--streaming"]
    assert p.parse_args(base).exact_streaming is False
    m = _CliModel()
    cli.cmd_once(p.parse_args(base), model=m)
    cli.cmd_once(p.parse_args(base + ["--exact-streaming"]), model=m)
    assert m.seen == [("stream", False), ("stream", True)] and m.exact is False
    a = p.parse_args(["serve", "--ref-audio", "r.wav", "--ref-text", "t", "--output-dir", str(tmp_path / "d"), "--streaming", "--exact-streaming"])
    cli.cmd_serve(a, model=m, lines=["one\n", "quit\n"])
    assert m.seen[-1] == ("stream", True) and m.exact is False


class _BatchModel(_ExactAware):
    """what BatchWorker needs of a model; ``streaming_vocoder`` runs on the worker's thread"""

    class _Voc:
        def push(self, codes, ready_event=None):
            return np.full(100 * int(codes.shape[0]), 0.5, np.float32), 24000

    class _Dec:
        def run(self, requests, on_error="raise", source=None, chunk_frames=None):
            pending = list(requests)
            while pending:
                req = pending.pop(0)
                yield req.rid, torch.zeros(3, 16, dtype=torch.long), {"is_final": True, "total_steps_so_far": 3, "steps": 3}
                while source is not None:
                    r = source()
                    if r is None:
                        break
                    pending.append(r)

    def _prepare_generation(self, text, **kw):
        return None, None, None, text, None, None, None, None

    @staticmethod
    def _gen_kwargs(*a):
        return {}

    def streaming_vocoder(self, rc, chunk):
        self.seen.append(("vocoder", self.exact))
        return self._Voc()

    def _batch_decoder(self, lanes):
        return self._Dec()

    def generate_voice_clone_streaming(self, text, chunk_size=12, **kw):
        self.seen.append(("stream", self.exact))
        yield np.full(480, 0.25, np.float32), 24000, {}


@pytest.mark.parametrize("scheduler", ["lock", "batch"])
def test_server_flag_enters_the_context_for_the_process(monkeypatch, scheduler):
    from fastapi.testclient import TestClient
    import uvicorn
    import fq3hip.batching as Bt
    from fq3hip import server

    class Req:
        def __init__(self, rid, talker, tie, tam, tth, tpe, config, kw):
            self.rid, self.gen_kwargs = rid, dict(kw)

    monkeypatch.setattr(Bt, "BatchRequest", Req)
    assert server.build_parser().parse_args(["--ref-audio", "r.wav"]).exact_streaming is False
    for flag in ([], ["--exact-streaming"]):
        m, apps = _BatchModel(), []
        monkeypatch.setattr(cli, "load_model", lambda args: m)
        monkeypatch.setattr(uvicorn, "run", lambda app, **kw: apps.append(app))
        server.main(["--ref-audio", "r.wav", "--ref-text", "t", "--scheduler", scheduler, "--lanes", "2", "--chunk-size", "4"] + flag)
        client = TestClient(apps[0])
        assert client.get("/health").json().get("exact_streaming", False) is bool(flag)
        r = client.post("/v1/audio/speech", json={"input": "abc", "voice": "default", "response_format": "pcm"})
        assert r.status_code == 200 and len(r.content) > 0
        assert m.seen and all(mode is bool(flag) for _what, mode in m.seen), (scheduler, flag, m.seen)
    with pytest.raises(ValueError, match="exact_streaming"):
        server.create_app(SimpleNamespace(sample_rate=24000), {"v": {}}, scheduler="lock", exact_streaming=True)
