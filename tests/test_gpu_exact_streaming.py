"""GPU: exact streaming end to end (tiny model as in tests/test_gpu_api.py).  ``StreamingVocoder(exact=True)`` and everything inside
``FasterQwen3TTS.exact_streaming()`` stream, sample for sample, the one-pass decode of the utterance's codes -- at any chunk size, single
and in lock-step lanes, with the output stage behind it -- and outside the context nothing changes.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_weights

SAMPLED = dict(temperature=0.9, top_k=20, repetition_penalty=1.05)
TEXT = "A line that is long enough to stream."


@pytest.fixture(scope="module")
def model():
    from fq3hip.model import FasterQwen3TTS
    cfg = tiny_test_config()
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "codec", "text"))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, codec_max_frames=128, max_frames=64)
    g = torch.Generator().manual_seed(4)
    ref = torch.randint(0, cfg.codec.codebook_size, (12, 16), generator=g)
    vcp = dict(ref_spk_embedding=[torch.randn(cfg.talker.hidden_size, generator=g)], ref_code=[ref], x_vector_only_mode=[False], icl_mode=[True])
    return cfg, m, vcp


def _codes(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.codec.codebook_size, (n, cfg.codec.num_quantizers), generator=g).cuda()


def _push_all(voc, gen, chunk):
    out = []
    for i in range(0, gen.shape[0], chunk):
        a, _sr = voc.push(gen[i:i + chunk].contiguous(), final=i + chunk >= gen.shape[0])
        out.append(np.asarray(a).copy())
    return out


@pytest.mark.parametrize("ref_len", [0, 21])
def test_exact_vocoder_is_the_one_pass_decode_at_any_chunk_size(model, ref_len):
    from fq3hip.model import StreamingVocoder
    cfg, m, _vcp = model
    tok = m.speech_tokenizer
    side = m._vocoder_stream(tok)
    ref = _codes(cfg, ref_len, 1) if ref_len else None
    gen = _codes(cfg, 40, 2)
    full = tok.decode_tensor(torch.cat([ref, gen]) if ref_len else gen).cpu().numpy()
    outs = {}
    for chunk in (1, 8, 12):
        voc = StreamingVocoder(tok, ref, chunk, "cuda", side, exact=True)
        outs[chunk] = np.concatenate(_push_all(voc, gen, chunk))
        c0 = voc.c0
        assert len(voc.flush()[0]) == 0
    assert (c0 == 0) if not ref_len else (tok.num_samples(ref_len) <= c0 <= int(ref_len / (ref_len + 40) * len(full)))
    for chunk, a in outs.items():
        assert a.shape == full[c0:].shape and np.array_equal(a, full[c0:]), chunk


def test_default_windowing_depends_on_the_chunk_size():
    """the fact the mode exists for, at the real codec shapes (the frame-level transformer attends over 71 earlier rows, phase 2 hands
    it 25): the default vocoder's audio for the same codes differs between chunk 8 and chunk 12 -- the exact vocoder's does not"""
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.model import StreamingVocoder
    from fq3hip.streams import concurrent_stream
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=96, precision="bf16")
    side = concurrent_stream(torch.device("cuda"))
    gen = _codes(cfg, 72, 3)
    windowed = [np.concatenate(_push_all(StreamingVocoder(tok, None, c, "cuda", side), gen, c)) for c in (8, 12)]
    assert windowed[0].shape != windowed[1].shape or not np.array_equal(windowed[0], windowed[1])
    exact = [np.concatenate(_push_all(StreamingVocoder(tok, None, c, "cuda", side, exact=True), gen, c)) for c in (8, 12)]
    assert np.array_equal(exact[0], exact[1]) and np.array_equal(exact[0], tok.decode_tensor(gen).cpu().numpy())
    tok.close()


@pytest.mark.parametrize("encoding", ["mulaw", "flac"])
def test_output_stage_behind_the_exact_vocoder(model, encoding):
    """the encoded chunks are one AudioOut over the whole exact waveform, byte for byte"""
    from fq3hip.audio_out import AudioOut, AudioOutSpec
    from fq3hip.model import StreamingVocoder
    cfg, m, _vcp = model
    tok = m.speech_tokenizer
    side = m._vocoder_stream(tok)
    gen = _codes(cfg, 40, 5)
    spec = AudioOutSpec(8000, encoding).validate(24000)
    for chunk, final_push in ((8, True), (12, False)):         # the tail with the last chunk / from flush() after a last chunk not marked final
        voc = StreamingVocoder(tok, None, chunk, "cuda", side, output=spec, exact=True)
        parts = []
        for i in range(0, 40, chunk):
            a, sr = voc.push(gen[i:i + chunk].contiguous(), final=final_push and i + chunk >= 40)
            assert sr == 8000
            parts.append(np.asarray(a).copy())
        parts.append(np.asarray(voc.flush()[0]).copy())
        got = np.concatenate(parts)
        torch.cuda.synchronize()
        st = AudioOut(spec, 24000, "cuda")
        want = st.push_host(tok.decode_tensor(gen).flatten().float(), final=True)
        if encoding == "flac":
            want = np.concatenate([np.frombuffer(st.header(), dtype=np.uint8), want])
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (encoding, chunk)


def _chunks(gen):
    return [(np.asarray(a).copy(), int(tm.get("chunk_steps", 0))) for a, _sr, tm in gen]


def test_single_stream_inside_the_context(model):
    cfg, m, vcp = model
    tok = m.speech_tokenizer
    kw = dict(ref_text="the reference sentence", voice_clone_prompt=vcp, max_new_tokens=30, min_new_tokens=30, **SAMPLED)
    with m.exact_streaming(), m.seeded(77):
        a4 = _chunks(m.generate_voice_clone_streaming(TEXT, "English", chunk_size=4, **kw))
        a12 = _chunks(m.generate_voice_clone_streaming(TEXT, "English", chunk_size=12, **kw))
        c0 = m.streaming_vocoder(vcp["ref_code"][0], 4).c0
        whole, sr = m.generate_voice_clone(TEXT, "English", **kw)
    assert [n for _a, n in a4] == [4] * 7 + [2] and [n for _a, n in a12] == [12, 12, 6]
    s4, s12 = np.concatenate([a for a, _n in a4]), np.concatenate([a for a, _n in a12])
    assert s4.shape == s12.shape and np.array_equal(s4, s12)
    cut = int(12 / 42 * tok.num_samples_total(42))
    assert 0 < c0 <= cut and s4.shape[0] == tok.num_samples_total(42) - c0
    assert np.array_equal(s4[cut - c0:], whole[0])
    assert m._exact_kw() == {}


def test_batch_lanes_give_the_single_stream_chunks(model, monkeypatch):
    cfg, m, vcp = model
    tok = m.speech_tokenizer
    texts = [TEXT, "Another one.", "The third line, a little longer than the others.", "Four."]
    kw = dict(ref_text="the reference sentence", voice_clone_prompt=vcp, max_new_tokens=22, min_new_tokens=22, chunk_size=4, **SAMPLED)
    groups = []
    push = tok.stream_push
    monkeypatch.setattr(tok, "stream_push", lambda streams, codes: (groups.append(len(streams)), push(streams, codes))[1])
    with m.exact_streaming():
        single = []
        for i, t in enumerate(texts):
            with m.seeded(900 + i):
                single.append([a for a, n in _chunks(m.generate_voice_clone_streaming(t, "English", **kw)) if n > 0])
        assert set(groups) == {1}
        got = [[] for _ in texts]
        for idx, a, sr, tm in m.generate_voice_clone_batch_streaming(texts, "English", lanes=4, seeds=900, **kw):
            if tm["chunk_steps"] > 0:
                got[idx].append(np.asarray(a).copy())
    assert max(groups) > 1, groups                      # lanes that reached a chunk boundary together shared one push
    for i, (g, s) in enumerate(zip(got, single)):
        assert len(g) == len(s) == 6, (i, len(g), len(s))
        for k, (x, y) in enumerate(zip(g, s)):
            assert x.shape == y.shape and np.array_equal(x, y), (i, k)


def test_long_form_streaming_inside_the_context_is_the_one_shot_waveform(model):
    """long form (x-vector clone, segments in lanes, joined on the device): the join is cut-independent and every segment's exact stream
    is its one-pass decode, so the exact stream of the whole text is the one-shot method's waveform, sample for sample"""
    from fq3hip.long_form import LongFormSpec
    cfg, m, vcp = model
    xvec = dict(ref_code=[None], ref_spk_embedding=[vcp["ref_spk_embedding"][0].cuda()], x_vector_only_mode=[True], icl_mode=[False])
    text = "The quick brown fox jumps. Over the lazy dog it goes! And then it sleeps for a while?"
    spec = LongFormSpec(max_chars=40, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=0.05, lead_hops=1, tail_hops=2, hold_hops=4)
    kw = dict(language="English", voice_clone_prompt=xvec, max_new_tokens=22, min_new_tokens=22, non_streaming_mode=False, lanes=3,
              long_form=spec, **SAMPLED)
    with m.seeded(7):
        one, sr = m.generate_long_voice_clone(text, **kw)
        with m.exact_streaming():
            got = [np.asarray(a).copy() for a, _sr, _tm in m.generate_long_voice_clone_streaming(text, chunk_size=4, **kw)]
    assert sr == 24000 and one[0].size > 0
    cat = np.concatenate(got)
    assert cat.shape == one[0].shape and np.array_equal(cat, one[0])


def test_outside_the_context_nothing_changes(model, monkeypatch):
    """the same calls give exactly today's chunks: those of a StreamingVocoder built the old way over the same codes; no stream state is
    opened"""
    from fq3hip.generate import fast_generate
    from fq3hip.model import StreamingVocoder
    cfg, m, vcp = model
    tok = m.speech_tokenizer
    monkeypatch.setattr(tok, "stream_open", lambda *a, **k: pytest.fail("a stream state outside exact_streaming()"))
    kw = dict(ref_text="the reference sentence", voice_clone_prompt=vcp, max_new_tokens=30, min_new_tokens=30, **SAMPLED)
    with m.seeded(77):
        got = _chunks(m.generate_voice_clone_streaming(TEXT, "English", chunk_size=8, **kw))
    assert not m.streaming_vocoder(vcp["ref_code"][0], 8).exact
    _, talker, config, tie, tam, tth, tpe, rc = m._prepare_generation(text=TEXT, language="English", ref_text="the reference sentence",
                                                                      voice_clone_prompt=vcp)
    codes, _ = fast_generate(talker, tie, tam, tth, tpe, config, m.predictor_graph, m.talker_graph, max_new_tokens=30, min_new_tokens=30,
                             top_p=1.0, do_sample=True, seed=77, **SAMPLED)
    want = _push_all(StreamingVocoder(tok, rc, 8, m.device, m._vocoder_stream(tok)), codes, 8)
    assert len(got) == len(want) == 4
    for k, ((a, _n), b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), k
