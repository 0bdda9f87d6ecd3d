"""GPU: the prefix KV cache end to end -- tiny synthetic voice-design and custom-voice models (as in
tests/test_gpu_api.py::test_custom_voice_and_voice_design_paths), max_seq_len 384, greedy decoding.

The relation held is the one of the existing fp32 API tests: the greedy codes equal the oracle's on the very prompt embeddings the
wrapper built (torch.equal) -- with the cache on, for a miss and for hits alike -- plus hit == miss bit for bit in bf16.  The public
streaming entry points hand out audio, not codes: their audio (a deterministic function of the codes) and chunk-step totals are
compared with an uncached run's."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_weights

GREEDY = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, min_new_tokens=0)
LONG = "a calm, low and slightly husky voice that speaks slowly and leaves long pauses between the sentences"
LONG2 = "a bright, quick and cheerful voice that nearly sings, rising at the end of every single sentence it says"
SHORT = "speak slowly"
TEXTS = ("Say this in a designed voice.", "And now something else entirely, please.")


def _model(kind, dtype=torch.float32):
    from fq3hip.model import FasterQwen3TTS
    cfg = copy.deepcopy(tiny_test_config())
    cfg.tts_model_type, cfg.tts_model_size = kind, "1b7"
    cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "codec", "text"))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=dtype, max_seq_len=384, codec_max_frames=64, max_frames=32)
    m.predictor_graph.do_sample = False
    m.predictor_graph.top_k = 0
    return cfg, W, m


def _codes(m, prep):
    from fq3hip.generate import fast_generate
    _, talker, config, tie, tam, tth, tpe = prep
    codes, _ = fast_generate(talker, tie, tam, tth, tpe, config, m.predictor_graph, m.talker_graph, max_new_tokens=10, **GREEDY)
    return codes.cpu()


def _oracle_codes(orc, prep):
    from oracle import qwen3tts_oracle as O
    _, _, _, tie, tam, tth, tpe = prep
    return orc.generate(tie.cpu(), tam.cpu(), tth.cpu(), tpe.cpu(), O.SamplingParams(max_new_tokens=10, **GREEDY))


def _oracle(cfg, W):
    from oracle import qwen3tts_oracle as O
    orc = O.OracleTTS(cfg, W, max_seq_len=384)
    orc.pred_sampling = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0)
    return orc


def test_miss_hit_hit_fp32_codes_equal_the_oracle():
    cfg, W, m = _model("voice_design")
    orc = _oracle(cfg, W)
    cache = m.enable_prefix_cache(384, min_rows=1)
    assert m.talker_graph.engine.prefix_cache is cache
    preps = [m._design_prepare(TEXTS[0], LONG, "English", None), m._design_prepare(TEXTS[1], LONG, "English", None),
             m._design_prepare(TEXTS[0], LONG, "English", None)]
    P, key = preps[0][3].fq3_prefix
    assert P > 64 and preps[1][3].fq3_prefix == (P, key)
    assert torch.equal(preps[0][3][0, :P], preps[1][3][0, :P])                # the premise, on the device prompt path
    codes = []
    for i, prep in enumerate(preps):
        codes.append(_codes(m, prep))
        st = cache.stats()
        assert (st["misses"], st["hits"]) == ((1, 0), (1, 1), (1, 2))[i], st
    assert torch.equal(codes[2], codes[0])
    for c, prep in zip(codes, preps):
        assert torch.equal(c, _oracle_codes(orc, prep))
    st = cache.stats()
    assert st["rows_reused"] == 2 * P and st["bypasses"] == 0 and st["evictions"] == 0
    assert st["blocks_held"] == (P + 63) // 64 and st["blocks_capacity"] == 6
    # a short instruct (P < 64) with min_rows=1: cached too
    prep = m._design_prepare(TEXTS[0], SHORT, "English", None)
    Ps = prep[3].fq3_prefix[0]
    assert Ps < 64
    a = _codes(m, prep)
    b = _codes(m, m._design_prepare(TEXTS[0], SHORT, "English", None))
    assert torch.equal(a, b) and torch.equal(a, _oracle_codes(orc, prep))
    st = cache.stats()
    assert (st["misses"], st["hits"], st["rows_reused"]) == (2, 3, 2 * P + Ps)
    # off again: the plain prefill, the oracle's codes
    m.disable_prefix_cache()
    assert m.talker_graph.engine.prefix_cache is None
    prep = m._design_prepare(TEXTS[1], LONG, "English", None)
    assert torch.equal(_codes(m, prep), _oracle_codes(orc, prep))


def test_hit_equals_miss_bf16():
    cfg, W, m = _model("voice_design", torch.bfloat16)
    cache = m.enable_prefix_cache(384)
    a = _codes(m, m._design_prepare(TEXTS[0], LONG, "English", None))
    b = _codes(m, m._design_prepare(TEXTS[0], LONG, "English", None))
    st = cache.stats()
    assert (st["misses"], st["hits"]) == (1, 1)
    assert torch.equal(a, b)
    m.disable_prefix_cache()


def _audio(gen):
    chunks = [(np.asarray(a).copy(), t) for a, _sr, t in gen]
    return np.concatenate([a for a, _ in chunks]), sum(int(t.get("chunk_steps", 0)) for _, t in chunks)


def test_streaming_and_text_stream_entry_points_hit_the_same_entry():
    cfg, W, m = _model("voice_design")
    kw = dict(max_new_tokens=10, chunk_size=4, **GREEDY)
    pieces = ["Say this in ", "a designed ", "voice."]
    plain_s = _audio(m.generate_voice_design_streaming(TEXTS[0], LONG, "English", **kw))
    plain_t = _audio(m.stream_voice_design(iter(pieces), LONG, "English", **kw))
    plain_g, _sr = m.generate_voice_design(TEXTS[0], LONG, "English", max_new_tokens=10, **GREEDY)
    cache = m.enable_prefix_cache(384)
    got_g, _sr = m.generate_voice_design(TEXTS[0], LONG, "English", max_new_tokens=10, **GREEDY)          # miss
    got_s = _audio(m.generate_voice_design_streaming(TEXTS[0], LONG, "English", **kw))                   # hit
    got_t = _audio(m.stream_voice_design(iter(pieces), LONG, "English", **kw))                           # hit
    st = cache.stats()
    assert (st["misses"], st["hits"], st["entries"]) == (1, 2, 1), st
    assert np.array_equal(np.asarray(got_g[0]), np.asarray(plain_g[0]))
    assert np.array_equal(got_s[0], plain_s[0]) and got_s[1] == plain_s[1] and got_s[1] > 0
    assert np.array_equal(got_t[0], plain_t[0]) and got_t[1] == plain_t[1] and got_t[1] > 0
    m.disable_prefix_cache()


def test_custom_voice_with_an_instruct_goes_through_the_cache():
    cfg, W, m = _model("custom_voice")
    plain, _sr = m.generate_custom_voice(TEXTS[0], "bob", "English", instruct=LONG, max_new_tokens=10, **GREEDY)
    cache = m.enable_prefix_cache(384)
    a, _sr = m.generate_custom_voice(TEXTS[0], "bob", "English", instruct=LONG, max_new_tokens=10, **GREEDY)
    b, _sr = m.generate_custom_voice(TEXTS[0], "bob", "English", instruct=LONG, max_new_tokens=10, **GREEDY)
    m.generate_custom_voice(TEXTS[0], "bob", "English", max_new_tokens=10, **GREEDY)                     # no instruct: no note
    st = cache.stats()
    assert (st["misses"], st["hits"], st["bypasses"]) == (1, 1, 1), st
    assert np.array_equal(np.asarray(a[0]), np.asarray(plain[0])) and np.array_equal(np.asarray(b[0]), np.asarray(plain[0]))
    m.disable_prefix_cache()


def test_eviction_under_a_block_budget_and_bypass_of_a_prefix_beyond_it():
    cfg, W, m = _model("voice_design")
    prep = m._design_prepare(TEXTS[0], LONG, "English", None)
    P = prep[3].fq3_prefix[0]
    blocks = (P + 63) // 64
    assert blocks == 2 and (m._design_prepare(TEXTS[0], LONG2, "English", None)[3].fq3_prefix[0] + 63) // 64 == 2
    cache = m.enable_prefix_cache(64 * blocks)                   # exactly the first voice's blocks
    first = _codes(m, m._design_prepare(TEXTS[0], LONG, "English", None))
    _codes(m, m._design_prepare(TEXTS[0], LONG2, "English", None))             # evicts the first voice
    st = cache.stats()
    assert (st["misses"], st["evictions"], st["entries"], st["blocks_held"]) == (2, 1, 1, 2), st
    again = _codes(m, m._design_prepare(TEXTS[0], LONG, "English", None))
    st = cache.stats()
    assert (st["misses"], st["hits"], st["evictions"]) == (3, 0, 2), st
    assert torch.equal(again, first)
    assert cache.pool.stats()["high_water"] <= blocks
    cache = m.enable_prefix_cache(64)                            # one block: the two-block prefix does not fit
    byp = _codes(m, m._design_prepare(TEXTS[0], LONG, "English", None))
    st = cache.stats()
    assert (st["bypasses"], st["misses"], st["hits"]) == (1, 0, 0), st
    assert torch.equal(byp, first)
    m.disable_prefix_cache()
