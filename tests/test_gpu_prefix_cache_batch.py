"""GPU: the prefix KV cache in the lock-step batch, end to end -- the tiny synthetic voice-design and custom-voice models of
tests/test_gpu_prefix_cache.py (max_seq_len 384, greedy decoding, max_new_tokens 10).

The relation held is that file's: with the batch cache on, the ``*_batch`` entry points hand out the audio (a deterministic function
of the greedy codes) they hand out with it off -- for misses, for members that share a miss, for hits and after an eviction -- in
fp32; in bf16 a batch served from the entries equals the batch that created them bit for bit.  The uncached fp32 runs are computed
once per module."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_prefix_cache import GREEDY, LONG, LONG2, _model

TEXTS4 = ["Say this in a designed voice.", "And now something else entirely, please.", "A third thing to say.",
          "The last of the four sentences."]
VOICES4 = [LONG, LONG2, LONG, LONG2]                       # two voices, each used twice
KW = dict(max_new_tokens=10, **GREEDY)


def _waves(batch):
    return [np.asarray(w[0]).copy() for w, _sr in batch]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _chunks(gen):
    out = {}
    for i, audio, _sr, _tm in gen:
        out.setdefault(i, []).append(np.asarray(audio).copy())
    return {i: np.concatenate(v) for i, v in out.items()}, {i: len(v) for i, v in out.items()}


@pytest.fixture(scope="module")
def design():
    """(model, uncached audio of the four-text batch at 4 lanes, at 1 lane, uncached streaming chunks)."""
    _cfg, _W, m = _model("voice_design")
    assert getattr(m, "_batch_prefix_cache", None) is None
    plain4 = _waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW))
    plain1 = _waves(m.generate_voice_design_batch(TEXTS4[:2], [LONG, LONG], "English", lanes=1, **KW))
    plain_s = _chunks(m.generate_voice_design_batch_streaming(TEXTS4, VOICES4, "English", lanes=4, chunk_size=4, **KW))
    yield m, plain4, plain1, plain_s
    m.disable_prefix_cache(batch=True)


def test_batch_of_two_voices_fp32_equals_the_uncached_run_and_a_second_batch_is_all_hits(design):
    m, plain4, _p1, _ps = design
    cache = m.enable_prefix_cache(384, batch=True)
    assert m.talker_graph.engine.prefix_cache is None and m.talker_graph.engine.prefix_split      # the lock path sees no cache
    assert m._batch_decoder(4).prefix_cache is cache
    got = _waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW))
    st = cache.stats()
    assert (st["misses"], st["hits"], st["bypasses"], st["entries"]) == (2, 2, 0, 2), st
    assert _same(got, plain4)
    again = _waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW))
    st = cache.stats()
    assert (st["misses"], st["hits"], st["evictions"]) == (2, 6, 0), st
    assert _same(again, plain4)
    m.disable_prefix_cache(batch=True)
    assert m._batch_decoder(4).prefix_cache is None and not m.talker_graph.engine.prefix_split
    assert _same(_waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW)), plain4)      # off again


def test_streaming_batch_gives_the_uncached_chunks_fp32(design):
    m, _p4, _p1, (plain_audio, plain_counts) = design
    cache = m.enable_prefix_cache(384, batch=True)
    audio, counts = _chunks(m.generate_voice_design_batch_streaming(TEXTS4, VOICES4, "English", lanes=4, chunk_size=4, **KW))
    st = cache.stats()
    assert (st["misses"], st["hits"]) == (2, 2), st
    assert counts == plain_counts and sorted(audio) == [0, 1, 2, 3]
    for i in audio:
        assert np.array_equal(audio[i], plain_audio[i]), i
    m.disable_prefix_cache(batch=True)


def test_eviction_with_room_for_one_voice_still_gives_the_uncached_audio(design):
    m, plain4, _p1, _ps = design
    P = m._design_prepare(TEXTS4[0], LONG, "English", None)[3].fq3_prefix[0]
    assert (P + 63) // 64 == 2
    cache = m.enable_prefix_cache(128, batch=True)               # exactly one voice's blocks
    got = _waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW))
    st = cache.stats()
    assert st["evictions"] >= 1 and st["entries"] == 1 and st["misses"] + st["hits"] == 4 and st["bypasses"] == 0, st
    assert cache.pool.stats()["high_water"] <= 2
    assert _same(got, plain4)
    m.disable_prefix_cache(batch=True)


def test_scheduler_admits_a_staged_request_through_the_cache(design):
    """One lane, one spare context: the second request is staged while the first decodes and admitted at a frame boundary -- its
    prefill is a hit through the single-member branch of the staging."""
    m, _p4, plain1, _ps = design
    cache = m.enable_prefix_cache(384, batch=True)
    dec = m._batch_decoder(1)
    assert len(dec.stages) == 1 and dec.prefix_cache is cache
    got = _waves(m.generate_voice_design_batch(TEXTS4[:2], [LONG, LONG], "English", lanes=1, **KW))
    st = cache.stats()
    assert (st["misses"], st["hits"], st["bypasses"]) == (1, 1, 0), st
    assert _same(got, plain1)
    m.disable_prefix_cache(batch=True)


def test_second_batch_equals_the_first_bf16():
    _cfg, _W, m = _model("voice_design", torch.bfloat16)
    cache = m.enable_prefix_cache(384, batch=True)
    a = _waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW))
    b = _waves(m.generate_voice_design_batch(TEXTS4, VOICES4, "English", lanes=4, **KW))
    st = cache.stats()
    assert (st["misses"], st["hits"]) == (2, 6), st
    assert _same(a, b)
    m.disable_prefix_cache(batch=True)


def test_custom_voice_batch_with_and_without_an_instruct():
    _cfg, _W, m = _model("custom_voice")
    texts, instr = TEXTS4[:3], [LONG, None, LONG]
    plain = _waves(m.generate_custom_voice_batch(texts, "bob", "English", instruct=instr, lanes=3, **KW))
    cache = m.enable_prefix_cache(384, batch=True)
    got = _waves(m.generate_custom_voice_batch(texts, "bob", "English", instruct=instr, lanes=3, **KW))
    st = cache.stats()
    assert (st["misses"], st["hits"], st["bypasses"]) == (1, 1, 1), st
    assert _same(got, plain)
    m.disable_prefix_cache(batch=True)
