"""GPU: long-form synthesis end to end (fq3hip/long_form.py): the sentences of a text decode in the lanes of
one lock-step batch and their waveforms are joined on the device.  Synthetic weights give noise, not speech, so the join threshold is
the median hop peak of the first segment's audio: hops are both removed and kept.  Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _join_ref as R
from fq3hip.long_form import LongFormSpec, split_text

TEXT = "The quick brown fox jumps. Over the lazy dog it goes! And then it sleeps for a while?"
MAX_CHARS = 40
_state = {}


def _model():
    if "m" not in _state:
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
        _state["m"] = m
        _state["kw"] = dict(language="English", voice_clone_prompt=vcp, do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0,
                            max_new_tokens=22, min_new_tokens=22, non_streaming_mode=False)
    return _state["m"], _state["kw"]


def _reference():
    """Computed once: the segments, what the existing batch entry points give for them, and the spec whose threshold is the median
    hop peak of the first segment's waveform."""
    if "ref" not in _state:
        m, kw = _model()
        segs = split_text(TEXT, MAX_CHARS)
        texts = [s.text for s in segs]
        full = [w[0] for w, _sr in m.generate_voice_clone_batch(texts, lanes=3, **kw)]
        chunks = {i: [] for i in range(len(texts))}
        for i, a, _sr, _tm in m.generate_voice_clone_batch_streaming(texts, chunk_size=4, lanes=3, **kw):
            chunks[i].append(np.asarray(a, dtype=np.float32).copy())
        streamed = [np.concatenate(chunks[i]) for i in range(len(texts))]
        x = full[0]
        peaks = [float(np.abs(x[h: h + 240]).max()) for h in range(0, len(x), 240)]
        thr = float(np.median(peaks))
        assert 0.0 < thr < 1.0
        spec = LongFormSpec(max_chars=MAX_CHARS, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=thr,
                            lead_hops=1, tail_hops=2, hold_hops=4)
        _state["ref"] = (segs, full, streamed, spec)
    return _state["ref"]


def _join(waves, segs, spec):
    return R.join([(w, spec.pause_samples(s.pause, 24000)) for w, s in zip(waves, segs)], 24000, spec.threshold, spec.lead_hops,
                  spec.tail_hops, spec.hold_hops)


def test_one_shot_equals_reference_join_of_the_batch_waveforms():
    m, kw = _model()
    segs, full, _streamed, spec = _reference()
    assert len(segs) == 3 and [s.pause for s in segs] == ["sentence", "sentence", "end"]
    got, sr = m.generate_long_voice_clone(TEXT, lanes=3, long_form=spec, **kw)
    want = _join(full, segs, spec)
    assert sr == 24000 and got[0].dtype == np.float32
    # the threshold removes hops and keeps hops
    assert 0 < want.size < sum(len(w) for w in full) + 2 * 1200
    assert np.array_equal(got[0], want)


def test_streaming_equals_reference_join_of_the_batch_chunks_in_text_order():
    m, kw = _model()
    segs, _full, streamed, spec = _reference()
    events = [(np.asarray(a).copy(), sr, tm) for a, sr, tm in
              m.generate_long_voice_clone_streaming(TEXT, chunk_size=4, lanes=3, long_form=spec, **kw)]
    assert np.array_equal(np.concatenate([a for a, _, _ in events]), _join(streamed, segs, spec))
    idx = [tm["segment_index"] for _, _, tm in events]
    assert idx == sorted(idx) and idx[0] == 0 and idx[-1] == 2                     # non-decreasing: strictly in text order
    assert all(tm["n_segments"] == 3 and sr == 24000 for _, sr, tm in events)
    assert [tm["chunk_index"] for _, _, tm in events] == list(range(len(events)))
    assert [tm["is_final"] for _, _, tm in events] == [False] * (len(events) - 1) + [True]


def test_inside_audio_output_streaming_equals_one_shot():
    m, kw = _model()
    _segs, _full, _streamed, spec = _reference()
    with m.audio_output(16000, "s16"):
        one, sr1 = m.generate_long_voice_clone(TEXT, lanes=3, long_form=spec, **kw)
        got = [(np.asarray(a).copy(), sr) for a, sr, _tm in
               m.generate_long_voice_clone_streaming(TEXT, chunk_size=4, lanes=3, long_form=spec, **kw)]
    cat = np.concatenate([a for a, _ in got])
    assert sr1 == 16000 and all(sr == 16000 for _, sr in got)
    assert one[0].dtype == np.dtype("<i2") and cat.dtype == one[0].dtype and one[0].size > 0
    assert np.array_equal(cat, one[0])
    assert m._audio_spec is None


def test_seeded_sampling_reproduces_itself():
    m, kw = _model()
    _segs, _full, _streamed, spec = _reference()
    kws = dict(kw, do_sample=True, top_k=20)
    with m.seeded(7):
        a, _ = m.generate_long_voice_clone(TEXT, lanes=3, long_form=spec, **kws)
        b, _ = m.generate_long_voice_clone(TEXT, lanes=3, long_form=spec, **kws)
    with m.seeded(8):
        c, _ = m.generate_long_voice_clone(TEXT, lanes=3, long_form=spec, **kws)
    assert a[0].size > 0 and np.array_equal(a[0], b[0])
    assert not np.array_equal(a[0], c[0])
    # segment i samples with seed + i: the batch entry point with seeds=7 gives the waveforms that were joined
    segs = split_text(TEXT, MAX_CHARS)
    waves = [w[0] for w, _sr in m.generate_voice_clone_batch([s.text for s in segs], lanes=3, seeds=7, **kws)]
    assert np.array_equal(a[0], _join(waves, segs, spec))


def test_existing_methods_are_unchanged_by_a_long_form_call():
    m, kw = _model()
    segs, full, streamed, spec = _reference()
    texts = [s.text for s in segs]
    single0, _ = m.generate_voice_clone(text=texts[0], **kw)
    m.generate_long_voice_clone(TEXT, lanes=3, long_form=spec, **kw)
    list(m.generate_long_voice_clone_streaming(TEXT, chunk_size=4, lanes=3, long_form=spec, **kw))
    again = [w[0] for w, _sr in m.generate_voice_clone_batch(texts, lanes=3, **kw)]
    assert all(np.array_equal(a, b) for a, b in zip(again, full))
    chunks = {i: [] for i in range(len(texts))}
    for i, a, _sr, _tm in m.generate_voice_clone_batch_streaming(texts, chunk_size=4, lanes=3, **kw):
        assert isinstance(a, np.ndarray)                            # what the function yields by default has not changed
        chunks[i].append(a.copy())
    assert all(np.array_equal(np.concatenate(chunks[i]), streamed[i]) for i in range(len(texts)))
    single1, _ = m.generate_voice_clone(text=texts[0], **kw)
    assert np.array_equal(single0[0], single1[0])


def test_one_segment_and_argument_errors():
    m, kw = _model()
    _segs, full, _streamed, spec = _reference()
    one_text = split_text(TEXT, MAX_CHARS)[0].text
    assert len(split_text(one_text, MAX_CHARS)) == 1
    got, _ = m.generate_long_voice_clone(one_text, lanes=3, long_form=spec, **kw)
    want = R.join([(full[0], 0)], 24000, spec.threshold, spec.lead_hops, spec.tail_hops, spec.hold_hops)
    assert np.array_equal(got[0], want)
    for bad in ("", "  \n\t "):
        with pytest.raises(ValueError):
            m.generate_long_voice_clone(bad, lanes=3, long_form=spec, **kw)
        with pytest.raises(ValueError):
            next(m.generate_long_voice_clone_streaming(bad, lanes=3, long_form=spec, **kw))
