"""GPU: long form for many texts end to end: the segments of three texts (1, 2 and 4 sentences; the last has
more segments than there are lanes) are the requests of ONE lock-step run of three lanes, and every text comes out as the single-text
call gives it inside ``seeded(seed_t)``, bit for bit -- one shot and streaming, plain, through ``output=`` and inside ``limiter()`` and
``leveller()``.  Synthetic weights give noise, not speech, so the join threshold is the median hop peak of a waveform: hops are both
removed and kept.  The model and the fixture are those of tests/test_gpu_long_form.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fq3hip.audio_out import AudioOutSpec
from fq3hip.long_form import LongFormSpec, split_text
from test_gpu_long_form import MAX_CHARS, _model

TEXTS = ["A lone sentence stands here.",
         "The quick brown fox jumps. Over the lazy dog it goes!",
         "And then it sleeps for a while? The morning comes around again. Nobody saw the fox that day! Where did the lazy dog go?"]
SEEDS = [11, 23, 5]
_state = {}


def _setup():
    """Computed once: the spec, the sampling arguments, and every text through the single-text call inside its seed."""
    if "ref" not in _state:
        m, kw = _model()
        assert [len(split_text(t, MAX_CHARS)) for t in TEXTS] == [1, 2, 4]
        kws = dict(kw, do_sample=True, top_k=20)
        x = m.generate_voice_clone(text=TEXTS[0], **kw)[0][0]
        thr = float(np.median([float(np.abs(x[h: h + 240]).max()) for h in range(0, len(x), 240)]))
        assert 0.0 < thr < 1.0
        spec = LongFormSpec(max_chars=MAX_CHARS, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=thr,
                            lead_hops=1, tail_hops=2, hold_hops=4)
        lkw = dict(kws, lanes=3, long_form=spec)
        _state["ref"] = (m, lkw, _singles(m, lkw))
    return _state["ref"]


def _singles(m, lkw):
    out = []
    for text, seed in zip(TEXTS, SEEDS):
        with m.seeded(seed):
            w, sr = m.generate_long_voice_clone(text, **lkw)
        out.append((w[0], sr))
    return out


def _streamed(m, lkw, **more):
    """the streaming entry point -> per text (concatenated audio, the events' infos, the rates)"""
    per = {t: [] for t in range(len(TEXTS))}
    for t, a, sr, info in m.generate_long_voice_clone_batch_streaming(TEXTS, chunk_size=4, seeds=SEEDS, **lkw, **more):
        per[t].append((np.asarray(a).copy(), sr, dict(info)))
    return per


def _check_events(per, n_segments):
    for t, events in per.items():
        idx = [info["segment_index"] for _a, _sr, info in events]
        assert idx == sorted(idx) and idx[0] >= 0 and idx[-1] == n_segments[t] - 1, (t, idx)       # never decreases: text order
        assert [info["is_final"] for _a, _sr, info in events] == [False] * (len(events) - 1) + [True], t  # exactly one closes the text
        assert [info["chunk_index"] for _a, _sr, info in events] == list(range(len(events))), t
        assert all(info["n_segments"] == n_segments[t] and info["total_steps_so_far"] >= 0 for _a, _sr, info in events)


def test_every_text_equals_its_single_call():
    m, lkw, want = _setup()
    got = m.generate_long_voice_clone_batch(TEXTS, seeds=SEEDS, **lkw)
    assert len(got) == len(TEXTS)
    for t, ((w, sr), (w1, sr1)) in enumerate(zip(got, want)):
        assert sr == sr1 == 24000 and w[0].dtype == np.float32 and w1.size > 0
        assert np.array_equal(w[0], w1), t
    assert not np.array_equal(want[1][0][:1000], want[2][0][:1000])  # (the texts do differ)
    # an int seed s gives text t the seed s + t
    one = m.generate_long_voice_clone_batch(TEXTS[:2], seeds=SEEDS[1] - 1, **lkw)
    assert np.array_equal(one[1][0][0], want[1][0])


def test_streaming_pieces_concatenate_to_the_same_samples_in_text_order():
    m, lkw, want = _setup()
    per = _streamed(m, lkw)
    _check_events(per, [1, 2, 4])
    for t, events in per.items():
        assert all(sr == 24000 for _a, sr, _i in events)
        assert np.array_equal(np.concatenate([a for a, _sr, _i in events]), want[t][0]), t


def test_output_spec_equals_the_single_call_inside_audio_output():
    m, lkw, _want = _setup()
    with m.audio_output(16000, "s16"):
        want = _singles(m, lkw)
    spec = AudioOutSpec(16000, "s16")
    got = m.generate_long_voice_clone_batch(TEXTS, seeds=SEEDS, output=spec, **lkw)
    per = _streamed(m, lkw, output=[spec, spec, spec])
    _check_events(per, [1, 2, 4])
    for t, (w1, sr1) in enumerate(want):
        assert sr1 == 16000 and w1.dtype == np.dtype("<i2") and w1.size > 0
        assert got[t][1] == 16000 and got[t][0][0].dtype == w1.dtype and np.array_equal(got[t][0][0], w1), t
        cat = np.concatenate([a for a, _sr, _i in per[t]])
        assert all(sr == 16000 for _a, sr, _i in per[t]) and cat.dtype == w1.dtype and np.array_equal(cat, w1), t
    # one spec or None per text; the context itself keeps refusing the batch entry points
    mixed = m.generate_long_voice_clone_batch(TEXTS[:2], seeds=SEEDS[:2], output=[None, spec], **lkw)
    assert mixed[0][1] == 24000 and mixed[0][0][0].dtype == np.float32 and np.array_equal(mixed[1][0][0], want[1][0])
    with m.audio_output(16000, "s16"):
        with pytest.raises(ValueError):
            m.generate_long_voice_clone_batch(TEXTS, seeds=SEEDS, **lkw)
        with pytest.raises(ValueError):
            next(m.generate_long_voice_clone_batch_streaming(TEXTS, seeds=SEEDS, **lkw))


def test_inside_limiter_and_leveller():
    m, lkw, plain = _setup()
    with m.limiter(ceiling_db=-6.0), m.leveller(target_lufs=-20.0):
        want = _singles(m, lkw)
        got = m.generate_long_voice_clone_batch(TEXTS, seeds=SEEDS, **lkw)
        per = _streamed(m, lkw)
    _check_events(per, [1, 2, 4])
    for t, (w1, _sr) in enumerate(want):
        assert w1.size > 0 and not np.array_equal(w1, plain[t][0])       # the stages did something
        assert np.array_equal(got[t][0][0], w1), t
        assert np.array_equal(np.concatenate([a for a, _sr, _i in per[t]]), w1), t


def test_argument_errors_come_before_anything_decodes():
    m, lkw, _want = _setup()
    for bad in ([], "one text", [TEXTS[0], "  "], [TEXTS[0], 5]):
        with pytest.raises(ValueError):
            m.generate_long_voice_clone_batch(bad, **lkw)
        with pytest.raises(ValueError):
            next(m.generate_long_voice_clone_batch_streaming(bad, **lkw))
    with pytest.raises(ValueError):
        m.generate_long_voice_clone_batch(TEXTS, seeds=[1, 2], **lkw)
    with pytest.raises(ValueError):
        m.generate_long_voice_clone_batch(TEXTS, output="s16", **lkw)
    with m.loudness():
        with pytest.raises(ValueError):
            next(m.generate_long_voice_clone_batch_streaming(TEXTS, **lkw))


def test_existing_entry_points_are_unchanged_by_a_many_text_call():
    m, lkw, want = _setup()
    _m, kw = _model()
    single0, _ = m.generate_voice_clone(text=TEXTS[0], **kw)
    m.generate_long_voice_clone_batch(TEXTS, seeds=SEEDS, **lkw)
    list(m.generate_long_voice_clone_batch_streaming(TEXTS, chunk_size=4, seeds=SEEDS, **lkw))
    again = _singles(m, lkw)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(again, want))
    with m.seeded(SEEDS[2]):
        cat = np.concatenate([np.asarray(a).copy() for a, _sr, _tm in m.generate_long_voice_clone_streaming(TEXTS[2], chunk_size=4, **lkw)])
    assert np.array_equal(cat, want[2][0])
    for i, a, _sr, _tm in m.generate_voice_clone_batch_streaming(TEXTS[:2], chunk_size=4, lanes=3, **kw):
        assert isinstance(a, np.ndarray)                            # what the function yields by default has not changed
    single1, _ = m.generate_voice_clone(text=TEXTS[0], **kw)
    assert np.array_equal(single0[0], single1[0])

