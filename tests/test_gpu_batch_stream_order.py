"""GPU: batch streaming when lanes are re-used at staggered frames (fq3hip/stream_groups.py).  Three short
texts with their own frame limits share two lanes: the lane that finishes first is re-armed while the other is in the middle of its
utterance, so one poll gives an utterance two chunks of different decode shapes of which the second one's class is already open.
Every case asserts that the order rule actually fired (``stats["order_launches"] > 0``) and that, per utterance, the chunks are the
single-stream streaming entry point's: as many, sample for sample, numbered 0..n-1, ``is_final`` on the last only -- plain, with
every utterance's own limiter / leveller / output stage (their states move with the launches), with the codec stream states of
``exact_streaming()``, and through long form (device rows).  Everything is bit for bit.

The frame limits of the stage cases are no multiples of the chunk size: an utterance then ends in a partial chunk on both sides, and
what a stage held back leaves with that chunk -- not in one more event, which the two entry points place differently."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_weights

TEXTS = ["First line.", "A second, rather longer line of text.", "Three."]
LONG_TEXT = "The quick brown fox jumps. Over the lazy dog it goes! And then it sleeps for a while?"
LEVEL = dict(target_lufs=-20.0, smooth_hops=3, min_blocks=2)          # short utterances: the stage must get to work inside them
_state = {}


def _model(n_ref=9):
    """the tiny fp32 greedy model of test_gpu_serving.py and an ICL voice with ``n_ref`` reference frames"""
    if "m" not in _state:
        from fq3hip.model import FasterQwen3TTS
        cfg = tiny_test_config()
        W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "codec", "text"))
        m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, codec_max_frames=128, max_frames=64)
        m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
        _state["m"], _state["cfg"] = m, cfg
    key = ("kw", n_ref)
    if key not in _state:
        cfg = _state["cfg"]
        g = torch.Generator().manual_seed(12)
        spk = torch.randn(cfg.talker.hidden_size, generator=g)
        codes = torch.cat([torch.randint(0, cfg.talker.vocab_size - 1024, (n_ref, 1), generator=g),
                           torch.randint(0, cfg.codec.codebook_size, (n_ref, cfg.num_code_groups - 1), generator=g)], 1)
        vcp = dict(ref_code=[codes], ref_spk_embedding=[spk], x_vector_only_mode=[False], icl_mode=[True])
        _state[key] = dict(language="English", do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0,
                           ref_text="the reference", voice_clone_prompt=vcp)
    return _state["m"], _state[key]


def _single(m, kw, text, budget, floor, chunk, spec=None):
    ctx = contextlib.nullcontext() if spec is None else m.audio_output(spec.sample_rate, spec.encoding)
    with ctx:
        return [(np.asarray(a).copy(), sr, bool(tm["is_final"])) for a, sr, tm in
                m.generate_voice_clone_streaming(text=text, max_new_tokens=budget, min_new_tokens=floor, chunk_size=chunk, **kw)]


def _batch(m, kw, budgets, chunk, spec=None):
    """-> ({utterance: [(audio, rate, is_final, chunk_index)]}, the layer's counters)"""
    got = {i: [] for i in range(len(TEXTS))}
    extra = {} if spec is None else dict(output=spec)
    for i, a, sr, tm in m.generate_voice_clone_batch_streaming(TEXTS, max_new_tokens=list(budgets), min_new_tokens=min(budgets),
                                                               chunk_size=chunk, lanes=2, **extra, **kw):
        got[i].append((np.asarray(a).copy(), sr, bool(tm["is_final"]), int(tm["chunk_index"])))
    return got, dict(m._stream_group_stats)


def _compare(got, want_of, rate, dtype):
    for i, events in got.items():
        want = [c for c in want_of(i) if len(c[0]) > 0]
        mine = [c for c in events if len(c[0]) > 0]
        print(f"utterance {i}: {len(mine)} chunks (single stream: {len(want)}), sizes {[len(c[0]) for c in mine]} / {[len(c[0]) for c in want]}")
        assert [c[3] for c in events] == list(range(len(events))), (i, [c[3] for c in events])
        assert [c[2] for c in events] == [False] * (len(events) - 1) + [True], (i, [c[2] for c in events])
        assert len(mine) == len(want) >= 1, (i, len(mine), len(want))
        for k, (a, b) in enumerate(zip(mine, want)):
            assert a[1] == b[1] == rate and a[0].dtype == b[0].dtype == dtype, (i, k)
            assert a[0].shape == b[0].shape and np.array_equal(a[0], b[0]), (i, k)


@contextlib.contextmanager
def _variant(m, name):
    with contextlib.ExitStack() as st:
        if name in ("limiter", "leveller"):
            st.enter_context(m.fixed_gain(18.0 if name == "limiter" else 6.0))
        if name == "leveller":
            st.enter_context(m.leveller(**LEVEL))
        if name == "limiter":
            st.enter_context(m.limiter())
        yield


# (frame limits per text, chunk size): the lane of text 0 is re-used by text 2 while text 1 decodes
PLAIN = [((4, 12, 8), 4), ((8, 38, 30), 4), ((8, 32, 24), 12)]
STAGED = [((9, 38, 30), 4), ((9, 33, 25), 12)]
# exact mode: the class of a chunk is (min(frames before it, 48), new frames), the same for every lane once 48 frames exist, and a
# different one per position before -- so the rule has work only where an utterance's two chunks of one poll straddle frame 48 while
# the other lane is past it.  Behind a 12-frame reference the chunks of a poll begin at frames 12 + 8 m: 44 and 48.  (With chunks of
# 12 frames a poll completes one chunk per lane, and no frame limits of three texts on two lanes produce the situation.)
EXACT = ((5, 53, 45), 4, 12)


@pytest.mark.parametrize("budgets,chunk", PLAIN, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else f"chunk{v}")
def test_staggered_lanes_plain(budgets, chunk):
    m, kw = _model()
    got, stats = _batch(m, kw, budgets, chunk)
    print(budgets, chunk, stats)
    assert stats["order_launches"] > 0, stats                       # a condition of the case: without it nothing was tested
    _compare(got, lambda i: _single(m, kw, TEXTS[i], budgets[i], min(budgets), chunk), 24000, np.float32)


@pytest.mark.parametrize("budgets,chunk", STAGED, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else f"chunk{v}")
@pytest.mark.parametrize("variant", ["limiter", "leveller", "s16"])
def test_staggered_lanes_with_a_state_per_utterance(variant, budgets, chunk):
    from fq3hip.audio_out import AudioOutSpec
    m, kw = _model()
    spec = AudioOutSpec(16000, "s16") if variant == "s16" else None
    with _variant(m, variant):
        got, stats = _batch(m, kw, budgets, chunk, spec)
        print(variant, budgets, chunk, stats)
        assert stats["order_launches"] > 0, stats
        _compare(got, lambda i: _single(m, kw, TEXTS[i], budgets[i], min(budgets), chunk, spec), 16000 if spec else 24000,
                 np.dtype("<i2") if spec else np.float32)
    if variant in ("limiter", "leveller"):
        # the stage had work to do: the plain stream differs
        plain = np.concatenate([c[0] for c in _single(m, kw, TEXTS[1], budgets[1], min(budgets), chunk)])
        assert not np.array_equal(plain, np.concatenate([c[0] for c in got[1]]))


def test_staggered_lanes_with_exact_stream_states():
    budgets, chunk, n_ref = EXACT
    m, kw = _model(n_ref)
    with m.exact_streaming():
        got, stats = _batch(m, kw, budgets, chunk)
        print("exact", budgets, chunk, stats)
        assert stats["order_launches"] > 0, stats
        _compare(got, lambda i: _single(m, kw, TEXTS[i], budgets[i], min(budgets), chunk), 24000, np.float32)


def _xvec_kw():
    """an x-vector-only voice (no reference frames), as tests/test_gpu_long_form.py uses"""
    if "xvec" not in _state:
        m, _kw = _model()
        g = torch.Generator().manual_seed(5)
        vcp = dict(ref_code=[None], ref_spk_embedding=[torch.randn(_state["cfg"].talker.hidden_size, generator=g).cuda()],
                   x_vector_only_mode=[True], icl_mode=[False])
        _state["xvec"] = dict(language="English", voice_clone_prompt=vcp, do_sample=False, temperature=1.0, top_k=0, top_p=1.0,
                              repetition_penalty=1.0, non_streaming_mode=False)
    return _state["xvec"]


def test_staggered_segments_of_a_long_form_stream():
    """long form takes the same layer's device rows (``device_audio=True``): three segments with their own frame limits on two lanes
    against the non-streaming call, through an s16 stage at 16 kHz, as tests/test_gpu_long_form.py compares them.  No segment
    passes 25 frames: every chunk is a slice of the decode of the segment's codes so far, which is what the one-shot call decodes.
    (Behind an ICL reference the two calls cut the reference's samples at different places, so the voice has none.)"""
    from fq3hip.long_form import LongFormSpec
    m, _kw = _model()
    kw = _xvec_kw()
    spec = LongFormSpec(max_chars=40, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=1e-4, lead_hops=1, tail_hops=2,
                        hold_hops=4)
    assert len(spec.split(LONG_TEXT)) == 3
    budgets = list(PLAIN[0][0])
    # (no end-of-speech before the longest limit: every segment runs to its own limit)
    lkw = dict(kw, lanes=2, long_form=spec, max_new_tokens=budgets, min_new_tokens=max(budgets))
    with m.audio_output(16000, "s16"):
        one, sr1 = m.generate_long_voice_clone(LONG_TEXT, **lkw)
        events = [(np.asarray(a).copy(), sr, tm) for a, sr, tm in m.generate_long_voice_clone_streaming(LONG_TEXT, chunk_size=PLAIN[0][1], **lkw)]
        stats = dict(m._stream_group_stats)
    print("long form", budgets, stats, len(events), one[0].size)
    assert stats["order_launches"] > 0, stats
    cat = np.concatenate([a for a, _sr, _tm in events])
    assert sr1 == 16000 and all(sr == 16000 for _a, sr, _tm in events)
    assert one[0].dtype == np.dtype("<i2") and cat.dtype == one[0].dtype and one[0].size > 0
    assert np.array_equal(cat, one[0])
    idx = [tm["segment_index"] for _a, _sr, tm in events]
    assert idx == sorted(idx) and idx[0] == 0 and idx[-1] == 2
    assert [tm["chunk_index"] for _a, _sr, tm in events] == list(range(len(events)))
    assert [tm["is_final"] for _a, _sr, tm in events] == [False] * (len(events) - 1) + [True]
