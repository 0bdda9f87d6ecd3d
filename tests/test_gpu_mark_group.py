"""GPU: mark_embed_group_kernel behind fq3_mark_push_group.  The yardstick is twin ``Watermark`` objects driven
by single pushes only: a row of a group equals its single push bit for bit, state included.  One case against the float64 reference."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mark_ref as R
from fq3hip import _lib, watermark as W

LENS = [0, 1, 255, 256, 257, 511, 512, 3839, 3840, 3841, 15360]          # the edges of the hop (256) and of a workgroup (3840), one chunk
# rows 0 .. 2 per round: an empty push between two others (equal neighbours in wg0), one that completes no hop, a final push of nothing
HEAD = [[15360, 0, 257], [1, 3841, 255], [0, 511, 3840]]


@functools.lru_cache(None)
def _x():
    return torch.from_numpy(np.random.default_rng(11).uniform(-1.0, 1.0, 50000).astype(np.float32)).cuda()


def _marks(B):
    return [W.Watermark(0x1234567800000000 + 977 * b, (0.05, 0.1, 0.3)[b % 3], "cuda") for b in range(B)]


def _same(got, want):
    for b, (g, w) in enumerate(zip(got, want, strict=True)):
        assert g.shape == w.shape and torch.equal(g, w), (b, g.shape, w.shape)


@pytest.mark.parametrize("B", [1, 3, 32])
def test_rows_equal_their_single_pushes(B):
    x, rows, twins = _x(), _marks(B), _marks(B)
    for r in range(3):
        ns = [HEAD[r][b] if b < 3 else LENS[(b + 4 * r) % len(LENS)] for b in range(B)]
        starts = [1 + 2 * b + 16001 * r for b in range(B)]                 # x[1:], x[3:], ...: not 16-byte aligned
        pcms, finals = [x[s:s + n] for s, n in zip(starts, ns)], [r == 2] * B
        _same(W.push_group(rows, pcms, finals), [t.push(p, f) for t, p, f in zip(twins, pcms, finals)])
        assert [(m.n_in, m.n_out, m.finished) for m in rows] == [(t.n_in, t.n_out, t.finished) for t in twins]
    assert all(m.n_out == m.n_in for m in rows)
    if B == 32:                                                            # forty rows take two calls of the library
        rows, twins, pcms = _marks(40), _marks(40), [x[b:b + 3000 + 7 * b] for b in range(40)]
        _same(W.push_group(rows, pcms, [True] * 40), [t.push(p, True) for t, p in zip(twins, pcms)])


@pytest.mark.parametrize("row", [0, 1, 2])
def test_group_against_the_float64_reference(row):
    xs = [R.voiced(0.6)[300 + 4000 * b:4300 + 4000 * b] for b in range(3)]                  # three rows of 4000 samples under three keys
    marks = [W.Watermark(0x0123456789ABCDEF + b, 0.1, "cuda") for b in range(3)]
    got = W.push_group(marks, [torch.from_numpy(np.array(v)).cuda() for v in xs], [True] * 3)[row].cpu().numpy()
    key, a = 0x0123456789ABCDEF + row, float(np.float32(0.1))
    ref = R.embed(xs[row], key, a)
    bound = 4.0 * float(np.max(np.abs(R.embed(xs[row], key, a, np.float32) - ref)))      # the rule of test_gpu_watermark.py
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"group row {row}: max |device - ref64| = {err:.3e}, bound = {bound:.3e}")
    assert len(got) == 4000 and err < bound


@pytest.mark.parametrize("bad", ["capacity", "finished"])
def test_all_or_nothing(bad):
    x, rows, twins, lib = _x(), _marks(3), _marks(3), _lib.load()
    [m.push(x[5:1005]) for m in rows + twins]
    if bad == "finished":
        rows[2].push(x[1005:1100], final=True)
    pcms = [x[1005 + b:5000 + b] for b in range(3)]
    caps = [W.count(1000 + int(p.numel()), False) - m.n_out for m, p in zip(rows, pcms)]
    caps[2] -= bad == "capacity"                                           # one sample short
    out, n_out = torch.empty(3 * 4096, dtype=torch.float32, device="cuda"), (C.c_int64 * 3)()
    rc = lib.fq3_mark_push_group((C.c_void_p * 3)(*[m._h.value for m in rows]), 3, (C.c_void_p * 3)(*[p.data_ptr() for p in pcms]),
                                 (C.c_int64 * 3)(*[int(p.numel()) for p in pcms]), (C.c_int * 3)(0, 0, 0),
                                 (C.c_void_p * 3)(*[out.data_ptr() + 4 * 4096 * b for b in range(3)]), (C.c_int64 * 3)(*caps), n_out,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == (_lib.FQ3_EINVAL if bad == "capacity" else _lib.FQ3_ESTATE)
    _same([m.push(p, True) for m, p in zip(rows[:2], pcms)], [t.push(p, True) for t, p in zip(twins[:2], pcms)])   # no object moved


# ---- through the model: the batch entry points' watermark= ------------------------------------------------------------------------
TEXTS = ["The quick brown fox jumps. Over the lazy dog it goes!", "A second, shorter line to speak.", "And then it sleeps for a while, or so they say?"]
KW = dict(do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0, max_new_tokens=30, min_new_tokens=30)    # 2.4 s


@functools.lru_cache(None)
def _model():
    from test_gpu_audio_out import _tiny_model                            # the tiny fp32 custom-voice model of test_through_the_model
    m = _tiny_model()
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    return m


def _single(x, spec):
    return W.Watermark(spec.key, spec.strength, "cuda").push(torch.from_numpy(np.asarray(x)).cuda(), final=True).cpu()


def test_batch_streaming_marks_each_row_under_its_own_key():
    m, sa, sb = _model(), W.MarkSpec(0x0123456789ABCDEF, 0.1), W.MarkSpec(77, 0.2)

    def batch(**extra):
        ev = {i: [] for i in range(3)}
        for i, arr, _sr, _tm in m.generate_custom_voice_batch_streaming(TEXTS, "bob", "English", non_streaming_mode=False, lanes=3,
                                                                        chunk_size=4, seeds=0, **extra, **KW):
            ev[i].append(np.asarray(arr).copy())
        return [torch.from_numpy(np.concatenate(ev[i])) for i in range(3)]
    with m.exact_streaming():
        plain, got = batch(), batch(watermark=[sa, None, sb])
        for i, sp in ((0, sa), (2, sb)):
            with m.seeded(i), m.watermark(sp.key, sp.strength):
                want = np.concatenate([np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(
                    TEXTS[i], "bob", "English", chunk_size=4, non_streaming_mode=False, **KW)])
            assert torch.equal(got[i], torch.from_numpy(want)) and not torch.equal(got[i], plain[i]), i
    assert torch.equal(got[1], plain[1])
    assert [m.detect_watermark(got[i].numpy(), 24000, k).present for i, k in ((0, sa.key), (1, sa.key), (2, sa.key), (0, sb.key))] == [True, False, False, False]


def test_marked_staged_and_plain_rows_share_launches_behind_a_limiter():
    """Frame limits 8 / 38 / 30 on two lanes at chunks of 4 frames (the shape of test_stream_groups_cpu.NAMED: the lane of text 0 is
    re-used by text 2 while text 1 decodes), a limiter on: text 0 is marked and lands in the limiter's buffers, text 1 leaves through
    its own s16 stage, text 2 is plain.  Every utterance is its own single stream under the same settings, bit for bit."""
    from fq3hip.audio_out import AudioOutSpec
    m, sa, s16, budgets = _model(), W.MarkSpec(0x0123456789ABCDEF, 0.1), AudioOutSpec(16000, "s16"), [8, 38, 30]
    kw = dict(KW, min_new_tokens=min(budgets))
    with m.limiter():
        ev = {i: [] for i in range(3)}
        for i, arr, _sr, _tm in m.generate_custom_voice_batch_streaming(TEXTS, "bob", "English", non_streaming_mode=False, lanes=2,
                                                                        chunk_size=4, seeds=0, watermark=[sa, None, None],
                                                                        output=[None, s16, None], **dict(kw, max_new_tokens=budgets)):
            ev[i].append(np.asarray(arr).copy())
        print(m._stream_group_stats, [[len(a) for a in ev[i]] for i in range(3)])
        for i, ctx in enumerate((m.watermark(sa.key, sa.strength), m.audio_output(16000, "s16"), contextlib.nullcontext())):
            with m.seeded(i), ctx:
                want = np.concatenate([np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(
                    TEXTS[i], "bob", "English", chunk_size=4, non_streaming_mode=False, **dict(kw, max_new_tokens=budgets[i]))])
            got = np.concatenate(ev[i])
            assert got.dtype == want.dtype == (np.dtype("<i2") if i == 1 else np.float32), i
            assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), (i, len(got), len(want))


def test_one_shot_batch_refusals_and_long_form():
    from fq3hip.audio_out import AudioOutSpec
    from fq3hip.long_form import LongFormSpec as LF
    m, sa, sb = _model(), W.MarkSpec(0x0123456789ABCDEF, 0.1), W.MarkSpec(77, 0.2)
    plain, got = (m.generate_custom_voice_batch(TEXTS, "bob", "English", lanes=3, seeds=0, **kw, **KW) for kw in ({}, dict(watermark=sa)))
    for i in range(3):
        assert torch.equal(torch.from_numpy(got[i][0][0]), _single(plain[i][0][0], sa)), i
    with m.watermark(sa.key), pytest.raises(ValueError, match="watermark="):
        m.generate_custom_voice_batch(TEXTS, "bob", "English", lanes=3, **KW)
    with pytest.raises(ValueError, match="speed"):
        m.generate_custom_voice_batch(TEXTS, "bob", "English", lanes=3, watermark=[None, sa, None],
                                      output=[None, AudioOutSpec(8000, "mulaw", 1.25), None], **KW)
    # long form for many texts: the public signatures are pinned (test_join_group_cpu.py), so the marks go in at _run_long_batch_full
    lf = LF(max_chars=40, pause_ms={"clause": 20, "sentence": 50, "paragraph": 80}, threshold=1e-4, lead_hops=1, tail_hops=2, hold_hops=4)
    texts = [TEXTS[0] + " And then it sleeps for a while?", TEXTS[2]]
    joined = m.generate_long_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=0, long_form=lf, **dict(KW, max_new_tokens=22, min_new_tokens=22))
    with torch.inference_mode():
        spec, segs, seeds, outputs = m._long_batch_setup(texts, lf, 0, None)
        prepared = m._prepare_long_batch(segs, lambda t, ts: m._prepare_custom_batch(ts, "bob", "English", None, None))
        marked = m._run_long_batch_full(prepared, segs, spec, m._gen_kwargs(22, 22, 1.0, 0, 1.0, False, 1.0), 3, seeds, outputs,
                                        marks=m._batch_marks([sa, sb], 2))
    for t, sp in enumerate((sa, sb)):
        assert torch.equal(torch.from_numpy(marked[t][0][0]), _single(joined[t][0][0], sp)), t
