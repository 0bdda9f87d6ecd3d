"""GPU: seeded sampling through the engine, the decode loops, the batch scheduler and the public interface.
Every comparison is ``torch.equal`` / ``np.array_equal``: the feature fills the noise rings the verified samplers read and adds no
arithmetic to the decode path, so codes are a pure function of (prompt, policy, seed) within one arithmetic path.

Sampled decoding at temperature 0.9, top-k 20, a sampling predictor; one batch lane with top_p 0.8."""
import copy
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_prompt, synth_weights

DTYPES = [torch.float32, torch.bfloat16]
POLICY = dict(do_sample=True, top_k=20, top_p=1.0, temperature=0.9)


class Solo:
    """One engine with the graph wrappers ``fast_generate`` takes (no model around it)."""

    def __init__(self, cfg, dtype, max_seq=160, max_frames=96, share=None):
        from fq3hip.engine import Fq3Engine
        from fq3hip.predictor_graph import PredictorGraph
        from fq3hip.talker_graph import TalkerGraph
        self.cfg, self.dtype = cfg, dtype
        self.W = share.W if share is not None else synth_weights(cfg, 0, dtype)
        self.eng = Fq3Engine(cfg, self.W, device="cuda", dtype=dtype, max_seq_len=max_seq, max_frames=max_frames,
                             share=share.eng if share is not None else None)
        self.pg, self.tg = PredictorGraph(self.eng, **POLICY), TalkerGraph(self.eng)
        self.talker = types.SimpleNamespace()
        self.config = types.SimpleNamespace(vocab_size=cfg.talker.vocab_size, codec_eos_token_id=cfg.codec_eos_token_id)


def _prompt(cfg, dtype, seed, plen, n_pad=0, trailing=4):
    tie, tam, tth, tpe, _ = synth_prompt(cfg, plen, trailing, 0, dtype=dtype, seed=seed)
    tam = tam.clone()
    tam[0, :n_pad] = 0
    return (tie * 30).to(dtype).cuda(), tam.cuda(), tth.cuda(), tpe.cuda()


def _kw(frames, top_p=1.0, min_new=None):
    return dict(max_new_tokens=frames, min_new_tokens=frames if min_new is None else min_new, temperature=0.9, top_k=20, top_p=top_p,
                do_sample=True, repetition_penalty=1.05)


def _generate(s: Solo, prompt, seed, **kw):
    from fq3hip.generate import fast_generate
    tie, tam, tth, tpe = prompt
    codes, _t = fast_generate(s.talker, tie, tam, tth, tpe, s.config, s.pg, s.tg, seed=seed, **kw)
    return codes.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_seeded_loop_equals_explicit_noise_path(dtype):
    """Tie to the verified samplers: a caller-owned 16-row ring filled by ``noise_fill`` and handed to ``decode_begin`` (the explicit-noise
    path of tests/test_gpu_batch.py::_arm) gives the codes of ``fast_generate(seed=...)`` with its own 64-row ring."""
    cfg = tiny_test_config()
    s = Solo(cfg, dtype)
    eng, seed, frames = s.eng, 20240607, 16
    V, G1, Vp = cfg.talker.vocab_size, cfg.num_code_groups - 1, cfg.predictor.vocab_size
    tie, tam, tth, tpe = prompt = _prompt(cfg, dtype, 11, 20)
    tn, pn = eng.new(16, V), eng.new(16, G1, Vp)
    eng.noise_fill(tn, pn, seed, 0, 16)
    first = eng.noise_first(seed)
    eng.set_predictor_sampling(**POLICY)
    x = tie[0].contiguous()
    eng.set_generation_state(0, 0)
    logits, hidden = eng.prefill(x, n_pad=0)
    skw = dict(temperature=0.9, top_k=20, top_p=1.0, do_sample=True)
    tok = eng.sample(logits, sup_lo=max(0, V - 1024), sup_hi=V, keep_id=cfg.codec_eos_token_id, suppress_eos=True, noise=first, **skw)
    eng.decode_begin(first_token=int(tok), prefill_len=x.shape[0], gen_step=0, past_hidden=hidden, trailing_text=tth[0].contiguous(),
                     tts_pad_embed=tpe.view(-1).contiguous(), repetition_penalty=1.05, min_new_tokens=frames, max_new_tokens=frames,
                     talker_noise=tn, pred_noise=pn, noise_frames=16, **skw)
    eng.graph_reset()
    eng.decode_frames(frames)
    n, _done = eng.decode_poll()
    explicit = eng.decode_codes(0, n).cpu()
    assert n == frames
    seeded = _generate(s, prompt, seed, **_kw(frames))
    assert torch.equal(seeded, explicit), "the seeded loop and the explicit-noise path disagree"
    assert torch.equal(_generate(s, prompt, seed, **_kw(frames)), seeded), "the same seed twice gave different codes"
    assert not torch.equal(_generate(s, prompt, seed + 1, **_kw(frames)), seeded), "another seed gave the same codes"
    assert torch.equal(_generate(s, prompt, seed, parity_mode=True, **_kw(frames)), seeded), "direct launches and the graph disagree"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_codes_do_not_depend_on_call_slicing(dtype):
    """70 frames, across the 64-frame ring boundary: one ``run_frames`` call == one frame per call == ``fast_generate`` ==
    ``fast_generate_streaming`` at chunk 4 and chunk 12."""
    from fq3hip.generate import _prefill_and_arm, run_frames
    from fq3hip.streaming import fast_generate_streaming, parity_generate_streaming
    cfg = tiny_test_config()
    s = Solo(cfg, dtype)
    seed, frames = 2 ** 63 + 5, 70
    tie, tam, tth, tpe = prompt = _prompt(cfg, dtype, 12, 33, n_pad=4)
    kw = _kw(frames)

    def sliced(step):
        eng, tn, pn, max_frames = _prefill_and_arm(s.talker, tie, tam, tth, tpe, s.config, s.pg, s.tg, kw["max_new_tokens"],
                                                   kw["min_new_tokens"], kw["temperature"], kw["top_k"], kw["top_p"], kw["do_sample"],
                                                   kw["repetition_penalty"], use_graph=True, seed=seed)
        issued = 0
        while issued < max_frames:
            issued = run_frames(eng, tn, pn, issued, min(step, max_frames - issued), seed)
        n, _ = eng.decode_poll()
        return eng.decode_codes(0, n).cpu()
    ref = sliced(frames)
    assert ref.shape[0] == frames
    assert torch.equal(sliced(1), ref), "one frame per call differs from one call"
    assert torch.equal(_generate(s, prompt, seed, **kw), ref), "fast_generate differs"
    for chunk in (4, 12):
        got = torch.cat([c.cpu() for c, _tm in fast_generate_streaming(s.talker, tie, tam, tth, tpe, s.config, s.pg, s.tg,
                                                                       chunk_size=chunk, seed=seed, **kw)])
        assert torch.equal(got, ref), f"streaming at chunk {chunk} differs"
    got = torch.cat([c.cpu() for c, _tm in parity_generate_streaming(s.talker, tie, tam, tth, tpe, s.config, chunk_size=12, predictor_graph=s.pg,
                                                                     talker_graph=s.tg, seed=seed, **kw)])
    assert torch.equal(got, ref), "seeded parity streaming (direct launches) differs from the graph path"


def _requests():
    """(rid, prompt seed, prompt rows, left pad, frames, top_p, sampling seed): three seeded requests of different prompt lengths, pads
    and budgets -- one across the ring boundary, one with nucleus sampling -- an unseeded one, and a late seeded one for a re-armed lane."""
    return [("a", 21, 20, 0, 9, 1.0, 7), ("b", 22, 33, 4, 70, 1.0, 2 ** 64 - 1), ("c", 23, 70, 2, 14, 0.8, 123456789012345),
            ("u", 24, 25, 0, 12, 1.0, None), ("late", 25, 18, 0, 11, 1.0, 99)]


@pytest.mark.parametrize("dtype,staged", [(torch.float32, False), (torch.bfloat16, True)], ids=["fp32", "bf16_mfma0_staged"])
def test_batch_lanes_equal_single_stream_seeded_runs(dtype, staged):
    """Four lanes: every seeded request gives the codes of its own single-stream seeded run -- whatever its lane and neighbours (the
    requests in permuted order), beside an unseeded lane, and in a lane re-armed after its first tenant finished.  fp32 on the default
    path without spare contexts (the lanes prefill themselves); bf16 with ``mfma`` 0 and spare contexts (staged prefill + hand-over)."""
    from fq3hip.batching import BatchDecoder, BatchRequest
    cfg = tiny_test_config()
    solo = Solo(cfg, dtype)
    reqs = {r[0]: r for r in _requests()}
    prompts = {rid: _prompt(cfg, dtype, ps, plen, pad) for rid, ps, plen, pad, _f, _p, _s in reqs.values()}
    want = {rid: _generate(solo, prompts[rid], sd, **_kw(fr, tp)) for rid, _ps, _pl, _pad, fr, tp, sd in reqs.values() if sd is not None}
    assert want["b"].shape[0] == 70
    lanes = [Solo(cfg, dtype, share=solo) for _ in range(4 + (2 if staged else 0))]
    dec = BatchDecoder([l.eng for l in lanes[:4]], predictor_policy=dict(POLICY), staging=[l.eng for l in lanes[4:]] or None)
    if dtype == torch.bfloat16:
        dec.batch.set_option("mfma", 0)                    # the bit-identity property belongs to the VALU GEMVs

    def run(order):
        batch = []
        for rid in order:
            _rid, _ps, _pl, _pad, fr, tp, sd = reqs[rid]
            tie, tam, tth, tpe = prompts[rid]
            batch.append(BatchRequest(rid, solo.talker, tie, tam, tth, tpe, solo.config, _kw(fr, tp), seed=sd))
        got = {}
        for rid, codes, timing in dec.run(batch):
            assert "error" not in timing, timing
            got[rid] = codes.cpu()
        return got

    for order in (["a", "b", "c", "u"], ["u", "c", "a", "b"], ["a", "b", "c", "u", "late"]):     # the last: a lane is re-armed
        got = run(order)
        assert sorted(got) == sorted(order)
        for rid in order:
            if rid in want:
                assert torch.equal(got[rid], want[rid]), f"{order}: request {rid} differs from its single-stream seeded run"
        assert got["u"].shape[0] == 12


def _tts_cfg():
    cfg = copy.deepcopy(tiny_test_config())
    cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "1b7"
    cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
    return cfg


def _model(cfg, dtype, **kw):
    from fq3hip.model import FasterQwen3TTS
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "codec", "text"))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=dtype, max_seq_len=200, codec_max_frames=128, max_frames=96, **kw)
    m.predictor_graph.do_sample, m.predictor_graph.top_k, m.predictor_graph.temperature = True, 20, 0.9
    return m


class _Starved:
    """A feeder that hands out ONE id each time the session blocks on it: every frame waits for its text row (the host's gate holds the
    frame), with nothing queued on the device meanwhile."""

    def __new__(cls, ids):
        from fq3hip.text_stream import TextFeeder

        class F(TextFeeder):
            def __init__(self, ids):
                super().__init__()
                self._todo, self.blocked = list(ids), 0

            def take(self, block=False, limit=None, timeout=None):
                if block and not self._ids and not self._closed:
                    self.blocked += 1
                    if self._todo:
                        self.feed_ids([self._todo.pop(0)])
                    else:
                        self.close()
                return super().take(block=False, limit=limit)
        return F(ids)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_incremental_text_equals_whole_text(dtype):
    """A seeded ``stream_custom_voice`` fed (a) in pieces cut inside words, all at hand, and (b) one token per blocking wait -- every frame
    held until its row arrives -- yields the audio chunks of the whole-text seeded call; 70 frames cross the ring boundary."""
    cfg = _tts_cfg()
    m = _model(cfg, dtype)
    text = "".join(chr(97 + (i * 7) % 26) if i % 6 != 5 else " " for i in range(60))
    kw = dict(max_new_tokens=70, min_new_tokens=70, chunk_size=12, temperature=0.9, top_k=20, repetition_penalty=1.05)

    def chunks(gen):
        return [(np.asarray(a).copy(), tm["chunk_steps"], tm["is_final"]) for a, _sr, tm in gen]
    with m.seeded(31337):
        ref = chunks(m.generate_custom_voice_streaming(text, "bob", "English", non_streaming_mode=False, **kw))
        assert sum(r[1] for r in ref) == 70
        pieces = [text[i:i + 7] for i in range(0, len(text), 7)]
        starved = _Starved(m._text_tokenize()(text))
        for name, src in (("pieces", iter(pieces)), ("starved", starved)):
            got = chunks(m.stream_custom_voice(src, "bob", "English", **kw))
            assert len(got) == len(ref), (name, len(got), len(ref))
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g[1:] == r[1:] and g[0].shape == r[0].shape and np.array_equal(g[0], r[0]), f"{name}: chunk {i} differs"
        assert starved.blocked >= 59, "the starved feeder must have been waited on once per row"
    assert m._seed is None
    with m.seeded(31338):
        other = chunks(m.generate_custom_voice_streaming(text, "bob", "English", non_streaming_mode=False, **kw))
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(other, ref)), "the seed must matter"


def test_public_batch_seeds_equal_single_seeded_calls():
    """``generate_custom_voice_batch(texts, ..., seeds=5)`` == the single calls under ``seeded(5 + i)``, fp32: bit-identical waveforms;
    a list of seeds with a None in it leaves that utterance unseeded and the others as they were."""
    cfg = _tts_cfg()
    m = _model(cfg, torch.float32)
    texts = ["One.", "A second, longer line to speak.", "Three words here.", "Four.", "The fifth and last line of this batch."]
    kw = dict(temperature=0.9, top_k=20, repetition_penalty=1.05, min_new_tokens=2, max_new_tokens=18)
    single = []
    for i, t in enumerate(texts):
        with m.seeded(5 + i):
            single.append(m.generate_custom_voice(t, "bob", "English", **kw))
    batch = m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=5, **kw)
    mixed = m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=[5, None, 7, 8, 9], **kw)
    for i, ((wa, sra), (wb, srb), (wc, _src)) in enumerate(zip(single, batch, mixed)):
        assert sra == srb and wa[0].shape == wb[0].shape and np.array_equal(wa[0], wb[0]), f"utterance {i}"
        if i != 1:
            assert np.array_equal(wa[0], wc[0]), f"utterance {i} beside an unseeded one"
    with m.seeded(6):
        again = m.generate_custom_voice(texts[1], "bob", "English", **kw)
    assert np.array_equal(again[0][0], single[1][0][0])
    with pytest.raises(ValueError):
        m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=[1, 2], **kw)
    with pytest.raises(ValueError):
        m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=2 ** 64, **kw)
