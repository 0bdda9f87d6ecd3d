"""GPU: the decode frame behind its preloaded kernel entry (csrc/decode_kernels.cuh, "kernel entry").

Every kernel of the frame takes its leading arguments as flat pointers / scalars (delivered in SGPRs at wave launch) and the rest
as a trailing struct; a launch helper splits GemvArgs / AttnArgs / the samplers' lists.  A swapped or mis-ordered argument changes ids:
12 sampled frames through the captured graph and through direct launches must be identical to each other, and in fp32 to the CPU
oracle.  Shapes: the tiny config (and its projection variant), a 70-token prompt in a 160-slot cache = 3 split-KV workers of which
two hold keys and one stays empty, so the o_proj merge prologue (PRO_COMBINE, n_part = 3), the predictor's two-token pass (M = 2),
attn_pred_kernel, attn_decode_kernel, both register samplers, frame_begin_kernel and embed_sum_kernel all run with real work.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_weights, synth_prompt

FRAMES, PROMPT, TRAILING, MAX_SEQ = 12, 70, 6, 160
TALKER = dict(temperature=0.9, top_k=50, top_p=1.0, do_sample=True)
PRED = dict(do_sample=True, top_k=50, top_p=1.0, temperature=0.9)


def _cfg(projection):
    return tiny_test_config(hidden=512, pred_hidden=256, heads=4, kv_heads=2) if projection else tiny_test_config()


def _noise(cfg):
    g = torch.Generator().manual_seed(21)
    tn = torch.empty(FRAMES + 1, cfg.talker.vocab_size).exponential_(1, generator=g)
    pn = torch.empty(FRAMES, cfg.num_code_groups - 1, cfg.predictor.vocab_size).exponential_(1, generator=g)
    return tn, pn


def _run(eng, cfg, dtype, prompt, tn, pn, graph):
    tie, tam, tth, tpe, _ = prompt
    logits, hidden = eng.prefill(tie[0].cuda().contiguous())
    V = cfg.talker.vocab_size
    tok = eng.sample(logits, sup_lo=max(0, V - 1024), sup_hi=V, keep_id=cfg.codec_eos_token_id, suppress_eos=True,
                     noise=tn[0].to(dtype).contiguous().cuda(), **TALKER)
    eng.decode_begin(first_token=int(tok), prefill_len=tie.shape[1], gen_step=0, past_hidden=hidden,
                     trailing_text=tth[0].cuda().contiguous(), tts_pad_embed=tpe.view(-1).cuda().contiguous(),
                     repetition_penalty=1.05, min_new_tokens=FRAMES, max_new_tokens=FRAMES,
                     talker_noise=tn[1:].to(dtype).contiguous().cuda(), pred_noise=pn.to(dtype).contiguous().cuda(),
                     noise_frames=FRAMES, **TALKER)
    if graph:
        eng.graph_capture()
    else:
        eng.graph_reset()
    eng.decode_frames(FRAMES)
    n, _done = eng.decode_poll()
    return eng.decode_codes(0, n).cpu()


@pytest.mark.parametrize("projection", [False, True], ids=["plain", "projection"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_frames_graph_direct_oracle(dtype, projection):
    from fq3hip.engine import Fq3Engine
    cfg = _cfg(projection)
    assert cfg.predictor_has_projection == projection
    W = synth_weights(cfg, 0, dtype)
    prompt = synth_prompt(cfg, PROMPT, TRAILING, 0, dtype=dtype)
    tn, pn = _noise(cfg)
    eng = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=MAX_SEQ, max_frames=64)
    eng.set_predictor_sampling(**PRED)
    by_graph = _run(eng, cfg, dtype, prompt, tn, pn, graph=True)
    direct = _run(eng, cfg, dtype, prompt, tn, pn, graph=False)
    assert by_graph.shape == (FRAMES, cfg.num_code_groups)
    assert torch.equal(by_graph, direct), "captured graph and direct launches disagree"
    assert len(set(by_graph[:, 0].tolist())) > 2            # it is sampling, not stuck on one id
    if dtype == torch.float32:
        from oracle import qwen3tts_oracle as O
        orc = O.OracleTTS(cfg, W, max_seq_len=MAX_SEQ)
        orc.pred_sampling = dict(PRED)
        sp = O.SamplingParams(max_new_tokens=FRAMES, min_new_tokens=FRAMES)
        tie, tam, tth, tpe, _ = prompt
        ref = orc.generate(tie, tam, tth, tpe, sp, talker_noise=tn, pred_noise=pn)
        assert ref.shape == by_graph.shape and torch.equal(by_graph, ref), "fp32 ids differ from the CPU oracle"


@pytest.mark.parametrize("projection", [False, True], ids=["plain", "projection"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_predictor_loop_immediate_mode(dtype, projection):
    """fq3_predictor_loop outside the fused loop (no DecodeState: the samplers take their policy and noise as immediate
    arguments) against the oracle's ids and logits, with the bounds of tests/test_gpu_decode.py::test_predictor_loop_matches_oracle."""
    from fq3hip.engine import Fq3Engine
    from oracle import qwen3tts_oracle as O
    cfg = _cfg(projection)
    W = synth_weights(cfg, 0, dtype)
    greedy = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0)
    orc = O.OracleTTS(cfg, W, max_seq_len=MAX_SEQ)
    orc.pred_sampling = dict(greedy)
    eng = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=MAX_SEQ, max_frames=64)
    eng.set_predictor_sampling(**greedy)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 2, cfg.talker.hidden_size, generator=g).to(dtype)
    o_ids, o_logits = orc.predictor_loop(x, return_logits=True)
    ids, lg = eng.predictor_loop(x.view(-1).cuda(), want_logits=True)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        assert torch.equal(ids.cpu(), o_ids)
        assert (lg.float().cpu() - o_logits.float()).abs().max() <= 5e-4
        # sampled, immediate noise: same noise -> same ids
        orc.pred_sampling = dict(PRED)
        eng.set_predictor_sampling(**PRED)
        noise = torch.empty(cfg.num_code_groups - 1, cfg.predictor.vocab_size).exponential_(1, generator=g)
        assert torch.equal(eng.predictor_loop(x.view(-1).cuda(), noise=noise.cuda()).cpu(), orc.predictor_loop(x, noise=noise))
    else:
        assert (lg[0].float().cpu() - o_logits[0].float()).abs().max() <= 0.15
