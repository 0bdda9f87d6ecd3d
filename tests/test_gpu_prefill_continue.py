"""GPU: fq3_prefill_continue and fq3_kv_copy through the engine -- two talker layers at the 0.6B and at the 1.7B dims.

A prompt prefilled whole (`prefill(x)`) against the same prompt prefilled in pieces (`prefill(x[:s])`, then
`prefill_continue(x[s:], s)`): logits, hidden state and EVERY K and V row of the last layer.

Bounds, fixed before anything ran:
* bf16, pieces against whole: 2^-6 x max(1, max|ref|) -- the bound tests/test_gpu_prefill_skinny.py uses for "the same arithmetic
  except for which token tile a row sits in" (packed against single): the GEMMs of a continuation run over another row count, so
  their tile / split-K choice and with it the fp32 summation order may differ; the attention's key splits add a merge.  Nothing
  promises bit identity; whether it came out identical is printed.
* bf16 against the fp32-arithmetic oracle: 0.025 x scale (the bound of the other bf16 prefill tests).
* fp32 against the oracle: 2e-4 x scale (tests/test_gpu_longprompt.py).
(1100, 1000) is there for the key splits: 100 new rows behind 1000 cached keys is the first size here at which the launcher cuts a
query block's key tiles over several workgroups and the merge launch runs (the other cases have fewer than 8 key tiles: one split).

Observed on the MI355X (a record): every case with one split, the three-chunk cases included, came out bit-identical to the whole
prefill at both sizes; (1100, 1000) differed by 9.15e-3 of the scale at most (bound 1.56e-2).  fp32 against the oracle: 6.5e-6."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip import _lib as L
from fq3hip.config import qwen3_tts_0p6b, qwen3_tts_1p7b
from fq3hip.weights import synth_weights, synth_prompt
from oracle import qwen3tts_oracle as O


def _cfg(size):
    cfg = qwen3_tts_0p6b() if size == "0p6b" else qwen3_tts_1p7b()
    cfg.talker.num_hidden_layers = 2
    cfg.predictor.num_hidden_layers = 1
    return cfg


def _setup(size, Lp, dtype=torch.bfloat16, max_seq=None):
    from fq3hip.engine import Fq3Engine
    cfg = _cfg(size)
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor"))
    tie, tam, _, _, _ = synth_prompt(cfg, Lp, 4, 0, dtype=dtype)
    tie = (tie * 30).to(dtype)                                   # O(1) activations
    eng = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=max_seq or Lp + 8, max_frames=8)
    return cfg, W, tie, tam, eng


def _snap(eng, cfg, out, Lp):
    k, v = eng.kv_export(cfg.talker.num_hidden_layers - 1, Lp)
    return out[0].float().cpu(), out[1].float().cpu(), k.float().cpu(), v.float().cpu()


@functools.lru_cache(maxsize=None)
def _oracle(size, Lp, dtype):
    """fp32 arithmetic on the same (bf16- or fp32-valued) weights: (logits, hidden) of the whole prompt.  Computed once per shape."""
    cfg = _cfg(size)
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor"))
    tie, tam, _, _, _ = synth_prompt(cfg, Lp, 4, 0, dtype=dtype)
    tie = (tie * 30).to(dtype)
    orc = O.OracleTTS(cfg, {k: v.float() for k, v in W.items()}, max_seq_len=Lp + 8)
    with torch.inference_mode():
        lo, ho, _, _ = orc.prefill(tie.float(), tam)
    return lo.float().view(-1), ho.float().view(-1)


NAMES = ("logits", "hidden", "K of the last layer", "V of the last layer")


def _check_pieces(size, Lp, cuts):
    cfg, W, tie, tam, eng = _setup(size, Lp)
    x = tie[0].cuda().contiguous()
    ref = _snap(eng, cfg, eng.prefill(x), Lp)
    torch.cuda.synchronize()
    out = eng.prefill(x[:cuts[0]].contiguous())
    for a, b in zip(cuts, cuts[1:] + [Lp]):
        out = eng.prefill_continue(x[a:b].contiguous(), a)
    got = _snap(eng, cfg, out, Lp)
    same = all(torch.equal(g, r) for g, r in zip(got, ref))
    worst = []
    for g, r, name in zip(got, ref, NAMES):
        d = float((g - r).abs().max())
        worst.append(d / max(1.0, float(r.abs().max())))
        assert d <= 2.0 ** -6 * max(1.0, float(r.abs().max())), (name, d)
    assert float(got[3].abs().amax(dim=(0, 2)).min()) > 0                  # every cache row written
    lo, ho = _oracle(size, Lp, torch.bfloat16)
    dh, dl = float((got[1] - ho).abs().max()), float((got[0] - lo).abs().max())
    print(f"[prefill_continue] {size} L={Lp} cuts={cuts}: bit-identical to the whole prefill: {same}; max rel diff {max(worst):.2e} "
          f"(bound {2.0 ** -6:.2e}); |hidden - oracle| {dh:.4f}, |logits - oracle| {dl:.4f}")
    assert dh <= 0.025 * max(1.0, float(ho.abs().max()))
    assert dl <= 0.025 * max(1.0, float(lo.abs().max()))
    eng.close()


@pytest.mark.parametrize("size", ["0p6b", "1p7b"])
@pytest.mark.parametrize("Lp,s", [(200, 64), (200, 37), (200, 130), (37, 16), (416, 200)])
def test_prefill_then_continue_matches_whole_prefill_bf16(size, Lp, s):
    _check_pieces(size, Lp, [s])


def test_continue_with_key_splits_matches_whole_prefill_bf16():
    _check_pieces("0p6b", 1100, [1000])


@pytest.mark.parametrize("size", ["0p6b", "1p7b"])
def test_three_chunks_bf16(size):
    _check_pieces(size, 200, [64, 128])


@pytest.mark.parametrize("Lp,s", [(200, 64), (37, 16)])
def test_continue_fp32_matches_oracle(Lp, s):
    cfg, W, tie, tam, eng = _setup("0p6b", Lp, dtype=torch.float32)
    x = tie[0].cuda().contiguous()
    eng.prefill(x[:s].contiguous())
    lg, hd = eng.prefill_continue(x[s:].contiguous(), s)
    lo, ho = _oracle("0p6b", Lp, torch.float32)
    dh, dl = float((hd.float().cpu() - ho).abs().max()), float((lg.float().cpu() - lo).abs().max())
    print(f"[prefill_continue] fp32 L={Lp} s={s}: |hidden - oracle| {dh:.2e}, |logits - oracle| {dl:.2e}")
    assert dh <= 2e-4 * max(1.0, float(ho.abs().max()))
    assert dl <= 2e-4 * max(1.0, float(lo.abs().max()))
    eng.close()


@pytest.mark.parametrize("mode", ["n<4", "prefill_mode 1"])
def test_token_walk_continuation(mode):
    """n < 4, or prefill_mode 1: the new rows walk through the decode kernels from position start."""
    Lp = 70
    s = 68 if mode == "n<4" else 40
    cfg, W, tie, tam, eng = _setup("0p6b", Lp)
    x = tie[0].cuda().contiguous()
    ref = _snap(eng, cfg, eng.prefill(x), Lp)
    eng.prefill(x[:s].contiguous())
    first = eng.kv_export(cfg.talker.num_hidden_layers - 1, s)
    if mode != "n<4":
        eng.set_prefill_mode(1)
    got = _snap(eng, cfg, eng.prefill_continue(x[s:].contiguous(), s), Lp)
    # the decode kernels against the oracle: 0.025 x scale (tests/test_gpu_decode.py holds both prefill modes to it); the K / V rows
    # against the matrix-core prefill's, which is held to the same bound: twice that
    lo, ho = _oracle("0p6b", Lp, torch.bfloat16)
    assert float((got[1] - ho).abs().max()) <= 0.025 * max(1.0, float(ho.abs().max()))
    assert float((got[0] - lo).abs().max()) <= 0.025 * max(1.0, float(lo.abs().max()))
    for i in (2, 3):
        assert float((got[i] - ref[i]).abs().max()) <= 0.05 * max(1.0, float(ref[i].abs().max())), NAMES[i]
        assert torch.equal(got[i][:, :s], first[i - 2].float().cpu())          # rows below start: still the first piece's
    assert float(got[3].abs().amax(dim=(0, 2)).min()) > 0
    eng.close()


def test_kv_copy_into_another_pool_then_continue_is_bit_identical():
    from fq3hip.engine import Fq3Engine, Fq3KvPool
    Lp, s = 200, 130
    cfg, W, tie, tam, src = _setup("0p6b", Lp, max_seq=256)
    x = tie[0].cuda().contiguous()
    nl = cfg.talker.num_hidden_layers
    src.prefill(x[:s].contiguous())
    src_blocks = src.kv_blocks()
    src_rows = [src.kv_export(i, s) for i in range(nl)]
    pool = Fq3KvPool(cfg, 4, dtype=torch.bfloat16)
    dst = Fq3Engine(cfg, W, device="cuda", dtype=torch.bfloat16, max_seq_len=256, max_frames=8, share=src, pool=pool)
    assert dst.kv_blocks() == 0
    dst.kv_copy(src, s)
    assert dst.kv_blocks() == 3 and src.kv_blocks() == src_blocks
    st = pool.stats()
    assert st["blocks"] == 4 and st["free"] == 1 and st["high_water"] == 3
    for i in range(nl):                                          # the source's rows stay as they were
        k, v = src.kv_export(i, s)
        assert torch.equal(k, src_rows[i][0]) and torch.equal(v, src_rows[i][1])
    a = dst.prefill_continue(x[s:].contiguous(), s)
    b = src.prefill_continue(x[s:].contiguous(), s)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in range(nl):
        ka, va = dst.kv_export(i, Lp)
        kb, vb = src.kv_export(i, Lp)
        assert torch.equal(ka, kb) and torch.equal(va, vb), i
    assert pool.stats()["free"] == 0 and dst.kv_blocks() == 4
    # a pool that is short: FQ3_ENOMEM and nothing taken
    other = Fq3Engine(cfg, W, device="cuda", dtype=torch.bfloat16, max_seq_len=256, max_frames=8, share=src, pool=pool)
    with pytest.raises(L.Fq3Error) as e:
        other.kv_copy(src, s)
    assert e.value.code == L.FQ3_ENOMEM and other.kv_blocks() == 0 and pool.stats()["free"] == 0
    for e_ in (other, dst, src):
        e_.close()
    pool.close()


def test_error_codes():
    from fq3hip.engine import Fq3Engine, Fq3KvPool
    cfg, W, tie, tam, eng = _setup("0p6b", 100, max_seq=128)
    x = tie[0].cuda().contiguous()
    lib, st = eng.lib, eng._stream()
    H = cfg.talker.hidden_size
    out = eng.new(H)

    def cont(ctx, ptr, start, n):
        return lib.fq3_prefill_continue(ctx, ptr, start, n, None, out.data_ptr(), st)
    assert cont(None, x.data_ptr(), 0, 4) == L.FQ3_EINVAL
    assert cont(eng.ctx, None, 0, 4) == L.FQ3_EINVAL
    assert cont(eng.ctx, x.data_ptr(), 0, 0) == L.FQ3_EINVAL
    assert cont(eng.ctx, x.data_ptr(), -1, 4) == L.FQ3_EINVAL
    assert cont(eng.ctx, x.data_ptr(), 100, 29) == L.FQ3_ETOOLONG
    assert b"Input is too long: prefill has 129 tokens but max_seq_len=128" in lib.fq3_last_error()
    pool = Fq3KvPool(cfg, 2, dtype=torch.bfloat16)
    pooled = Fq3Engine(cfg, W, device="cuda", dtype=torch.bfloat16, max_seq_len=128, max_frames=8, share=eng, pool=pool)
    assert cont(pooled.ctx, x.data_ptr(), 65, 4) == L.FQ3_ESTATE          # owns 0 blocks, rows [0, 65) need 2
    pooled.kv_reserve(64)
    assert cont(pooled.ctx, x.data_ptr(), 65, 4) == L.FQ3_ESTATE          # owns 1
    assert lib.fq3_kv_copy(None, eng.ctx, 10, st) == L.FQ3_EINVAL
    assert lib.fq3_kv_copy(eng.ctx, None, 10, st) == L.FQ3_EINVAL
    assert lib.fq3_kv_copy(eng.ctx, eng.ctx, 10, st) == L.FQ3_EINVAL
    assert lib.fq3_kv_copy(eng.ctx, pooled.ctx, 65, st) == L.FQ3_EINVAL    # L outside the source cache (it owns one block)
    assert lib.fq3_kv_copy(eng.ctx, pooled.ctx, -1, st) == L.FQ3_EINVAL
    f32 = Fq3Engine(cfg, synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor")), device="cuda", dtype=torch.float32,
                    max_seq_len=128, max_frames=8)
    assert lib.fq3_kv_copy(f32.ctx, eng.ctx, 10, st) == L.FQ3_EINVAL       # contexts of different shape
    small = Fq3Engine(cfg, W, device="cuda", dtype=torch.bfloat16, max_seq_len=64, max_frames=8, share=eng)
    assert lib.fq3_kv_copy(small.ctx, eng.ctx, 100, st) == L.FQ3_ETOOLONG
    assert b"Input is too long" in lib.fq3_last_error()
    torch.cuda.synchronize()
    for e in (small, f32, pooled, eng):
        e.close()
    pool.close()


def test_two_identical_continuations_give_identical_bits():
    Lp, s = 1100, 1000                                           # key splits + merge
    cfg, W, tie, tam, eng = _setup("0p6b", Lp)
    x = tie[0].cuda().contiguous()
    eng.prefill(x[:s].contiguous())
    a = _snap(eng, cfg, eng.prefill_continue(x[s:].contiguous(), s), Lp)
    b = _snap(eng, cfg, eng.prefill_continue(x[s:].contiguous(), s), Lp)
    for g, r, name in zip(a, b, NAMES):
        assert torch.equal(g, r), name
    eng.close()
