"""GPU: fq3_prefill_continue_batch through the engine -- two talker layers at the 0.6B dims (tests/test_gpu_prefill_continue.py's
configs, prompts and oracle).

Member q of a pack is a prompt of Lp[q] rows whose first start[q] rows were prefilled into its context (`prefill(x[:s])`); the pack
then continues all members in one call.  Bounds, fixed before anything ran:
* fp32 against the oracle: 2e-4 x scale; bf16 against the oracle: 0.025 x scale (the bounds of tests/test_gpu_prefill_continue.py).
* bf16 against single fq3_prefill_continue calls of the same (start, n): BIT-IDENTICAL.  The pack is chosen so that every key split is
  1 (at most 4 key tiles per member) and the packed rows stay <= 416: the attention is then flash_prefill_cont_kernel's arithmetic in
  its order (tests/test_gpu_prefill_pack_cont_reference.py), and the weight-stationary GEMMs treat a row alike at any row count.
* the same call twice: identical bits, key splits and merge included.

Observed on the MI355X (a record): fp32 against the oracle 9.1e-6 at most; bf16 hidden 3.9e-2 and logits 3.7e-2 at most in absolute
terms (the bounds scale with max |ref| > 1), the same figures with one pool and with private caches; the pack equalled the single calls
bit for bit."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip import _lib as L
from fq3hip.weights import synth_weights, synth_prompt
from test_gpu_prefill_continue import _cfg, _oracle

STARTS = (0, 40, 64, 130)
LPS = (50, 100, 134, 200)                    # new rows 50, 60, 70, 70: 250 packed rows; at most 4 key tiles per member


def _members(dtype, lps, max_seq, pooled=True, blocks=None):
    """Contexts on ONE weight table (and one KV pool), one prompt each."""
    from fq3hip.engine import Fq3Engine, Fq3KvPool
    cfg = _cfg("0p6b")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor"))
    pool = Fq3KvPool(cfg, blocks or len(lps) * ((max_seq + 63) // 64), dtype=dtype) if pooled else None
    first = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=max_seq, max_frames=8, pool=pool)
    engs = [first] + [Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=max_seq, max_frames=8, share=first, pool=pool)
                      for _ in lps[1:]]
    xs = []
    for Lp in lps:
        tie, _tam, _, _, _ = synth_prompt(cfg, Lp, 4, 0, dtype=dtype)
        xs.append((tie * 30).to(dtype)[0].cuda().contiguous())
    return cfg, engs, xs, pool


def _close(engs, pool):
    torch.cuda.synchronize()
    for e in reversed(engs):
        e.close()
    if pool is not None:
        pool.close()


def _prefix(engs, xs, starts):
    for e, x, s in zip(engs, xs, starts):
        e.kv_release(0)
        if s:
            e.prefill(x[:s].contiguous(), want_logits=False)


def _pack(engs, xs, starts):
    from fq3hip.engine import Fq3Engine
    return Fq3Engine.prefill_continue_batch(engs, [x[s:].contiguous() for x, s in zip(xs, starts)], list(starts))


def _against_oracle(dtype, bound, pooled):
    cfg, engs, xs, pool = _members(dtype, LPS, 256, pooled=pooled)
    _prefix(engs, xs, STARTS)
    outs = _pack(engs, xs, STARTS)
    for q, ((lg, hd), Lp) in enumerate(zip(outs, LPS)):
        lo, ho = _oracle("0p6b", Lp, dtype)
        dh, dl = float((hd.float().cpu() - ho).abs().max()), float((lg.float().cpu() - lo).abs().max())
        print(f"[prefill_continue_batch] {dtype} pooled={pooled} member {q} (start {STARTS[q]}, n {Lp - STARTS[q]}): |hidden - oracle| {dh:.3e}, "
              f"|logits - oracle| {dl:.3e}")
        assert dh <= bound * max(1.0, float(ho.abs().max())), (q, dh)
        assert dl <= bound * max(1.0, float(lo.abs().max())), (q, dl)
        k, v = engs[q].kv_export(cfg.talker.num_hidden_layers - 1, Lp)
        assert float(v.float().abs().amax(dim=(0, 2)).min()) > 0            # every cache row written
    _close(engs, pool)


def test_pack_of_four_fp32_matches_the_oracle():
    _against_oracle(torch.float32, 2e-4, True)


@pytest.mark.parametrize("pooled", [True, False])
def test_pack_of_four_bf16_matches_the_oracle(pooled):
    """One pool: the pack kernels.  Private caches (contexts of different pools): the per-prompt launches on each slice."""
    _against_oracle(torch.bfloat16, 0.025, pooled)


def test_pack_bf16_equals_single_continuations_bit_for_bit():
    cfg, engs, xs, pool = _members(torch.bfloat16, LPS, 256)
    nl = cfg.talker.num_hidden_layers
    _prefix(engs, xs, STARTS)
    outs = _pack(engs, xs, STARTS)
    got = [(lg.clone(), hd.clone(), [engs[q].kv_export(i, LPS[q]) for i in range(nl)]) for q, (lg, hd) in enumerate(outs)]
    again = _pack(engs, xs, STARTS)                                         # the same call twice
    for (lg, hd), g in zip(again, got):
        assert torch.equal(lg, g[0]) and torch.equal(hd, g[1])
    # "cont_pack" 0: the per-prompt attention launches on each slice -- the same arithmetic
    for e in engs:
        e.set_option("cont_pack", 0)
    _prefix(engs, xs, STARTS)
    for (lg, hd), g in zip(_pack(engs, xs, STARTS), got):
        assert torch.equal(lg, g[0]) and torch.equal(hd, g[1])
    _prefix(engs, xs, STARTS)
    for q, (e, x, s) in enumerate(zip(engs, xs, STARTS)):
        lg, hd = e.prefill_continue(x[s:].contiguous(), s)
        assert torch.equal(lg, got[q][0]) and torch.equal(hd, got[q][1]), f"member {q} (start {s}): logits / hidden differ from the single call"
        for i in range(nl):
            k, v = e.kv_export(i, LPS[q])
            assert torch.equal(k, got[q][2][i][0]) and torch.equal(v, got[q][2][i][1]), f"member {q} layer {i}: K / V differ from the single call"
    _close(engs, pool)


def test_two_identical_packs_with_key_splits_give_identical_bits():
    lps, starts = (1100, 768, 130), (1000, 704, 0)                          # 18 and 12 key tiles: splits + merge; (0, 130): none
    cfg, engs, xs, pool = _members(torch.bfloat16, lps, 1108)
    _prefix(engs, xs, starts)
    a = [(lg.clone(), hd.clone()) for lg, hd in _pack(engs, xs, starts)]
    ka = engs[0].kv_export(cfg.talker.num_hidden_layers - 1, lps[0])
    b = _pack(engs, xs, starts)
    kb = engs[0].kv_export(cfg.talker.num_hidden_layers - 1, lps[0])
    for (la, ha), (lb, hb) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(ha, hb)
    assert torch.equal(ka[0], kb[0]) and torch.equal(ka[1], kb[1])
    for q, Lp in enumerate(lps):                                             # and within the bf16 bound of the oracle
        lo, ho = _oracle("0p6b", Lp, torch.bfloat16)
        assert float((a[q][1].float().cpu() - ho).abs().max()) <= 0.025 * max(1.0, float(ho.abs().max())), q
        assert float((a[q][0].float().cpu() - lo).abs().max()) <= 0.025 * max(1.0, float(lo.abs().max())), q
    _close(engs, pool)


def test_error_codes_leave_every_block_count_unchanged():
    from fq3hip.engine import Fq3Engine, Fq3KvPool
    cfg, engs, xs, pool = _members(torch.bfloat16, (100, 100, 100), 192, blocks=5)
    lib, st = engs[0].lib, engs[0]._stream()
    H = cfg.talker.hidden_size
    outs = [e.new(H) for e in engs]
    engs[0].prefill(xs[0][:64].contiguous(), want_logits=False)             # member 0 owns one block, the others none
    vp = C.c_void_p

    def call(es, starts, cnts, n=None, embeds=None):
        k = len(es)
        ctxs = (vp * k)(*[e.ctx if e is not None else None for e in es])
        emb = (vp * k)(*(embeds or [xs[0].data_ptr()] * k))
        hd = (vp * k)(*[o.data_ptr() for o in outs[:k]])
        before = [e.kv_blocks() for e in engs]
        rc = lib.fq3_prefill_continue_batch(ctxs, k if n is None else n, emb, (C.c_int * k)(*starts), (C.c_int * k)(*cnts), None, hd, st)
        assert [e.kv_blocks() for e in engs] == before, (rc, starts, cnts)
        return rc

    assert call(engs, [64, 0, 0], [10, 10, 10], n=0) == L.FQ3_EINVAL
    assert call(engs, [64, 0, 0], [10, 10, 10], n=65) == L.FQ3_EINVAL
    assert call(engs, [64, 0, 0], [10, 0, 10]) == L.FQ3_EINVAL              # cnt < 1
    assert call(engs, [64, -1, 0], [10, 10, 10]) == L.FQ3_EINVAL            # start < 0
    assert call([engs[0], engs[1], engs[0]], [64, 0, 64], [10, 10, 10]) == L.FQ3_EINVAL      # a context twice
    assert call(engs, [64, 0, 0], [10, 10, 10], embeds=[xs[0].data_ptr(), None, xs[0].data_ptr()]) == L.FQ3_EINVAL
    W32 = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor"))
    f32 = Fq3Engine(cfg, W32, device="cuda", dtype=torch.float32, max_seq_len=192, max_frames=8)
    assert call([engs[0], f32], [64, 0], [10, 10]) == L.FQ3_EINVAL           # mixed dtypes / weight tables
    assert call(engs, [64, 65, 0], [10, 10, 10]) == L.FQ3_ESTATE            # member 1 owns no block of rows [0, 65)
    assert call(engs, [128, 0, 0], [10, 10, 10]) == L.FQ3_ESTATE            # member 0 owns one block, rows [0, 128) need two
    assert call(engs, [64, 0, 0], [129, 10, 10]) == L.FQ3_ETOOLONG          # start + cnt > max_seq_len
    assert b"Input is too long: prefill has 193 tokens but max_seq_len=192" in lib.fq3_last_error()
    assert call(engs, [0, 0, 0], [70, 70, 70]) == L.FQ3_ETOOLONG            # 210 packed rows on a workspace of 192
    # a short pool: 5 blocks, member 0 holds one; one more + 2 + 2 are needed -> FQ3_ENOMEM with nothing taken (192 packed rows fit)
    assert call(engs, [64, 0, 0], [60, 66, 66]) == L.FQ3_ENOMEM
    assert pool.stats()["free"] == 4
    # and a call that fits goes through
    tail = xs[0][64:].contiguous()
    ctxs = (vp * 2)(engs[0].ctx, engs[1].ctx)
    emb = (vp * 2)(tail.data_ptr(), xs[1].data_ptr())
    hd = (vp * 2)(outs[0].data_ptr(), outs[1].data_ptr())
    assert lib.fq3_prefill_continue_batch(ctxs, 2, emb, (C.c_int * 2)(64, 0), (C.c_int * 2)(36, 64), None, hd, st) == 0
    assert [e.kv_blocks() for e in engs] == [2, 1, 0]
    f32.close()
    _close(engs, pool)
