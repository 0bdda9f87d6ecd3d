"""GPU: the speech-tokenizer encoder's group form (csrc/tokgroup_kernels.cuh: tok_conv_in_group_kernel, tok_clear_kernel,
tok_rope_group_kernel, tok_attn_group_kernel, tok_pad_group_kernel, tok_rvq_group_kernel) against the single call, bit for bit, and
against the oracle (oracle/refenc_oracle.tokenizer_encode) under the near-tie rule of tests/test_gpu_refenc.py.

Tiny configuration: ratios (2, 3, 4), so a 25 Hz row is 24 samples, a frame 48, and 48 is also the row space's alignment unit.  The
lengths are the ones the single call's test found sharp (whole frames, one sample more, an odd tail, less than a frame's worth of
rows at some stage, many tiles of the front stage), one sample, and a short multiple of 48.  Clips and seeds of the oracle test are
those of tests/test_gpu_refenc.py (the oracle has no second summation order for the encoder to choose seeds by)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd"))

pytestmark = pytest.mark.gpu

from fq3hip.config import RefAudioConfig, tiny_ref_audio_config            # noqa: E402
from fq3hip.weights import synth_ref_audio_weights                          # noqa: E402
from tests.test_gpu_refenc import _compare_codes                            # noqa: E402
from tests.test_refenc_oracle_pins import make_wave                         # noqa: E402

LENGTHS = [48 * 40, 48 * 40 + 1, 48 * 13 + 29, 97, 5000, 1, 48 * 7]


@pytest.fixture(scope="module")
def env():
    from fq3hip.refenc import HipRefAudioAnalyzer
    rc = tiny_ref_audio_config()
    W = synth_ref_audio_weights(rc, 0)
    an = HipRefAudioAnalyzer(rc, W)
    clips = [make_wave(LENGTHS[i % 7], seed=LENGTHS[i % 7] + 1000 * (i // 7)) for i in range(32)]
    single = [an.encode(x) for x in clips]
    return rc, W, an, clips, single


@pytest.mark.parametrize("rows", [1, 3, 32])
def test_group_equals_single_bit_for_bit(env, rows):
    _rc, _W, an, clips, single = env
    got = an.encode_many(clips[:rows])
    assert [g.shape[0] for g in got] == [an.num_frames(x.numel()) for x in clips[:rows]]
    differ = [b for b in range(rows) if not torch.equal(got[b], single[b])]
    assert not differ, f"rows whose codes differ from their single call: {differ}"
    again = an.encode_many(clips[:rows])                                    # the same workspace
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_group_against_the_oracle(env):
    from oracle import refenc_oracle as RO
    rc, W, an, clips, _single = env
    for x, got in zip(clips[:3], an.encode_many(clips[:3])):
        ref, margins = RO.tokenizer_encode(W, rc, x, return_all=True)[:2]
        n_cmp, n_div = _compare_codes(rc, got.cpu(), ref, margins)
        print(f"{x.numel()} samples: {n_cmp} decisions compared, {n_div} chains diverged at near-ties")
        assert n_div <= max(1, ref.shape[0] // 10), (n_cmp, n_div)


@pytest.mark.parametrize("pos", [0, 2, 4])
def test_a_clip_does_not_depend_on_its_neighbours_or_its_place(env, pos):
    _rc, _W, an, clips, single = env
    for c in (2, 4, 5):                                                     # an odd tail, many tiles, one sample
        for others in ([x for i, x in enumerate(clips[:7]) if i != c][:4], clips[12:24][::-1][:4]):
            group = others[:pos] + [clips[c]] + others[pos:]
            assert torch.equal(an.encode_many(group)[pos], single[c]), (c, pos)


def test_real_shapes():
    """Mimi-default shapes: 0.5 s, 3.1 s (39 frames, more than 64 keys per query: two passes of the attention) and 1 s + 7 samples."""
    from fq3hip.refenc import HipRefAudioAnalyzer
    from oracle import refenc_oracle as RO
    rc = RefAudioConfig()
    W = {k: v for k, v in synth_ref_audio_weights(rc, 1).items() if k.startswith("encoder.")}
    an = HipRefAudioAnalyzer(rc, W)
    clips = [make_wave(12000, seed=3), make_wave(24000 * 3 + 2500, seed=7), make_wave(24007, seed=5)]
    got = an.encode_many(clips)
    for x, g in zip(clips, got):
        assert torch.equal(g, an.encode(x)), x.numel()
    ref, margins = RO.tokenizer_encode(W, rc, clips[1], return_all=True)[:2]
    assert got[1].shape == ref.shape == (39, 16)
    _n_cmp, n_div = _compare_codes(rc, got[1].cpu(), ref, margins)
    exact = int((got[1].cpu() == ref).sum())
    print(f"real-shape encoder group: {exact}/{ref.numel()} ids identical, {n_div} chains diverged at near-ties")
    assert n_div <= 2 and exact >= ref.numel() - 40


@pytest.mark.parametrize("case, rows, code, named", [("none", 0, "EINVAL", "rows"), ("too_many", 33, "EINVAL", "rows"), ("null_row", 3, "EINVAL", "row 1"),
                                                     ("empty_row", 3, "EINVAL", "row 2"), ("long_row", 3, "ETOOLONG", "row 1")])
def test_errors_are_all_or_nothing(env, case, rows, code, named):
    from fq3hip import _lib as L
    rc, _W, an, clips, _single = env
    xs = [an._wave(clips[i % 3]) for i in range(max(rows, 1))]
    if case == "long_row":
        xs[1] = torch.zeros(rc.max_positions * 24 + 1, device=an.device)    # one 25 Hz row more than the position table has
    ptrs = (L.vp * len(xs))(*[x.data_ptr() for x in xs])
    lens = (C.c_int64 * len(xs))(*[x.numel() for x in xs])
    if case == "null_row":
        ptrs[1] = None
    if case == "empty_row":
        lens[2] = 0
    out = [torch.full((max(an.num_frames(x.numel()), 1), rc.num_quantizers), -7, dtype=torch.long, device=an.device) for x in xs]
    dst = (L.vp * len(xs))(*[o.data_ptr() for o in out])
    ret = an.lib.fq3_refenc_encode_group(an.h, ptrs, lens, rows, dst, torch.cuda.current_stream().cuda_stream)
    msg = an.lib.fq3_last_error().decode()
    torch.cuda.synchronize()
    assert ret == getattr(L, "FQ3_" + code) and named in msg, (ret, msg)
    assert all(bool((o == -7).all()) for o in out)


def test_public_methods():
    """``create_voice_clone_prompts`` over four clips, one of them x-vector only, and a list through the tokenizer's ``encode``."""
    from fq3hip.config import tiny_test_config
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = tiny_test_config()
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "codec", "text"))
    W.update(synth_ref_audio_weights(cfg.ref_audio, 4))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, codec_max_frames=128, max_frames=64)
    clips = [make_wave(n, seed=n).numpy() for n in (48 * 30, 2917, 48 * 13 + 29, 5000)]
    texts, xvec = ["one", "two", "", "four"], [False, False, True, False]
    items = m.create_voice_clone_prompts([(x, 24000) for x in clips], texts, xvec)
    assert len(items) == 4 and items[2].ref_code is None and items[2].x_vector_only_mode and not items[2].icl_mode
    spk = m.model.ref_analyzer.speaker_embeddings(clips)                    # the speaker group's: a clip's bits do not depend on its place
    for i, (x, t, xv, it) in enumerate(zip(clips, texts, xvec, items)):
        one = m.model.create_voice_clone_prompt(ref_audio=(x, 24000), ref_text=t, x_vector_only_mode=xv)[0]
        assert (it.ref_text, it.icl_mode) == (one.ref_text, one.icl_mode)
        assert it.ref_code is None if xv else torch.equal(it.ref_code, one.ref_code)
        assert torch.equal(it.ref_spk_embedding, spk[i].to(it.ref_spk_embedding.dtype))
    tok = m.model.model.speech_tokenizer
    many = tok.encode(clips[:3], sr=24000).audio_codes
    assert all(torch.equal(g, tok.encode(x, sr=24000).audio_codes[0]) for g, x in zip(many, clips))
