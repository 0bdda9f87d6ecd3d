"""GPU: the speaker encoder's group form and the cosine (csrc/spkgroup_kernels.cuh: spk_logmel_group_kernel, spk_pad_group_kernel,
spk_stats_group_kernel, spk_rowvec_group_kernel, spk_frag_pack_kernel, spk_cosine_kernel) against the float64 evaluation of the
oracle's encoder (oracle/refenc_oracle.speaker_embedding with dtype=torch.float64), and against themselves for independence.

Small configuration (hop 64, n_fft 256: a clip of n samples has n // 64 frames; the front end's tile is 32 frames) and the seeded
weights of tests/test_gpu_refenc.py.  The bound of the float64 test is measured, not chosen: 4 x the largest error of the single-clip
fq3_refenc_speaker against the same reference on the same clips.  The shortest clip (98 samples, one above what the single call
accepts: one frame, the front end's reflection covers nearly the whole clip) is beyond the oracle -- torch refuses to reflect-pad one
frame by the TDNN's 2 -- so its float64 reference is tests/_spk_ref.py, the oracle's encoder with the library's padding rule written
out (equal to the oracle's on every other clip: checked in the fixture)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd"))

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_ref_audio_config                             # noqa: E402
from fq3hip.weights import synth_ref_audio_weights                          # noqa: E402
from tests import _spk_ref                                                  # noqa: E402
from tests.test_refenc_oracle_pins import make_wave                         # noqa: E402

# odd frame count (45 frames + 37 samples), exactly one tile, one tile + one frame, the shortest clip, the shortest with a float64
# reference (4 frames + 1 sample), then lengths that are multiples of nothing: 32 clips, two workgroups of the front end for three
LENGTHS = [2917, 2048, 2112, 98, 257] + [300 + 97 * i for i in range(27)]


@pytest.fixture(scope="module")
def env():
    from fq3hip.refenc import HipRefAudioAnalyzer
    from oracle import refenc_oracle as RO
    rc = tiny_ref_audio_config()
    W = synth_ref_audio_weights(rc, 2)
    an = HipRefAudioAnalyzer(rc, W)
    clips = [make_wave(n, seed=1000 + i) for i, n in enumerate(LENGTHS)]
    ref = [RO.speaker_embedding(W, rc, x, torch.float64)[0] if n >= 256 else _spk_ref.speaker_embedding(W, rc, x) for x, n in zip(clips, LENGTHS)]
    assert torch.equal(_spk_ref.speaker_embedding(W, rc, clips[4]), ref[4]) and torch.equal(_spk_ref.speaker_embedding(W, rc, clips[0]), ref[0])
    single = [an.speaker_embedding(x).cpu() for x in clips]
    return an, clips, ref, single


def _err(got, ref):
    return float((got.double() - ref).abs().max())


@pytest.mark.parametrize("rows", [1, 3, 32])
def test_group_against_float64(env, rows):
    an, clips, ref, single = env
    got = an.speaker_embeddings(clips[:rows]).cpu()
    assert got.shape == (rows, an.cfg.enc_dim)
    e_single = max(_err(single[i], ref[i]) for i in range(rows))
    e_group = max(_err(got[i], ref[i]) for i in range(rows))
    print(f"rows {rows}: single path max |err| {e_single:.3e}, bound {4 * e_single:.3e}, group max |err| {e_group:.3e}, "
          f"rows bit-identical to the single call: {sum(bool(torch.equal(got[i], single[i])) for i in range(rows))}/{rows}")
    assert e_group <= 4 * e_single


def test_real_shapes_against_float64():
    """128 mel bins, n_fft 1024, hop 256, 512 / 1536 channels: the front end's tile takes 104 KB of dynamic LDS (the raised limit),
    34 bin blocks over 8 waves; 131 frames = four tiles and three frames beside a clip of less than one tile."""
    from fq3hip.config import RefAudioConfig
    from fq3hip.refenc import HipRefAudioAnalyzer
    from oracle import refenc_oracle as RO
    rc = RefAudioConfig()
    W = {k: v for k, v in synth_ref_audio_weights(rc, 2).items() if k.startswith("speaker_encoder.")}
    an = HipRefAudioAnalyzer(rc, W)
    clips = [make_wave(n, seed=n) for n in (131 * 256 + 77, 5000)]
    ref = [RO.speaker_embedding(W, rc, x, torch.float64)[0] for x in clips]
    single = [an.speaker_embedding(x).cpu() for x in clips]
    got = an.speaker_embeddings(clips).cpu()
    e_single, e_group = max(_err(s, r) for s, r in zip(single, ref)), max(_err(g, r) for g, r in zip(got, ref))
    print(f"real shapes: single path max |err| {e_single:.3e}, bound {4 * e_single:.3e}, group max |err| {e_group:.3e}")
    assert e_group <= 4 * e_single
    assert torch.equal(an.speaker_embeddings(clips[::-1]).cpu(), got.flip(0))


@pytest.mark.parametrize("c", [0, 2, 3, 4])
def test_a_clip_does_not_depend_on_its_neighbours(env, c):
    an, clips, _ref, _single = env
    alone = an.speaker_embeddings([clips[c]])[0]
    others = [x for i, x in enumerate(clips) if i != c]
    of3 = an.speaker_embeddings([others[5], clips[c], others[1]])[1]
    of32 = an.speaker_embeddings(others[::-1] + [clips[c]])[31]
    assert torch.equal(alone, of3) and torch.equal(alone, of32)
    assert torch.equal(an.speaker_embeddings(clips[:3] + [clips[c]])[3], alone)       # a second call on the same workspace


def test_more_than_32_clips_go_in_slices(env):
    an, clips, _ref, _single = env
    got = an.speaker_embeddings(clips + clips[:2])
    assert got.shape[0] == 34 and torch.equal(got[:32], an.speaker_embeddings(clips)) and torch.equal(got[32:], got[:2])


def test_cosine_against_float64(env):
    an, _clips, ref, _single = env
    e = torch.stack(ref).float()
    a, b = e, e.roll(1, 0)
    cos64 = lambda u, v: (u.double() * v.double()).sum(1) / (u.double().norm(dim=1) * v.double().norm(dim=1))
    want = cos64(a, b)
    got = an.similarity(a, b).cpu()
    print(f"cosine: max |err| {float((got.double() - want).abs().max()):.3e}")
    assert (got.double() - want).abs().max() <= 1e-6
    assert (an.similarity(a, a).cpu().double() - 1.0).abs().max() <= 1e-6
    wide = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (5, 2048)).astype(np.float32))      # dim = 2048: 32 terms per lane
    want = cos64(wide, wide.roll(2, 0))
    assert (an.similarity(wide, wide.roll(2, 0)).cpu().double() - want).abs().max() <= 1e-6
    z = torch.zeros_like(a)
    for x, y in ((z, a), (a, z), (z, z)):
        assert torch.equal(an.similarity(x, y).cpu(), torch.zeros(a.shape[0]))
    assert torch.equal(an.similarity(a[0], a).cpu(), an.similarity(a[:1].expand_as(a), a).cpu())       # one vector against many


@pytest.mark.parametrize("case, rows, row_named", [("none", 0, "rows"), ("too_many", 33, "rows"), ("null_row", 3, "row 1"), ("short_row", 3, "row 2")])
def test_errors_are_all_or_nothing(env, case, rows, row_named):
    from fq3hip import _lib as L
    an, clips, _ref, _single = env
    xs = [an._wave(clips[i % 3]) for i in range(max(rows, 1))]
    ptrs = (L.vp * len(xs))(*[x.data_ptr() for x in xs])
    lens = (C.c_int64 * len(xs))(*[x.numel() for x in xs])
    if case == "null_row":
        ptrs[1] = None
    if case == "short_row":
        lens[2] = 96                                                        # the single call takes 97 and more
    out = torch.full((max(rows, 1), an.cfg.enc_dim), 7.0, device=an.device)
    rc = an.lib.fq3_refenc_speaker_group(an.h, ptrs, lens, rows, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    msg = an.lib.fq3_last_error().decode()
    torch.cuda.synchronize()
    assert rc == L.FQ3_EINVAL and row_named in msg, (rc, msg)
    assert bool((out == 7.0).all())
    ws = an.lib.fq3_refenc_speaker_group_workspace(an.h, lens, rows)                    # the size query sees lengths only
    assert ws > 0 if case == "null_row" else ws == L.FQ3_EINVAL


def test_batch_verify_scores_every_utterance_on_the_device():
    """``verify=True`` on the lock-step batch: the same waveforms as without it, and per utterance the cosine that
    ``speaker_similarity`` gives for that waveform and the prompt's embedding (the vocoder groups differ; a clip's bits do not)."""
    import dataclasses
    from fq3hip.config import tiny_test_config
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = tiny_test_config()
    cfg.ref_audio = dataclasses.replace(tiny_ref_audio_config(), enc_dim=cfg.talker.hidden_size)
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "codec", "text"))
    W.update({k: v for k, v in synth_ref_audio_weights(cfg.ref_audio, 2).items() if k.startswith("speaker_encoder.")})
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, codec_max_frames=128, max_frames=64)
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    vcp = dict(ref_spk_embedding=[torch.randn(cfg.talker.hidden_size, generator=torch.Generator().manual_seed(4))])
    texts = ["One.", "A second, longer line to speak.", "Three words here.", "Four.", "The fifth and last line of this batch."]
    kw = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, min_new_tokens=0, max_new_tokens=20)
    plain = m.generate_voice_clone_batch(texts, language="English", voice_clone_prompt=vcp, lanes=3, **kw)
    scored = m.generate_voice_clone_batch(texts, language="English", voice_clone_prompt=vcp, lanes=3, verify=True, **kw)
    assert all(len(r) == 2 for r in plain) and all(len(r) == 3 for r in scored)
    for (wa, sra), (wb, srb, cos) in zip(plain, scored):
        assert sra == srb and np.array_equal(wa[0], wb[0])
        want = m.speaker_similarity(wb[0], srb, vcp)
        print(f"verify: {len(wb[0])} samples, cosine {cos:.6f}, speaker_similarity {want:.6f}")
        assert -1.0 <= cos <= 1.0 and abs(cos - want) <= 1e-6
