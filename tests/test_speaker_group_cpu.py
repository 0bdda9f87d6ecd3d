"""CPU: the host half of ``fq3_refenc_speaker_group`` / ``fq3_refenc_similarity`` and the Python wrappers over stand-ins (DESIGN.md
section 4.25).  The kernels of csrc/spkgroup_kernels.cuh get their lines of the kernel census from here: their reference test is
tests/test_gpu_speaker_group.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_kernel_census_cpu as census
from fq3hip import _lib, speaker_check
from fq3hip.config import tiny_ref_audio_config
from fq3hip.refenc import HipRefAudioAnalyzer, ref_config_struct

census.COVERAGE.update({k: ("test_gpu_speaker_group.py", "test_gpu_speaker_group.py", "spkgroup_kernels.cuh")
                        for k in ("spk_frag_pack_kernel", "spk_logmel_group_kernel", "spk_pad_group_kernel", "spk_stats_group_kernel",
                                  "spk_rowvec_group_kernel", "spk_cosine_kernel")})


def test_symbol_binding_and_range_checks():
    lib = _lib.load()
    h = _lib.vp()
    cc = ref_config_struct(tiny_ref_audio_config())
    assert lib.fq3_refenc_create(C.byref(cc), C.byref(h)) == 0               # host only: no device call before finalize
    lens = lambda *v: (C.c_int64 * len(v))(*v)
    ws = lib.fq3_refenc_speaker_group_workspace
    assert ws(h, lens(97, 2048, 5000), 3) > ws(h, lens(97, 2048), 2) > 0
    for rows, n, named in ((0, lens(2048), b"rows"), (33, lens(*[2048] * 33), b"rows"), (3, lens(2048, 2048, 96), b"row 2"), (2, lens(1 << 27, 2048), b"row 0")):
        assert ws(h, n, rows) == _lib.FQ3_EINVAL and named in lib.fq3_last_error(), rows
    assert ws(None, lens(2048), 1) == _lib.FQ3_EINVAL and ws(h, None, 1) == _lib.FQ3_EINVAL
    one = (_lib.vp * 1)(None)
    assert lib.fq3_refenc_speaker_group(None, one, lens(2048), 1, None, None) == _lib.FQ3_EINVAL
    assert lib.fq3_refenc_speaker_group(h, one, lens(2048), 1, one, None) == _lib.FQ3_ESTATE      # nothing bound, nothing finalized
    for a, b, rows, dim, out in ((None, one, 1, 4, one), (one, None, 1, 4, one), (one, one, 1, 4, None), (one, one, 0, 4, one), (one, one, 1, 0, one)):
        assert lib.fq3_refenc_similarity(a, b, rows, dim, out, None) == _lib.FQ3_EINVAL
    assert lib.fq3_refenc_destroy(h) == 0


class _Analyzer(HipRefAudioAnalyzer):
    """The wrapper's slicing over a library that only records: (rows, lengths, offset of the output in rows)."""

    def __init__(self):
        self.cfg, self.device, self.calls = tiny_ref_audio_config(), torch.device("cpu"), []

    def _group_call(self, ptrs, lens, rows, out_ptr):
        self.calls.append((rows, list(lens), out_ptr))


def test_more_than_32_clips_go_in_slices_of_32():
    an = _Analyzer()
    clips = [np.zeros(100 + i, np.float32) for i in range(70)]
    out = an.speaker_embeddings(clips)
    assert out.shape == (70, an.cfg.enc_dim) and [c[0] for c in an.calls] == [32, 32, 6]
    assert [n for c in an.calls for n in c[1]] == [100 + i for i in range(70)]
    row = an.cfg.enc_dim * 4
    assert [c[2] - out.data_ptr() for c in an.calls] == [0, 32 * row, 64 * row]
    an.calls.clear()
    assert an.speaker_embeddings([]).shape == (0, an.cfg.enc_dim) and not an.calls
    with pytest.raises(ValueError):
        HipRefAudioAnalyzer.similarity(an, torch.zeros(3, 8), torch.zeros(2, 8))
    with pytest.raises(ValueError):
        HipRefAudioAnalyzer.similarity(an, torch.zeros(3, 8), torch.zeros(3, 4))


def _stand_in():
    """An analyser whose embedding of a clip is (its length, 1) and whose cosine is torch's; it records what it was asked for."""
    asked = []

    def embeddings(clips):
        asked.append([len(c) for c in clips])
        return torch.tensor([[float(len(c)), 1.0] for c in clips])
    an = SimpleNamespace(device=torch.device("cpu"), speaker_embeddings=embeddings,
                         similarity=lambda e, r: torch.nn.functional.cosine_similarity(e, r.reshape(1, -1).float().expand_as(e), dim=1))
    return an, asked


@pytest.mark.parametrize("form", ["prompt", "items", "item", "tensor", "array"])
def test_a_stored_embedding_is_used_as_it_is(form):
    an, asked = _stand_in()
    emb = torch.tensor([3.0, 1.0])
    ref = dict(prompt=dict(ref_code=[None], ref_spk_embedding=[emb]), items=[SimpleNamespace(ref_spk_embedding=emb)],
               item=SimpleNamespace(ref_spk_embedding=emb), tensor=emb, array=emb.numpy())[form]
    refuse = lambda r: pytest.fail("a stored embedding must not be recomputed")
    got = speaker_check.speaker_similarity(an, [np.zeros(3, np.float32), np.zeros(40, np.float32)], 24000, ref, refuse)
    assert asked == [[3, 40]] and got[0] == pytest.approx(1.0) and 0 < got[1] < 1
    assert speaker_check.speaker_similarity(an, np.zeros(3, np.float32), 24000, ref, refuse) == pytest.approx(1.0)      # one clip: a float


@pytest.mark.parametrize("ref", ["voice.wav", (np.zeros(7, np.float32), 16000)])
def test_a_reference_clip_rides_in_the_group_call(ref):
    an, asked = _stand_in()
    seen = []
    got = speaker_check.speaker_similarity(an, [np.zeros(5, np.float32)], [24000], ref, lambda r: seen.append(r) or np.zeros(5, np.float32))
    assert seen == [ref] and asked == [[5, 5]] and got == [pytest.approx(1.0)]


def test_argument_errors():
    an, _asked = _stand_in()
    x = np.zeros(5, np.float32)
    for audio, sr, ref in (([x, x], [24000], torch.ones(2)), ([x], 24000, torch.ones(3)), ([x], 24000, torch.ones(2, 2)), ([x], 24000, dict(ref_code=[None]))):
        with pytest.raises(ValueError):
            speaker_check.speaker_similarity(an, audio, sr, ref, None)
    assert speaker_check.speaker_similarity(an, [], 24000, torch.ones(2), None) == []
    from fq3hip.model import FasterQwen3TTS
    with pytest.raises(NotImplementedError, match="speaker_encoder"):
        FasterQwen3TTS.speaker_similarity(SimpleNamespace(model=SimpleNamespace(ref_analyzer=None)), x, 24000, torch.ones(2))


def test_cli_verify_prints_one_cosine_per_file(tmp_path, monkeypatch, capsys):
    from fq3hip import cli
    from fq3hip.audio_io import write_wav
    paths = []
    for i, n in enumerate((2400, 4800)):
        paths.append(str(tmp_path / f"{i}.wav"))
        write_wav(paths[-1], np.zeros(n, np.float32), 16000)
    calls = []
    model = SimpleNamespace(speaker_similarity=lambda audio, sr, ref: calls.append(([len(a) for a in audio], sr, ref)) or [0.25, -0.5])
    monkeypatch.setattr(cli, "load_model", lambda args: model)
    cli.main(["verify", "--ref", "ref.wav"] + paths)
    assert calls == [([2400, 4800], [16000, 16000], "ref.wav")]
    assert capsys.readouterr().out.splitlines() == [f"{paths[0]}: 0.250000", f"{paths[1]}: -0.500000"]


def test_verify_none_leaves_the_batch_call_as_it_was(monkeypatch):
    import inspect
    from fq3hip.model import FasterQwen3TTS
    from test_stage_group_cpu import _wrapper
    w, seen = _wrapper(), []
    monkeypatch.setattr(w, "_run_batch_full", lambda *a, **kw: seen.append(kw) or [])
    monkeypatch.setattr(w, "_prepare_custom_batch", lambda *a: iter(()))
    monkeypatch.setattr(w, "_prepare_design_batch", lambda *a: iter(()))
    monkeypatch.setattr(w, "_prepare_clone_batch", lambda *a: iter(()))
    for name in ("generate_voice_clone_batch", "generate_custom_voice_batch", "generate_voice_design_batch"):
        assert inspect.signature(getattr(FasterQwen3TTS, name)).parameters["verify"].default is None
    w.generate_custom_voice_batch(["a", "b"], "s")
    w.generate_custom_voice_batch(["a", "b"], "s", verify=None)
    assert seen[0] == seen[1] and "verify" not in seen[0]                  # the keywords _run_batch_full always got, nothing more
    with pytest.raises(ValueError, match="verify"):
        w.generate_custom_voice_batch(["a"], "s", verify=0.7)              # no threshold is taken
    with pytest.raises(NotImplementedError, match="speaker_encoder"):
        w.generate_custom_voice_batch(["a"], "s", verify=True)
    w.model.ref_analyzer = SimpleNamespace(has_speaker=True)
    w.generate_custom_voice_batch(["a", "b"], "s", verify=True)
    w.generate_voice_design_batch(["a"], "a calm voice", verify=True)
    assert seen[-2]["verify"] == [None, None] and seen[-1]["verify"] == [None]      # no speaker embedding in the prompt: no score
    emb = torch.ones(4)
    monkeypatch.setattr(w, "_resolve_voice_clone_prompt", lambda **kw: (dict(ref_spk_embedding=[emb]), [None], False))
    w.generate_voice_clone_batch(["a", "b", "c"], ref_audio="voice.wav", xvec_only=True, verify=True)
    assert len(seen[-1]["verify"]) == 3 and all(e is emb for e in seen[-1]["verify"])


def test_a_vocoder_group_is_scored_in_one_call():
    from fq3hip.model import _SideVocoder
    voc, calls = _SideVocoder(SimpleNamespace(sample_rate=24000), "cpu"), []
    emb = torch.ones(4)
    voc.verify = {0: emb, 1: None, 2: emb, 3: 2 * emb}

    def score_rows(refs, rows):
        calls.append(([float(r[0]) for r in refs], [int(x.numel()) for x in rows]))
        return torch.tensor([0.5, 0.25])
    voc.score_rows = score_rows
    voc._scored([0, 1, 2, 3], [torch.zeros(2000), torch.zeros(3000), torch.zeros(10), torch.zeros(1, 4000)])
    assert calls == [([1.0, 2.0], [2000, 4000])]                           # the rows with an embedding and a window's worth of samples
    assert [voc.score(k) for k in range(5)] == [0.5, None, None, 0.25, None]
