"""CPU: the host half of ``fq3_refenc_encode_group`` and the Python wrappers over stand-ins.  The kernels of
csrc/tokgroup_kernels.cuh get their lines of the kernel census from here: their reference test is tests/test_gpu_tokenizer_group.py."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_kernel_census_cpu as census
from fq3hip import _lib
from fq3hip.config import tiny_ref_audio_config
from fq3hip.refenc import HipRefAudioAnalyzer, ref_config_struct

census.COVERAGE.update({k: ("test_gpu_tokenizer_group.py", "test_gpu_tokenizer_group.py", "tokgroup_kernels.cuh")
                        for k in ("tok_conv_in_group_kernel", "tok_clear_kernel", "tok_rope_group_kernel", "tok_attn_group_kernel",
                                  "tok_pad_group_kernel", "tok_rvq_group_kernel")})

lens = lambda *v: (C.c_int64 * len(v))(*v)
RC = dataclasses.replace(tiny_ref_audio_config(), max_positions=1 << 18)     # 2^18 rows of 24 samples: one clip may approach the cap of 65535 * 64


@pytest.fixture()
def handle():
    lib, h = _lib.load(), _lib.vp()
    cc = ref_config_struct(RC)
    assert lib.fq3_refenc_create(C.byref(cc), C.byref(h)) == 0               # host only: no device call before finalize
    yield lib, h
    assert lib.fq3_refenc_destroy(h) == 0


def test_symbol_binding_and_range_checks(handle):
    lib, h = handle
    ws = lib.fq3_refenc_encode_group_workspace
    assert ws(h, lens(97, 1920, 5000), 3) > ws(h, lens(97, 1920), 2) > ws(h, lens(97), 1) > 0
    for rows, n, code, named in ((0, lens(1920), _lib.FQ3_EINVAL, b"rows"), (33, lens(*[1920] * 33), _lib.FQ3_EINVAL, b"rows"),
                                 (3, lens(1920, 1920, 0), _lib.FQ3_EINVAL, b"row 2"), (2, lens((1 << 26) + 1, 1920), _lib.FQ3_EINVAL, b"row 0"),
                                 (2, lens(1920, (24 << 18) + 1), _lib.FQ3_ETOOLONG, b"row 1"),                 # one row more than the position table has
                                 (3, lens(*[3 << 19] * 3), _lib.FQ3_ETOOLONG, b"row 2")):                    # the third clip passes the cap on packed samples
        assert ws(h, n, rows) == code and named in lib.fq3_last_error(), (rows, lib.fq3_last_error())
    assert ws(None, lens(1920), 1) == _lib.FQ3_EINVAL and ws(h, None, 1) == _lib.FQ3_EINVAL
    one = (_lib.vp * 1)(None)
    for r, pcm, n, codes in ((None, one, lens(1920), one), (h, None, lens(1920), one), (h, one, None, one), (h, one, lens(1920), None)):
        assert lib.fq3_refenc_encode_group(r, pcm, n, 1, codes, None) == _lib.FQ3_EINVAL
    assert lib.fq3_refenc_encode_group(h, one, lens(1920), 1, one, None) == _lib.FQ3_ESTATE      # nothing bound, nothing finalized


class _Analyzer(HipRefAudioAnalyzer):
    """The wrapper's slicing over a library that only records; the handle is a real one, so frame counts and the cap are the library's."""

    def __init__(self, lib, h):
        self.cfg, self.device, self.lib, self.h, self.calls = RC, torch.device("cpu"), lib, h, []

    def __del__(self):
        pass

    def _encode_group_call(self, ptrs, lens, rows, dst):
        self.calls.append((rows, list(lens), list(dst)))


def test_slices_end_at_32_rows_or_at_the_cap(handle):
    an = _Analyzer(*handle)
    clips = [np.zeros(100 + i, np.float32) for i in range(70)]
    out = an.encode_many(clips)
    assert [c[0] for c in an.calls] == [32, 32, 6] and [n for c in an.calls for n in c[1]] == [100 + i for i in range(70)]
    assert [p for c in an.calls for p in c[2]] == [o.data_ptr() for o in out]
    assert [tuple(o.shape) for o in out] == [(an.num_frames(100 + i), an.cfg.num_quantizers) for i in range(70)]
    an.calls.clear()
    an._wave = lambda c: SimpleNamespace(numel=lambda: c, data_ptr=lambda: 64)         # lengths only: nothing this long is allocated
    an.num_frames = lambda n: 1
    an.encode_many([3 << 19, 3 << 19, 3 << 19, 1000, 3 << 19])                           # two clips of 1.5 Mi samples fit under the cap, three do not
    assert [c[1] for c in an.calls] == [[3 << 19, 3 << 19], [3 << 19, 1000, 3 << 19]]
    an.calls.clear()
    assert an.encode_many([]) == [] and not an.calls
    with pytest.raises(ValueError, match="empty"):
        an.encode_many([1000, 0])


def _model(has_encoder=True):
    """A native model whose analyser records what it is asked for: a clip's embedding is (its length,), its codes are its length."""
    from fq3hip.native_model import NativeQwen3TTS
    asked = []
    an = SimpleNamespace(has_speaker=True, has_encoder=has_encoder,
                         speaker_embeddings=lambda ws: asked.append(("spk", [len(w) for w in ws])) or torch.tensor([[float(len(w))] for w in ws]),
                         encode_many=lambda ws: asked.append(("enc", [len(w) for w in ws])) or [torch.tensor([[len(w)]]) for w in ws])
    m = SimpleNamespace(ref_analyzer=an, dtype=torch.float32, _reference_wave=lambda a: np.asarray(a, np.float32))
    return (lambda *a, **kw: NativeQwen3TTS.create_voice_clone_prompts(m, *a, **kw)), asked


def test_prompts_of_many_clips_come_from_two_group_calls():
    make, asked = _model()
    clips = [np.zeros(n, np.float32) for n in (10, 20, 30, 40)]
    items = make(clips, ["a", "b", "", "d"], [False, False, True, False])
    assert asked == [("spk", [10, 20, 30, 40]), ("enc", [10, 20, 40])]                  # the x-vector-only clip is left out of the encode group
    assert [None if it.ref_code is None else int(it.ref_code) for it in items] == [10, 20, None, 40]
    assert [float(it.ref_spk_embedding) for it in items] == [10.0, 20.0, 30.0, 40.0]
    assert [(it.ref_text, it.icl_mode, it.x_vector_only_mode) for it in items] == [("a", True, False), ("b", True, False), (None, False, True), ("d", True, False)]
    asked.clear()
    assert all(it.ref_code is None for it in make(clips, x_vector_only_mode=True)) and asked == [("spk", [10, 20, 30, 40])]
    assert [it.ref_text for it in make(clips[:2], "same")] == ["same", "same"]          # one value for all clips
    for args in ((clips, ["a", "b"]), (clips[:2], ["a", ""]), ([clips[0], None], "a"), (clips[:2], "a", [True])):
        with pytest.raises(ValueError):
            make(*args)
    with pytest.raises(NotImplementedError, match="encoder"):
        _model(has_encoder=False)[0](clips, "a")


def test_cli_enroll_writes_one_cache_entry_per_clip(tmp_path, monkeypatch, capsys):
    from fq3hip import cli
    from fq3hip.native_model import VoiceClonePromptItem
    from fq3hip.voice_cache import VoiceRefCache, cache_key
    audio = [np.full(n, 0.25, np.float32) for n in (100, 200)]
    calls = []

    def prompts(waves, texts, x_vector_only_mode):
        calls.append(([len(w) for w in waves], texts, x_vector_only_mode))
        return [VoiceClonePromptItem(torch.full((3, 16), i), torch.ones(4) * i, False, True, t) for i, t in enumerate(texts)]
    entry = lambda p, xvec, sil: (audio[int(p[0])], *cache_key(audio[int(p[0])], append_silence=True, model_identity="m", mode="icl"), True, "m")
    monkeypatch.setattr(cli, "load_model", lambda args: SimpleNamespace(create_voice_clone_prompts=prompts, _voice_cache_entry=entry))
    (tmp_path / "t.txt").write_text("first\nsecond\n")
    cli.main(["enroll", "--out", str(tmp_path / "v"), "--ref-text-file", str(tmp_path / "t.txt"), "0.wav", "1.wav"])
    assert calls == [([100, 200], ["first", "second"], False)]
    cache = VoiceRefCache(tmp_path / "v")
    for i, line in enumerate(capsys.readouterr().out.splitlines()):
        key, meta = cache_key(audio[i], append_silence=True, model_identity="m", mode="icl")
        hit = cache.load(key, meta)
        assert line == f"{i}.wav: {key}" and hit["ref_text"] == ("first", "second")[i] and (hit["ref_code"] == i).all() and hit["ref_code"].shape == (3, 16)
    with pytest.raises(SystemExit):
        cli.main(["enroll", "--out", str(tmp_path / "v"), "--ref-text-file", str(tmp_path / "t.txt"), "0.wav"])
