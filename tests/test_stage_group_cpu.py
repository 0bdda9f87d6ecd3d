"""CPU: the host half of the group form of the output stages: the two symbols and their bindings, the range
checks that are answered before any HIP call (there is no GPU here, so an answer at all shows where they sit), and the validation of
the batch entry points' ``output=`` keyword over a model made of stand-ins."""
import ctypes as C
import inspect
from types import SimpleNamespace

import pytest

from fq3hip import _lib
from fq3hip.audio_out import AudioOutSpec
from fq3hip.model import FasterQwen3TTS

GROUP = ("fq3_audio_out_push_group", "fq3_tsm_push_group")
BATCH = ("generate_voice_clone_batch", "generate_custom_voice_batch", "generate_voice_design_batch",
         "generate_voice_clone_batch_streaming", "generate_custom_voice_batch_streaming", "generate_voice_design_batch_streaming",
         "stream_custom_voice_batch", "stream_voice_design_batch", "stream_voice_clone_batch")


def test_symbols_and_bindings():
    lib = _lib.load()
    for name in GROUP:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 9 and args[1] is C.c_int
    assert _lib.FQ3_STAGE_GROUP_MAX == 32
    lib.fq3_abi_version.restype = C.c_int
    assert lib.fq3_abi_version() == 5                           # additive: the version stays


def test_range_checks_come_before_any_hip_call():
    lib = _lib.load()
    one_p, one_l, one_i = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0), (C.c_int * 1)(0)
    for name in GROUP:
        fn = getattr(lib, name)
        full = [one_p, 1, one_p, one_l, one_i, one_p, one_l, one_l, None]
        for B in (-1, 33, 1 << 20):
            assert fn(*(full[:1] + [B] + full[2:])) == _lib.FQ3_EINVAL, (name, B)
        assert b"32" in lib.fq3_last_error()
        for at in (0, 2, 3, 4, 5, 6, 7):                        # every array
            args = list(full)
            args[at] = None
            assert fn(*args) == _lib.FQ3_EINVAL, (name, at)
        assert fn(*full) == _lib.FQ3_EINVAL                     # a null object in the array
        assert fn(None, 0, None, None, None, None, None, None, None) == 0      # B == 0: nothing to do


class _Graph:
    def capture(self, **kw):
        pass


def _wrapper(kind="custom_voice"):
    inner = SimpleNamespace(speech_tokenizer=SimpleNamespace(sample_rate=24000), tts_model_type=kind, tts_model_size="0b6")
    return FasterQwen3TTS(base_model=SimpleNamespace(model=inner), predictor_graph=_Graph(), talker_graph=_Graph())


def test_every_batch_entry_point_has_the_keyword():
    for name in BATCH:
        p = inspect.signature(getattr(FasterQwen3TTS, name)).parameters
        assert list(p)[-1] == "output" and p["output"].default is None, name
        assert list(p)[-2] == "seeds", name                     # what was there keeps its place


def test_output_list_validation():
    w = _wrapper()
    a, b = AudioOutSpec(8000, "mulaw", 1.25), AudioOutSpec(16000, "s16")
    assert w._batch_outputs(None, 3) is None
    assert w._batch_outputs([None, None, None], 3) is None      # nothing to do: the path without the keyword
    assert w._batch_outputs(a, 3) == [a, a, a]
    assert w._batch_outputs([a, None, b], 3) == [a, None, b] and w._batch_outputs((a, b), 2) == [a, b]
    for bad, n in (([a, b], 3), ([a], 0), ("mulaw", 2), ([a, "s16"], 2), ({"encoding": "s16"}, 1), (8000, 1)):
        with pytest.raises(ValueError):
            w._batch_outputs(bad, n)
    with pytest.raises(ValueError, match="320"):
        w._batch_outputs(AudioOutSpec(24001, "s16"), 1)         # the library's reason: a rate pair it refuses
    # inside audio_output(): the keyword is refused, and without it the context's refusal stands, with its message
    with w.audio_output(16000, "s16"):
        with pytest.raises(ValueError, match="output="):
            w._batch_outputs(a, 1)
        with pytest.raises(ValueError, match="output="):
            w.generate_voice_clone_batch(["a"], language="English", output=a)
        with pytest.raises(ValueError, match="output="):
            next(w.generate_voice_clone_batch_streaming(["a"], language="English", output=a))
        with pytest.raises(ValueError, match="batch entry points"):
            w.generate_voice_clone_batch(["a"], language="English")
    # argument errors of the keyword surface before anything is prepared or decoded
    with pytest.raises(ValueError, match="one value or one per text"):
        w.generate_voice_clone_batch(["a", "b"], language="English", output=[a])
    with pytest.raises(ValueError, match="AudioOutSpec"):
        next(w.generate_voice_clone_batch_streaming(["a"], language="English", output="mulaw"))
    with pytest.raises(ValueError, match="AudioOutSpec"):
        next(w.stream_voice_clone_batch([iter(["a"])], output=[16000]))


class _ScriptedModel:
    """Stand-in for the model under the CLI: notes the batch call and answers with what the output spec promises"""
    sample_rate = 24000

    def __init__(self):
        self.calls = []

    def generate_voice_clone_batch(self, texts, lanes=8, output=None, **kw):
        import numpy as np
        self.calls.append((list(texts), lanes, output))
        if output is None:
            return [([np.full(240 * len(t), 0.25, np.float32)], 24000) for t in texts]
        return [([np.full(80 * len(t), 0x7F, np.uint8)], output.out_rate(24000)) for t in texts]


def test_cli_lock_step_mode_passes_the_output_flags(tmp_path):
    import os
    from fq3hip import cli
    p, m = cli.build_parser(), _ScriptedModel()
    base = ["serve", "--ref-audio", "r.wav", "--ref-text", "t", "--lanes", "3"]
    d = str(tmp_path / "plain")
    cli.cmd_serve(p.parse_args(base + ["--output-dir", d]), model=m, lines=["a\n", "bb\n", "ccc\n", "exit\n"])
    assert m.calls[-1] == (["a", "bb", "ccc"], 3, None)          # without the flags: the call as it was
    d = str(tmp_path / "mulaw")
    cli.cmd_serve(p.parse_args(base + ["--output-dir", d, "--out-rate", "8000", "--encoding", "mulaw", "--speed", "1.25"]), model=m,
                  lines=["a\n", "bb\n", "ccc\n", "exit\n"])
    assert m.calls[-1] == (["a", "bb", "ccc"], 3, AudioOutSpec(8000, "mulaw", 1.25))
    assert sorted(os.listdir(d)) == ["out_0001.wav", "out_0002.wav", "out_0003.wav"]
