"""CPU: the host half of ``fq3_mark_push_group`` and the batch entry points' ``watermark=`` over a model made of stand-ins (as
tests/test_stage_group_cpu.py does for ``output=``).  mark_embed_group_kernel gets its line of the kernel census from here."""
import ctypes as C
from types import SimpleNamespace

import pytest

import test_kernel_census_cpu as census
from fq3hip import _lib
from fq3hip.audio_out import AudioOutSpec
from fq3hip.watermark import MarkSpec
from test_stage_group_cpu import _wrapper

census.COVERAGE["mark_embed_group_kernel"] = ("test_gpu_mark_group.py", "test_gpu_mark_group.py", "mark_kernels.cuh")


def test_symbol_binding_and_range_checks():
    lib = _lib.load()
    assert hasattr(lib, "fq3_mark_push_group") and _lib.SIGNATURES["fq3_mark_push_group"] == _lib.SIGNATURES["fq3_limit_push_group"]
    fn = lib.fq3_mark_push_group
    one_p, one_l, one_i = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0), (C.c_int * 1)(0)
    full = [one_p, 1, one_p, one_l, one_i, one_p, one_l, one_l, None]
    for B in (-1, 33):
        assert fn(*(full[:1] + [B] + full[2:])) == _lib.FQ3_EINVAL and b"32" in lib.fq3_last_error(), B
    for at in (0, 2, 3, 4, 5, 6, 7, 8):                         # every array in turn; 8: none, but a null object in the array
        assert fn(*[None if i == at else v for i, v in enumerate(full)]) == _lib.FQ3_EINVAL, at
    assert fn(None, 0, None, None, None, None, None, None, None) == 0      # B == 0: nothing to do


def test_watermark_keyword_validation():
    w = _wrapper()
    a, b = MarkSpec(5, 0.1), MarkSpec(6, 0.25)
    assert w._batch_marks(None, 3) is None and w._batch_marks([None, None], 2) is None
    assert w._batch_marks(a, 2) == [a, a] and w._batch_marks([a, None, b], 3) == [a, None, b]
    fast = AudioOutSpec(8000, "mulaw", 1.25)
    for bad, n, outputs in (([a, b], 3, None), (5, 1, None), ([a, "key"], 2, None), ({"key": 5}, 1, None), (MarkSpec(5, 0.0), 1, None),
                            ([a, b], 2, [None, fast])):
        with pytest.raises(ValueError):
            w._batch_marks(bad, n, outputs)
    assert w._batch_marks([a, None], 2, [None, fast]) == [a, None]          # the row with the speed carries no mark
    with pytest.raises(ValueError, match="speed"):
        w.generate_voice_clone_batch(["a", "b"], language="English", watermark=a, output=fast)
    with w.watermark(5), pytest.raises(ValueError, match="watermark="):     # the context carries one key: it keeps refusing the batch
        w._batch_marks(a, 1)


@pytest.mark.parametrize("long", [False, True])
def test_cli_serve_lanes_with_the_watermark_key(tmp_path, long):
    # clone mode with --lanes: the batch call takes the mark; with --long the lines go one by one inside the context, as before
    import contextlib
    import numpy as np
    from fq3hip import cli
    calls, one = [], ([np.zeros(240, np.float32)], 24000)

    @contextlib.contextmanager
    def context(key, strength=0.1):
        calls.append(("context", MarkSpec(key, strength)))
        yield
    m = SimpleNamespace(sample_rate=24000, watermark=context, generate_long_voice_clone=lambda text, **kw: calls.append(("long", text)) or one,
                        generate_voice_clone_batch=lambda texts, watermark=None, **kw: calls.append(("batch", list(texts), watermark)) or [one] * len(texts))
    argv = ["serve", "--ref-audio", "r.wav", "--ref-text", "t", "--lanes", "2", "--watermark-key", "0x11", "--output-dir", str(tmp_path)]
    cli.cmd_serve(cli.build_parser().parse_args(argv + ["--long"] * long), model=m, lines=["a\n", "bb\n", "exit\n"])
    spec = MarkSpec(0x11, 0.1)
    assert calls == ([("context", spec), ("long", "a"), ("long", "bb")] if long else [("batch", ["a", "bb"], spec)])
