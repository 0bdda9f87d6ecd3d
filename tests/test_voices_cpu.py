"""CPU: the host half of ``fq3_voices_*`` and the Python / CLI layers over stand-ins.  The kernels of
csrc/voices_kernels.cuh get their lines of the kernel census from here: their reference test is tests/test_gpu_voices.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_kernel_census_cpu as census
from fq3hip import _lib
from fq3hip.voice_library import VoiceLibrary

census.COVERAGE.update({k: ("test_gpu_voices.py", "test_gpu_voices.py", "voices_kernels.cuh")
                        for k in ("voices_add_kernel", "voices_query_pack_kernel", "voices_scan_kernel", "voices_merge_kernel")})


def test_symbols_bound_and_the_refusals_that_need_no_object():
    """create's ranges and every null object; the refusals on a live object need the device: tests/test_gpu_voices.py"""
    lib = _lib.load()
    h, one = _lib.vp(), (_lib.vp * 1)(None)
    E = _lib.FQ3_EINVAL
    for dim, cap, out in ((64, 8, None), (0, 8, C.byref(h)), (24, 8, C.byref(h)), (8208, 8, C.byref(h)), (64, 0, C.byref(h)), (64, (1 << 22) + 1, C.byref(h))):
        assert lib.fq3_voices_create(dim, cap, out) == E and not h.value, (dim, cap)
    assert b"capacity" in lib.fq3_last_error()
    assert lib.fq3_voices_count(None) == E and lib.fq3_voices_reset(None) == E and lib.fq3_voices_destroy(None) == 0
    assert lib.fq3_voices_add(None, one, 1, None) == E and lib.fq3_voices_drop(None, 0, None) == E
    assert lib.fq3_voices_search(None, one, 1, 1, one, one, None) == E and lib.fq3_voices_search_workspace(None, 1, 1) == E
    assert lib.fq3_voices_slab_rows(None) == E and lib.fq3_voices_set_option(None, b"slab_rows", 128) == E


class _Library(VoiceLibrary):
    """The wrapper's bookkeeping over a library that only records; its search answers with the rows' own indices, cosine 1 - row / 100."""

    def _create(self):
        self.calls, self.count = [], 0

    def _add_call(self, embeds):
        self.calls.append(("add", embeds.shape[0]))
        self.count += embeds.shape[0]
        return self.count - embeds.shape[0]

    def _drop_call(self, index):
        self.calls.append(("drop", index))

    def _search_call(self, q, k, idx, cos):
        self.calls.append(("search", q.shape[0], k))
        for r in range(q.shape[0]):
            for j in range(k):
                idx[r, j] = int(q[r, 0]) + j if j < 2 else -1
                cos[r, j] = 1.0 - j / 100 if j < 2 else -2.0


def test_names_slices_drop_save_and_load(tmp_path):
    lib = _Library(4, 100, "cpu")
    e = np.arange(80, dtype=np.float32).reshape(20, 4) * 0 + np.arange(20, dtype=np.float32)[:, None]
    assert lib.add(e[:12], [f"v{i}" for i in range(12)]) == 0 and lib.add(e[12:], [f"v{i}" for i in range(12, 20)]) == 12 and len(lib) == 20
    for rows, bad in ((e[:1], ["v0"]), (e[:2], ["a", "a"]), (e[:2], ["only"]), (np.zeros((1, 8), np.float32), ["wide"])):
        with pytest.raises(ValueError):
            lib.add(rows, bad)
    lib.calls.clear()
    q = np.zeros((70, 4), np.float32)
    q[:, 0] = np.arange(70) % 18
    found = lib.search(q, k=3)
    assert lib.calls == [("search", 32, 3), ("search", 32, 3), ("search", 6, 3)]
    assert found[5] == [("v5", 1.0), ("v6", pytest.approx(0.99))] and len(found) == 70            # the -1 slot is left out
    lib.drop("v6")
    assert lib.calls[-1] == ("drop", 6) and len(lib) == 19 and lib.names[6] is None
    with pytest.raises(KeyError):
        lib.drop("v6")
    with pytest.raises(ValueError):
        lib.search(q, k=17)
    assert lib.search(np.zeros((0, 4), np.float32)) == []
    path = tmp_path / "lib.npz"
    lib.save(path)
    back = _Library.load(path, "cpu")
    assert back.dim == 4 and back.capacity == 1024 and len(back) == 19 and back.calls == [("add", 19)]
    assert back.names[6] == "v7" and np.array_equal(np.stack(back._raw), np.delete(e, 6, axis=0))


def _cli_model(near):
    asked = []
    item = lambda v: SimpleNamespace(ref_spk_embedding=torch.tensor([v, 1.0, 0.0, 0.0]), ref_text="")
    model = SimpleNamespace(
        create_voice_clone_prompts=lambda audios, texts, x_vector_only_mode: [item(float(i)) for i in range(len(audios))],
        nearest_voices=lambda audio, sr, library, k=1: asked.append((len(audio), sr, len(library), k)) or near[:len(audio)],
        _voice_cache_entry=lambda p, xvec, flag: (np.zeros(10, np.float32), "key", {}, False, "id"))
    return model, asked


def test_cli_voices_build_and_search(tmp_path, monkeypatch, capsys):
    from fq3hip import cli, voice_library
    from fq3hip.audio_io import write_wav
    paths = [str(tmp_path / f"{i}.wav") for i in range(2)]
    for p in paths:
        write_wav(p, np.zeros(2400, np.float32), 16000)
    model, asked = _cli_model([[("a", 0.9), ("b", 0.5)], [("b", 0.25), ("a", 0.125)]])
    monkeypatch.setattr(cli, "load_model", lambda args: model)
    monkeypatch.setattr(voice_library, "VoiceLibrary", _Library)
    out = str(tmp_path / "lib.npz")
    cli.main(["--device", "cpu", "voices", "build", "--out", out] + paths)
    with np.load(out) as z:
        assert list(z["names"]) == paths and z["embeds"].shape == (2, 4)
    capsys.readouterr()
    cli.main(["--device", "cpu", "voices", "search", "--lib", out, "--k", "2"] + paths)
    assert asked == [(2, [16000, 16000], 2, 2)]
    assert capsys.readouterr().out.splitlines() == [f"{paths[0]}: a 0.900000", f"{paths[0]}: b 0.500000", f"{paths[1]}: b 0.250000", f"{paths[1]}: a 0.125000"]
    cli.main(["--device", "cpu", "voices", "search", "--lib", out, "--refuse-above", "0.95"] + paths)        # below the threshold: exit 0
    with pytest.raises(SystemExit) as exc:
        cli.main(["--device", "cpu", "voices", "search", "--lib", out, "--refuse-above", "0.9"] + paths)
    assert exc.value.code == 3


def test_cli_enroll_blocklist(tmp_path, monkeypatch, capsys):
    from fq3hip import cli, voice_cache, voice_library
    model, asked = _cli_model([[("blocked", 0.8)], [("blocked", 0.3)]])
    written = []
    monkeypatch.setattr(cli, "load_model", lambda args: model)
    monkeypatch.setattr(voice_library, "VoiceLibrary", _Library)
    monkeypatch.setattr(voice_cache, "VoiceRefCache", lambda d: d)
    monkeypatch.setattr(voice_cache, "export_voice_clone_prompt", lambda cache, audio, item, **kw: written.append(cache) or "k")
    block = str(tmp_path / "block.npz")
    _Library(4, 8, "cpu").save(block)
    base = ["--device", "cpu", "enroll", "--out", str(tmp_path / "cache")]
    for flags in (["--blocklist", block], ["--refuse-above", "0.5"]):         # both flags or neither
        with pytest.raises(SystemExit) as exc:
            cli.main(base + flags + ["a.wav"])
        assert "go together" in str(exc.value.code) and not written
    with pytest.raises(SystemExit) as exc:
        cli.main(base + ["--blocklist", block, "--refuse-above", "0.5", "a.wav", "b.wav"])
    assert exc.value.code == 3 and not written and "REFUSED a.wav: blocked 0.800000" in capsys.readouterr().out
    cli.main(base + ["--blocklist", block, "--refuse-above", "0.85", "a.wav", "b.wav"])
    assert len(written) == 2 and asked[-1] == (2, 24000, 0, 1)
    cli.main(base + ["a.wav"])                                               # without the flags: no library is consulted
    assert len(written) == 3 and len(asked) == 2
