"""GPU: the voice library search (voices_kernels.cuh: voices_add, voices_query_pack, voices_scan, voices_merge) through the C ABI against
the float64 reference of tests/_voices_ref.py, its exact rules bit for bit, and one case through the Python interface.

Largest error observed against the bound of _voices_ref.bound (MI355X): see profiles/voice_library.json."""
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

from fq3hip import _lib as L                                                # noqa: E402
from tests import _voices_ref as R                                          # noqa: E402


class Lib:
    """fq3_voices_* on numpy arrays"""

    def __init__(self, dim, capacity, slab=None):
        self.lib, self.h, self.dim = L.load(), L.vp(), dim
        L.check(self.lib.fq3_voices_create(dim, capacity, C.byref(self.h)))
        if slab:
            L.check(self.lib.fq3_voices_set_option(self.h, b"slab_rows", slab))
        self.slab = self.lib.fq3_voices_slab_rows(self.h)

    def __del__(self):
        self.lib.fq3_voices_destroy(self.h)

    def add(self, rows):
        t = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
        first = self.lib.fq3_voices_add(self.h, t.data_ptr(), t.shape[0], torch.cuda.current_stream().cuda_stream)
        assert first >= 0, self.lib.fq3_last_error()
        torch.cuda.synchronize()
        return first

    def drop(self, index):
        L.check(self.lib.fq3_voices_drop(self.h, index, torch.cuda.current_stream().cuda_stream))

    def search(self, q, k):
        t = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        idx = torch.full((t.shape[0], k), 77, dtype=torch.int32, device="cuda")
        cos = torch.full((t.shape[0], k), 77.0, dtype=torch.float32, device="cuda")
        L.check(self.lib.fq3_voices_search(self.h, t.data_ptr(), t.shape[0], k, idx.data_ptr(), cos.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return idx.cpu().numpy(), cos.cpu().numpy()


def slab_rows():
    return Lib(16, 1).slab


def sizes():
    s = slab_rows()
    return [1, 15, 16, 17, s - 1, s, s + 1, 2 * s + 5]


@pytest.mark.parametrize("dim", [16, 64, 1024])
@pytest.mark.parametrize("n_at", range(8))
def test_against_float64(dim, n_at):
    n = sizes()[n_at]
    lib_rows, queries = R.ladder(dim, n, 32, seed=1000 * dim + n)
    lib, tol, worst = Lib(dim, n), R.bound(dim), 0.0
    lib.add(lib_rows)
    for rows in (1, 16, 17, 32):
        want_idx, want_cos = R.top_k(lib_rows, queries[:rows], 17)           # one rank more: the gap behind the last compared rank
        have = min(n, 16)
        gaps = want_cos[:, :have] - np.where(want_idx[:, 1:have + 1] >= 0, want_cos[:, 1:have + 1], -2.0)
        assert gaps.min() >= 1e-3 > 2 * tol, "the inputs do not decide every rank"     # a property of the inputs: float64 alone
        for k in (1, 5, 16):
            idx, cos = lib.search(queries[:rows], k)
            m = min(n, k)
            assert np.array_equal(idx[:, :m], want_idx[:, :m]) and (idx[:, m:] == -1).all() and (cos[:, m:] == -2.0).all(), (rows, k)
            worst = max(worst, float(np.abs(cos[:, :m] - want_cos[:, :m]).max()))
    print(f"dim {dim} N {n}: max |cos - cos64| {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol


@pytest.fixture(scope="module")
def rows64():
    rng = np.random.default_rng(7)
    return rng.standard_normal((2 * slab_rows() + 40, 64)).astype(np.float32), rng.standard_normal((32, 64)).astype(np.float32)


def _cos_of(lib, q, index, k=16):
    """bits of library row `index`'s cosine per query; the row must be among each query's k best"""
    idx, cos = lib.search(q, k)
    at = [list(r).index(index) for r in idx]
    return np.array([cos[i, a] for i, a in enumerate(at)]).view(np.uint32)


def test_duplicates_come_in_index_order_with_equal_bits(rows64):
    x, q = rows64
    lib = Lib(64, 64)
    lib.add(np.stack([x[0], x[1], x[0], x[2], x[0]] + list(x[3:40])))
    idx, cos = lib.search(x[:1] * 3.0, 5)
    assert list(idx[0, :3]) == [0, 2, 4] and len(set(cos[0, :3].view(np.uint32))) == 1 and abs(cos[0, 0] - 1.0) <= R.bound(64)


@pytest.mark.parametrize("case", ["rows_in_front", "across_a_slab", "query_place", "three_adds", "slab_size"])
def test_a_rows_cosine_bits_do_not_move(rows64, case):
    x, q = rows64
    s = slab_rows()
    target = (q[:1] + 0.05 * x[:1]) * 2.0                                     # close to query 0: among its best wherever it sits
    alone = Lib(64, 8)
    alone.add(target)
    want = _cos_of(alone, q[:1], 0)
    other = Lib(64, len(x) + 1, slab=128 if case == "slab_size" else None)
    if case == "rows_in_front":
        other.add(np.concatenate([x[:17], target]))
        got = _cos_of(other, q[:1], 17)
    elif case == "across_a_slab":
        other.add(np.concatenate([x[:s - 1], target]))
        before = _cos_of(other, q[:1], s - 1)
        other.add(x[s:s + 30])                                              # N grows from one slab to two
        got = _cos_of(other, q[:1], s - 1)
        assert np.array_equal(before, got)
    elif case == "query_place":
        other.add(np.concatenate([x[:5], target]))
        idx, cos = other.search(np.concatenate([q[1:32], q[:1]]), 16)        # the query as row 31 of 32
        got = cos[31][list(idx[31]).index(5)].reshape(1).view(np.uint32)
    elif case == "three_adds":
        assert [other.add(x[:7]), other.add(np.concatenate([x[7:20], target])), other.add(x[20:41])] == [0, 7, 21]
        got = _cos_of(other, q[:1], 20)
    else:
        other.add(np.concatenate([x[:2 * s + 9], target]))
        got = _cos_of(other, q[:1], 2 * s + 9)
    assert np.array_equal(got, want)


def test_dropped_and_zero_rows(rows64):
    x, q = rows64
    rows = x[:40].copy()
    rows[3] = 0.0
    lib = Lib(64, 40)
    lib.add(rows)
    best = int(lib.search(q[:1], 1)[0][0, 0])
    lib.drop(best)
    lib.drop(11)
    idx, cos = lib.search(q[:2], 16)
    want_idx, _ = R.top_k(rows, q[:2], 16, dead=(best, 11))
    assert np.array_equal(idx, want_idx) and best not in idx and 11 not in idx
    idx, cos = lib.search(np.concatenate([q[:1], np.zeros((1, 64), np.float32)]), 16)
    assert (cos[1].view(np.uint32) == 0).all() and list(idx[1]) == [i for i in range(40) if i not in (best, 11)][:16]      # a zero query: every cosine +0
    tiny = Lib(64, 4)
    tiny.add(rows[2:5])
    idx, cos = tiny.search(q[:1], 3)
    assert cos[0][list(idx[0]).index(1)].view(np.uint32) == 0               # the zero row scores exactly 0


REFUSALS = {   # call on a live library of 5 rows, capacity 8 -> (code, a word of fq3_last_error)
    "search_rows_0": (lambda v, t: v.fq3_voices_search(t.h, t.p, 0, 1, t.p, t.p, None), L.FQ3_EINVAL, b"rows = 0"),
    "search_rows_33": (lambda v, t: v.fq3_voices_search(t.h, t.p, 33, 1, t.p, t.p, None), L.FQ3_EINVAL, b"rows = 33"),
    "search_k_0": (lambda v, t: v.fq3_voices_search(t.h, t.p, 1, 0, t.p, t.p, None), L.FQ3_EINVAL, b"k = 0"),
    "search_k_17": (lambda v, t: v.fq3_voices_search(t.h, t.p, 1, 17, t.p, t.p, None), L.FQ3_EINVAL, b"k = 17"),
    "search_null_q": (lambda v, t: v.fq3_voices_search(t.h, None, 1, 1, t.p, t.p, None), L.FQ3_EINVAL, b"null"),
    "search_null_idx": (lambda v, t: v.fq3_voices_search(t.h, t.p, 1, 1, None, t.p, None), L.FQ3_EINVAL, b"null"),
    "search_null_cos": (lambda v, t: v.fq3_voices_search(t.h, t.p, 1, 1, t.p, None, None), L.FQ3_EINVAL, b"null"),
    "workspace_k_17": (lambda v, t: v.fq3_voices_search_workspace(t.h, 1, 17), L.FQ3_EINVAL, b"k = 17"),
    "add_rows_0": (lambda v, t: v.fq3_voices_add(t.h, t.p, 0, None), L.FQ3_EINVAL, b"rows"),
    "add_null": (lambda v, t: v.fq3_voices_add(t.h, None, 1, None), L.FQ3_EINVAL, b"null"),
    "add_full": (lambda v, t: v.fq3_voices_add(t.h, t.p, 4, None), L.FQ3_ENOMEM, b"5 of 8 taken"),
    "drop_minus_1": (lambda v, t: v.fq3_voices_drop(t.h, -1, None), L.FQ3_EINVAL, b"index -1"),
    "drop_count": (lambda v, t: v.fq3_voices_drop(t.h, 5, None), L.FQ3_EINVAL, b"index 5"),
    "option_name": (lambda v, t: v.fq3_voices_set_option(t.h, b"slab", 128), L.FQ3_EINVAL, b"unknown option"),
    "option_value": (lambda v, t: v.fq3_voices_set_option(t.h, b"slab_rows", 64), L.FQ3_EINVAL, b"128, 256 or 512"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_on_a_live_library_change_nothing(rows64, case):
    x, q = rows64
    lib = Lib(64, 8)
    lib.add(x[:5])
    lib.buf = torch.zeros(64 * 64, device="cuda")                           # room for whatever a call that got through would touch
    lib.p = lib.buf.data_ptr()
    before = lib.search(q[:2], 5)
    call, code, word = REFUSALS[case]
    assert call(lib.lib, lib) == code and word in lib.lib.fq3_last_error(), lib.lib.fq3_last_error()
    assert lib.lib.fq3_voices_count(lib.h) == 5 and lib.slab == lib.lib.fq3_voices_slab_rows(lib.h)
    after = lib.search(q[:2], 5)                                             # the object is as it was and stays usable
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    assert lib.add(x[5:8]) == 5 and list(lib.search(x[7:8], 1)[0][0]) == [7]


def test_a_clip_finds_itself_through_the_python_interface():
    import dataclasses
    from fq3hip.config import tiny_ref_audio_config, tiny_test_config
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.voice_library import VoiceLibrary
    from fq3hip.weights import synth_ref_audio_weights, synth_weights
    from tests.test_refenc_oracle_pins import make_wave
    cfg = tiny_test_config()
    cfg.ref_audio = dataclasses.replace(tiny_ref_audio_config(), enc_dim=cfg.talker.hidden_size)
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "codec", "text"))
    W.update({k: v for k, v in synth_ref_audio_weights(cfg.ref_audio, 2).items() if k.startswith("speaker_encoder.")})
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, codec_max_frames=128, max_frames=64)
    an = m.model.ref_analyzer
    clips = [make_wave(2000 + 301 * i, seed=40 + i) for i in range(35)]
    lib = VoiceLibrary(an.cfg.enc_dim, 64, "cuda")
    assert lib.add(an.speaker_embeddings(clips), [f"voice{i}" for i in range(35)]) == 0 and len(lib) == 35
    found = an.nearest(clips, lib, k=2)                                     # 35 queries: two slices
    assert [f[0][0] for f in found] == [f"voice{i}" for i in range(35)] and all(abs(f[0][1] - 1.0) <= 1e-5 and f[1][1] <= f[0][1] for f in found)
    lib.drop("voice4")
    from fq3hip.speaker_check import StoredEmbedding
    near = m.nearest_voices([clips[4], clips[9], dict(ref_spk_embedding=[an.speaker_embedding(clips[2])]), StoredEmbedding(an.speaker_embedding(clips[7]))],
                            24000, lib, k=1)
    assert near[0][0][0] != "voice4" and [n[0][0] for n in near[1:]] == ["voice9", "voice2", "voice7"]
