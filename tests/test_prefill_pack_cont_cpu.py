"""CPU: the packed continuation prefill without a GPU -- the mirror of the pack split rule (tests/_prefill_pack_cont_ref.py) on a pack
of one and on the packs of the GPU module; the partition logic of ``PrefixCache.prefill_pack`` against fake engines that record
calls; the new entry point in the header, the library and the binding table."""
import ctypes
import os
import re

import pytest
import torch

import _prefill_cont_ref as R1
import _prefill_pack_cont_ref as R
from fq3hip import _lib as L
from fq3hip.prefix_cache import PrefixCache
from test_prefix_cache_cpu import _FakeEngine, _note, _x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
HDR = os.path.join(ROOT, "include", "fq3hip.h")


# ---- split rule ----------------------------------------------------------------------------------------------------------
def test_a_pack_of_one_splits_like_the_single_kernel():
    for start, n in R1.CASES:
        for n_cu in (R1.N_CU, 304, 64):
            assert R.pack_splits([start], [n], n_cu=n_cu) == [R1.splits(start, n, n_cu=n_cu)], (start, n, n_cu)
    # the product shape: 128 new rows, 16 heads, behind 3968 keys, and a workspace that forces the shrink loop
    for ws in (8 << 20, 3 * 128 * 16 * R.REC, 128 * 16 * R.REC):
        assert R.pack_splits([3968], [128], nh=16, ws_floats=ws) == [R1.splits(3968, 128, nh=16, ws_floats=ws)], ws


@pytest.mark.parametrize("name", sorted(R.PACKS))
def test_the_packs_fit_the_workspace_and_keep_their_tiles(name):
    pack = R.PACKS[name]
    assert 1 <= len(pack) <= R.MAX_PACK
    starts, cnts = [s for s, _ in pack], [n for _, n in pack]
    for n_cu in (R.N_CU, 304):
        S = R.pack_splits(starts, cnts, n_cu=n_cu)
        assert R.pack_ws_floats(cnts, S) <= R.WS_FLOATS
        for (s, n), sq in zip(pack, S):
            assert 1 <= sq <= R.MAX_SPLIT
            assert sq == 1 or R.tiles_of(s, n) // sq >= R.MIN_TILES, (name, s, n, sq)
    if name == "D":
        assert len(set(R.pack_splits(starts, cnts))) > 1                 # mixed split counts in one launch
        for f in R.FORCED_D:
            assert R.pack_ws_floats(cnts, [f] * len(cnts)) <= R.WS_FLOATS


def test_the_shrink_takes_from_the_largest_split_first():
    starts, cnts = [1000, 1000, 200], [64, 64, 64]
    S = R.pack_splits(starts, cnts, n_cu=4096)
    assert S == [4, 4, 1]
    one = 64 * R.NH * R.REC
    assert R.pack_splits(starts, cnts, n_cu=4096, ws_floats=7 * one) == [3, 4, 1]
    assert R.pack_splits(starts, cnts, n_cu=4096, ws_floats=6 * one) == [3, 3, 1]
    assert R.pack_splits(starts, cnts, n_cu=4096, ws_floats=one) == [1, 1, 1]      # a single split stores no record
    assert R.pack_splits(starts, cnts, n_cu=4096, ws_floats=0) == [1, 1, 1]


def test_pack_tables_interleave_the_sequences():
    for name, pack in R.PACKS.items():
        n_blocks, tables = R.pack_tables(pack)
        ids = [b for t in tables for b in t]
        assert len(set(ids)) == len(ids) == n_blocks - 3 and all(0 <= b < n_blocks for b in ids)
        assert [len(t) for t in tables] == [R.tiles_of(s, n) for s, n in pack]
    assert len({R.v_scale(q) for q in range(14)}) == 14


# ---- PrefixCache.prefill_pack against fake engines -------------------------------------------------------------------------
@pytest.fixture()
def packed(monkeypatch):
    """Fq3Engine's two static packed calls, recorded in the engines' shared log."""
    from fq3hip.engine import Fq3Engine

    def prefill_batch(engines, embeds, n_pads=None, want_logits=True):
        engines[0].log.append(("prefill_batch", [e.name for e in engines], [int(x.shape[0]) for x in embeds], list(n_pads), want_logits))
        return [(f"lg:{e.name}" if want_logits else None, f"hd:{e.name}") for e in engines]

    def prefill_continue_batch(engines, embeds, starts):
        engines[0].log.append(("prefill_continue_batch", [e.name for e in engines], [int(x.shape[0]) for x in embeds], list(starts)))
        return [(f"lg+:{e.name}", f"hd+:{e.name}") for e in engines]

    monkeypatch.setattr(Fq3Engine, "prefill_batch", staticmethod(prefill_batch))
    monkeypatch.setattr(Fq3Engine, "prefill_continue_batch", staticmethod(prefill_continue_batch))


def _members(n):
    log, table = [], object()
    gen = _FakeEngine(log, name="gen", table=table)
    gen.max_seq_len = 2048
    ms = []
    for i in range(n):
        e = _FakeEngine(log, name=f"m{i}", table=table)
        e.max_seq_len = 2048
        ms.append(e)
    return gen, ms, log


def test_prefill_pack_partitions_the_group(packed):
    gen, ms, log = _members(6)
    cache = PrefixCache(gen, capacity_rows=1024, min_rows=64)
    voice_a, voice_b = list(range(100, 170)), list(range(300, 390))                 # 70 and 90 instruct rows
    cache.prefill(gen, _x(200), 0, _note(voice_b))                                    # voice_b is cached by an earlier request
    before = cache.stats()
    assert before["misses"] == 1
    del log[:]
    xs = [_x(200), _x(150), _x(180), _x(120), _x(220), _x(70)]
    pads = [0, 0, 0, 0, 5, 0]
    notes = [_note(voice_a), _note(voice_b), _note(voice_a), None, _note(voice_a), _note(voice_a)]     # m4 left-padded, m5: P >= L
    res = cache.prefill_pack(ms, xs, pads, notes)
    calls = [c for c in log if c[0] in ("prefill_batch", "prefill_continue_batch") or c[1] in ("prefill", "kv_copy", "prefill_continue")]
    assert calls == [
        ("prefill_batch", ["m3", "m4", "m5"], [120, 220, 70], [0, 5, 0], True),      # the rest: today's call
        ("m1", "kv_copy", "entry1", 90),                                             # the hit
        ("m0", "prefill", 70, 0, False),                                             # the one distinct miss, once
        ("entry2", "kv_copy", "m0", 70),                                             # saved
        ("m2", "kv_copy", "m0", 70),                                                 # the second member of the same key
        ("prefill_continue_batch", ["m0", "m1", "m2"], [130, 60, 110], [70, 90, 70]),
    ]
    assert res == [("lg+:m0", "hd+:m0"), ("lg+:m1", "hd+:m1"), ("lg+:m2", "hd+:m2"), ("lg:m3", "hd:m3"), ("lg:m4", "hd:m4"), ("lg:m5", "hd:m5")]
    st = cache.stats()
    assert [st[k] - before[k] for k in ("misses", "hits", "bypasses", "rows_reused", "evictions")] == [1, 2, 3, 160, 0] and st["entries"] == 2
    # the same group again: all hits, no prefix prefill, no save
    del log[:]
    cache.prefill_pack(ms, xs, pads, notes)
    assert [c for c in log if c[1] == "prefill"] == [] and [c for c in log if c[1] == "kv_copy"] == [
        ("m0", "kv_copy", "entry2", 70), ("m1", "kv_copy", "entry1", 90), ("m2", "kv_copy", "entry2", 70)]
    assert cache.stats()["hits"] == 5 and cache.stats()["misses"] == 2


def test_prefill_pack_without_notes_is_the_plain_packed_prefill(packed):
    gen, ms, log = _members(3)
    cache = PrefixCache(gen, capacity_rows=1024)
    res = cache.prefill_pack(ms, [_x(50), _x(60), _x(70)], [0, 2, 0], [None, None, None])
    assert log == [("prefill_batch", ["m0", "m1", "m2"], [50, 60, 70], [0, 2, 0], True)]
    assert res == [("lg:m0", "hd:m0"), ("lg:m1", "hd:m1"), ("lg:m2", "hd:m2")] and cache.stats()["bypasses"] == 3


def test_prefill_pack_several_misses_share_one_prefix_pass_and_split_at_the_workspace(packed):
    gen, ms, log = _members(3)
    for e in ms:
        e.max_seq_len = 256
    cache = PrefixCache(gen, capacity_rows=1024, min_rows=64)
    va, vb, vc = list(range(0, 64)), list(range(100, 228)), list(range(300, 428))
    cache.prefill_pack(ms, [_x(100), _x(200), _x(250)], [0, 0, 0], [_note(va), _note(vb), _note(vc)])
    packed_calls = [c for c in log if c[0] in ("prefill_batch", "prefill_continue_batch")]
    assert packed_calls == [
        ("prefill_batch", ["m0", "m1"], [64, 128], [0, 0], False),                   # 64 + 128 + 128 prefix rows exceed 256: a second pass
        ("prefill_continue_batch", ["m0", "m1", "m2"], [36, 72, 122], [64, 128, 128]),
    ]
    assert ("m2", "prefill", 128, 0, False) in log
    assert cache.stats()["misses"] == 3 and cache.stats()["entries"] == 3


def test_prefill_pack_eviction_keeps_every_member_served(packed):
    gen, ms, log = _members(3)
    cache = PrefixCache(gen, capacity_rows=128, min_rows=64)                        # two blocks: one 128-row voice at a time
    va, vb = list(range(0, 128)), list(range(500, 628))
    res = cache.prefill_pack(ms, [_x(200), _x(200), _x(200)], [0, 0, 0], [_note(va), _note(vb), _note(va)])
    assert [r[0] for r in res] == ["lg+:m0", "lg+:m1", "lg+:m2"]
    assert ("m2", "kv_copy", "m0", 128) in log                                      # from the member: va's entry is gone by then
    st = cache.stats()
    assert (st["misses"], st["hits"], st["evictions"], st["entries"]) == (2, 1, 1, 1)


# ---- C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def test_entry_point_declared_exported_and_bound(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(fq3_[a-z0-9_]+)\s*\(", src))
    n = "fq3_prefill_continue_batch"
    assert n in declared and hasattr(lib, n) and n in L.SIGNATURES
    assert len(L.SIGNATURES[n][1]) == 8
    lib.fq3_abi_version.restype = ctypes.c_int
    assert lib.fq3_abi_version() == 5


def test_null_arguments_return_einval_without_a_gpu(lib):
    vp = ctypes.c_void_p
    fn = lib.fq3_prefill_continue_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    assert fn(None, 1, None, None, None, None, None, None) == -1
    one = (vp * 1)(None)
    ints = (ctypes.c_int * 1)(4)
    for n in (0, 65):
        assert fn(one, n, one, ints, ints, one, one, None) == -1
    assert fn(one, 1, one, ints, ints, one, one, None) == -1                       # a null context


def test_engine_and_scheduler_carry_the_new_surface():
    import inspect
    from fq3hip.batching import BatchDecoder
    from fq3hip.engine import Fq3Engine
    from fq3hip.model import FasterQwen3TTS
    assert callable(getattr(Fq3Engine, "prefill_continue_batch"))
    assert inspect.signature(BatchDecoder.__init__).parameters["prefix_cache"].default is None
    assert inspect.signature(FasterQwen3TTS.enable_prefix_cache).parameters["batch"].default is False
