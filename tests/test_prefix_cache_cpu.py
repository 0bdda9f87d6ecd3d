"""CPU: the prefix KV cache without a GPU -- the two new entry points in the header, the library and the binding table; the host
logic of fq3hip/prefix_cache.py against a fake engine that records calls; the premise (instruct rows first, a function of the
instruct ids alone) on the CPU prompt paths; the server and CLI flags."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from fq3hip import _lib as L
from fq3hip.prefix_cache import PrefixCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
HDR = os.path.join(ROOT, "include", "fq3hip.h")
NEW = ("fq3_prefill_continue", "fq3_kv_copy")


# ---- C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def test_entry_points_declared_exported_and_bound(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(fq3_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in declared and hasattr(lib, n) and n in L.SIGNATURES, n
    lib.fq3_abi_version.restype = ctypes.c_int
    assert lib.fq3_abi_version() == 5


def test_null_arguments_return_einval_without_a_gpu(lib):
    vp = ctypes.c_void_p
    lib.fq3_prefill_continue.restype = ctypes.c_int
    lib.fq3_prefill_continue.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    lib.fq3_kv_copy.restype = ctypes.c_int
    lib.fq3_kv_copy.argtypes = [vp, vp, ctypes.c_int, vp]
    assert lib.fq3_prefill_continue(None, None, 0, 4, None, None, None) == -1
    assert lib.fq3_kv_copy(None, None, 64, None) == -1


# ---- PrefixCache against a fake engine -----------------------------------------------------------------------------------
class _FakePool:
    def __init__(self, n_blocks):
        self.n, self.free, self.high = n_blocks, n_blocks, 0

    def stats(self):
        return {"blocks": self.n, "free": self.free, "high_water": self.high, "bytes_per_block": 0}

    def close(self):
        self.closed = True


class _FakeEngine:
    """Duck-typed Fq3Engine: records every call in a log shared with the contexts it spawns; pooled contexts keep block accounts."""

    def __init__(self, log=None, pool=None, name="gen", dtype=torch.bfloat16, table=None):
        self.log = log if log is not None else []
        self.pool, self.name, self.dtype, self.blocks, self.n_spawned = pool, name, dtype, 0, 0
        self._table = table if table is not None else object()

    def kv_pool(self, n_blocks):
        self.made_pool = _FakePool(n_blocks)
        return self.made_pool

    def spawn_pooled(self, pool):
        self.n_spawned += 1
        return _FakeEngine(self.log, pool, f"entry{self.n_spawned}", self.dtype, self._table)

    def prefill(self, x, n_pad=0, want_logits=True):
        self.log.append((self.name, "prefill", int(x.shape[0]), n_pad, want_logits))
        return "logits", "hidden"

    def prefill_continue(self, x, start):
        self.log.append((self.name, "prefill_continue", int(x.shape[0]), start))
        return "logits+", "hidden+"

    def kv_copy(self, src, rows):
        need = (rows + 63) // 64
        if self.pool is not None:
            if need - self.blocks > self.pool.free:
                raise L.Fq3Error(L.FQ3_ENOMEM, "KV pool exhausted")
            self.pool.free -= need - self.blocks
            self.pool.high = max(self.pool.high, self.pool.n - self.pool.free)
            self.blocks = need
        self.log.append((self.name, "kv_copy", src.name, rows))

    def kv_release(self, keep=0):
        if self.pool is not None:
            self.pool.free += self.blocks
            self.blocks = 0
        self.log.append((self.name, "kv_release"))

    def close(self):
        self.log.append((self.name, "close"))


def _x(rows):
    return torch.zeros(rows, 8)


def _note(ids):
    return (len(ids), tuple(ids))


def test_miss_then_hit_call_sequences_and_stats():
    eng = _FakeEngine()
    cache = PrefixCache(eng, 256, min_rows=1)
    ids = list(range(100))
    out = cache.prefill(eng, _x(130), 0, _note(ids))
    assert out == ("logits+", "hidden+")
    assert eng.log == [("gen", "prefill", 100, 0, False), ("entry1", "kv_copy", "gen", 100), ("gen", "prefill_continue", 30, 100)]
    del eng.log[:]
    cache.prefill(eng, _x(150), 0, _note(ids))
    assert eng.log == [("gen", "kv_copy", "entry1", 100), ("gen", "prefill_continue", 50, 100)]
    st = cache.stats()
    assert st == dict(hits=1, misses=1, bypasses=0, evictions=0, rows_reused=100, entries=1, blocks_held=2, blocks_capacity=4)
    cache.clear()
    assert cache.stats()["entries"] == 0 and cache.stats()["blocks_held"] == 0 and eng.made_pool.free == 4
    assert cache.stats()["hits"] == 1                            # the counters stay
    del eng.log[:]
    cache.prefill(eng, _x(130), 0, _note(ids))                  # a miss again; the evicted entry's context is reused
    assert eng.log[0] == ("gen", "prefill", 100, 0, False) and eng.log[1] == ("entry1", "kv_copy", "gen", 100) and eng.n_spawned == 1
    cache.close()
    assert eng.made_pool.closed and ("entry1", "close") in eng.log


def test_lru_eviction_order_under_a_block_budget():
    eng = _FakeEngine()
    cache = PrefixCache(eng, 4 * 64, min_rows=1)                 # four blocks
    A, B, C = [1] * 100, [2] * 100, [3] * 70                     # 2 + 2 + 2 blocks
    cache.prefill(eng, _x(200), 0, _note(A))
    cache.prefill(eng, _x(200), 0, _note(B))
    cache.prefill(eng, _x(200), 0, _note(A))                    # hit: A is now the most recently used
    cache.prefill(eng, _x(200), 0, _note(C))                    # evicts B, not A
    st = cache.stats()
    assert (st["hits"], st["misses"], st["evictions"], st["entries"], st["blocks_held"]) == (1, 3, 1, 2, 4)
    del eng.log[:]
    cache.prefill(eng, _x(200), 0, _note(A))
    assert eng.log[0][1] == "kv_copy"                            # still a hit
    cache.prefill(eng, _x(200), 0, _note(B))                    # a miss: evicts C (least recently used), then fits
    assert cache.stats()["evictions"] == 2 and cache.stats()["misses"] == 4
    cache.prefill(eng, _x(300), 0, _note([4] * 250))            # four blocks: evicts both
    st = cache.stats()
    assert (st["evictions"], st["entries"], st["blocks_held"]) == (4, 1, 4)
    assert eng.made_pool.high <= 4 and eng.made_pool.free == 0


def test_keys_separate_by_ids_dtype_and_weight_table():
    eng = _FakeEngine()
    cache = PrefixCache(eng, 1024, min_rows=1)
    ids = [5] * 80
    cache.prefill(eng, _x(100), 0, _note(ids))
    cache.prefill(eng, _x(100), 0, _note(ids[:-1] + [6]))
    assert cache.stats()["misses"] == 2
    other_dtype = _FakeEngine(eng.log, name="gen32", dtype=torch.float32, table=eng._table)
    cache.prefill(other_dtype, _x(100), 0, _note(ids))
    other_table = _FakeEngine(eng.log, name="gen2", dtype=eng.dtype)
    cache.prefill(other_table, _x(100), 0, _note(ids))
    assert cache.stats()["misses"] == 4 and cache.stats()["hits"] == 0
    cache.prefill(eng, _x(100), 0, _note(ids))
    assert cache.stats()["hits"] == 1


@pytest.mark.parametrize("why", ["no note", "n_pad", "P < min_rows", "P beyond the capacity", "P == L"])
def test_bypass_conditions(why):
    eng = _FakeEngine()
    cache = PrefixCache(eng, 128, min_rows=64)
    ids = list(range(100))
    args = {"no note": (_x(130), 0, None), "n_pad": (_x(130), 3, _note(ids)), "P < min_rows": (_x(130), 0, _note(ids[:63])),
            "P beyond the capacity": (_x(200), 0, _note(list(range(129)))), "P == L": (_x(100), 0, _note(ids))}[why]
    assert cache.prefill(eng, *args) == ("logits", "hidden")
    assert eng.log == [("gen", "prefill", int(args[0].shape[0]), args[1], True)]
    st = cache.stats()
    assert (st["bypasses"], st["hits"], st["misses"], st["entries"]) == (1, 0, 0, 0)
    assert PrefixCache(eng, 128).min_rows == 64                  # the default


# ---- the premise, on the CPU prompt paths ---------------------------------------------------------------------------------
def _prompt_setup(dtype):
    from fq3hip.weights import synth_weights
    from oracle import qwen3tts_oracle as O
    from oracle.make_golden_prompt import case_config
    from test_prompt_builder_cpu import _FakeEngine as PromptEngine
    cfg = case_config()
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    om = O.OraclePromptModel(cfg, W)
    eng = PromptEngine(cfg, W)
    return cfg, om, eng


def _ids(n, seed, vocab=200):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(10, vocab, (1, n), generator=g)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("path", ["hip row program", "tensor ops"])
def test_instruct_rows_come_first_and_depend_on_the_instruct_alone(dtype, path):
    from fq3hip.prompt import build_talker_inputs_hip
    from fq3hip.model import FasterQwen3TTS
    cfg, om, eng = _prompt_setup(dtype)
    eng.prefix_cache = object()                                  # on: the builder projects the instruct ids in a call of their own
    m = NS(talker=NS(engine=eng, **vars(om.talker)), config=om.config, generate_speaker_prompt=om.generate_speaker_prompt)
    langs = sorted(cfg.codec_language_id)
    spks = sorted(cfg.spk_id) or [None]

    def build(instruct, text_ids, language, speaker):
        if path == "hip row program":
            return build_talker_inputs_hip(m, text_ids, None, None, 0, language, speaker, True, instruct)[0]
        return FasterQwen3TTS._build_talker_inputs_local(None, m, [text_ids], [None], None, [language], [speaker], True,
                                                         instruct_ids=[instruct])[0]
    ins_a, ins_b = _ids(40, 1), _ids(40, 2)
    a1 = build(ins_a, _ids(20, 3), langs[0], spks[0])
    a2 = build(ins_a, _ids(33, 4), langs[-1], spks[-1])
    b = build(ins_b, _ids(20, 3), langs[0], spks[0])
    none = build(None, _ids(20, 3), langs[0], spks[0])
    key = tuple(int(i) for i in ins_a.reshape(-1))
    assert a1.fq3_prefix == (40, key) and a2.fq3_prefix == (40, key)
    assert a1.shape[1] != a2.shape[1]
    assert torch.equal(a1[0, :40], a2[0, :40])                   # bit for bit
    assert b.fq3_prefix[1] != key and not torch.equal(b[0, :40], a1[0, :40])
    assert getattr(none, "fq3_prefix", None) is None
    # the rows behind the prefix do differ between the two requests (text, speaker, language)
    assert not torch.equal(a1[0, 40:60], a2[0, 40:60])


def test_no_note_for_batches():
    from fq3hip.model import FasterQwen3TTS
    cfg, om, eng = _prompt_setup(torch.float32)
    m = NS(talker=NS(**vars(om.talker)), config=om.config, generate_speaker_prompt=om.generate_speaker_prompt)
    lang = sorted(cfg.codec_language_id)[0]
    tie = FasterQwen3TTS._build_talker_inputs_local(None, m, [_ids(20, 3), _ids(25, 4)], [None, None], None, [lang, lang], [None, None],
                                                    True, instruct_ids=[_ids(40, 1), _ids(40, 1)])[0]
    assert tie.shape[0] == 2 and getattr(tie, "fq3_prefix", None) is None


# ---- server and CLI ---------------------------------------------------------------------------------------------------------
def test_server_and_cli_flags_parse_and_default_to_off():
    from fq3hip import server, cli
    p = server.build_parser()
    assert p.parse_args([]).prefix_cache_rows == 0
    assert p.parse_args(["--prefix-cache-rows", "4096", "--scheduler", "lock"]).prefix_cache_rows == 4096
    c = cli.build_parser()
    base = ["--text", "hi", "--output", "o.wav"]
    assert c.parse_args(["design", "--instruct", "calm"] + base).prefix_cache_rows == 0
    assert c.parse_args(["design", "--instruct", "calm", "--prefix-cache-rows", "512"] + base).prefix_cache_rows == 512
    assert c.parse_args(["custom", "--speaker", "bob", "--prefix-cache-rows", "512"] + base).prefix_cache_rows == 512


def test_health_carries_the_stats_when_on():
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app
    from test_serving_cpu import _ScriptedModel

    class Model(_ScriptedModel):
        def enable_prefix_cache(self, capacity_rows, min_rows=None):
            self.cache_rows = capacity_rows
            return NS(stats=lambda: {"hits": 3, "misses": 1, "blocks_capacity": capacity_rows // 64})

    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "x", "instruct": "a calm low voice"}}
    m = Model()
    client = TestClient(create_app(m, voices, default_voice="alloy", scheduler="lock"))
    assert "prefix_cache" not in client.get("/health").json() and not hasattr(m, "cache_rows")      # off by default
    m = Model()
    client = TestClient(create_app(m, voices, default_voice="alloy", scheduler="lock", prefix_cache_rows=1024))
    assert m.cache_rows == 1024
    assert client.get("/health").json()["prefix_cache"] == {"hits": 3, "misses": 1, "blocks_capacity": 16}
    r = client.post("/v1/audio/speech", json={"model": "tts-1", "input": "hello", "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and m.calls[-1][2]["instruct"] == "a calm low voice"               # the voice's instruct reaches the model
    # the batch scheduler runs on engines of its own: the flag does nothing there
    m = Model()
    client = TestClient(create_app(m, voices, default_voice="alloy", scheduler="batch", prefix_cache_rows=1024,
                                   worker=NS(submit=None, submit_text=None)))
    assert not hasattr(m, "cache_rows") and "prefix_cache" not in client.get("/health").json()
