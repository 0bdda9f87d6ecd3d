#!/usr/bin/env python3
"""Times the prefix KV cache's paths against the plain prefill and writes profiles/prefix_cache.json.

Shapes: the 1.7B and the 0.6B talker dims at full depth, bf16, synthetic weights; a suffix of 128 rows behind a prefix of P rows,
P in {64, 256, 1024, 3968}.  Per P three paths, timed with device events after a warm-up, ALTERNATING within one process, median of
`reps` (>= 5):
  (a) plain     prefill(P + 128)                                  -- the path without the cache
  (b) hit       kv_copy(entry -> engine, P) + prefill_continue(x[P:], P)
  (c) miss      prefill(x[:P], no logits) + kv_copy(engine -> entry, P) + prefill_continue(x[P:], P)
and kv_copy alone, the key-split count S the continuation's attention takes, and max |logits(b) - logits(a)| over max(1, max |logits(a)|).
usage: prefix_cache_probe.py [reps = 7] [sizes = 1p7b,0p6b] [output = profiles/prefix_cache.json]       (development aid; bench.py is the contract)

PACK MODE (`prefix_cache_probe.py pack [reps = 7] [sizes = 1p7b,0p6b] [output = profiles/prefix_cache_batch.json]`): the batch scheduler's
packed admission.  Packs of 8 and 32 requests of one voice, 128 new rows behind P in {64, 256, 1024} cached rows, contexts of one KV pool
with max_seq_len 4096 (the packed rows of one pass are capped by it, as in BatchDecoder._stage_many).  Four paths, alternating, median:
  (a) plain     Fq3Engine.prefill_batch of the whole prompts, in runs of at most max_seq_len rows   -- the path without the cache
  (b) hits      PrefixCache.prefill_pack with the voice cached: n kv_copy + ONE prefill_continue_batch
  (c) miss      PrefixCache.prefill_pack on an empty cache: one prefix prefill + save + n - 1 copies + ONE prefill_continue_batch
  (d) per-prompt (b) with "cont_pack" 0: the continuation's norm / attention launches per prompt instead of the pack kernels"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]
import torch
from fq3hip.config import qwen3_tts_0p6b, qwen3_tts_1p7b
from fq3hip.engine import Fq3Engine
from fq3hip.weights import synth_weights, synth_prompt

SUFFIX = 128
PREFIXES = (64, 256, 1024, 3968)
WS_FLOATS = 8 << 20                    # kPrefillWsFloats of csrc/fq3_prefill.hip


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def splits_of(start, n, heads):
    lib = os.path.join(ROOT, "tools", "microbench", "libprefill_cont_probe.so")
    if not os.path.exists(lib):
        return None
    h = ctypes.CDLL(lib)
    h.cont_probe_splits.argtypes = [ctypes.c_int] * 4 + [ctypes.c_long]
    return int(h.cont_probe_splits(start, n, heads, torch.cuda.get_device_properties(0).multi_processor_count, WS_FLOATS))


def probe(size, reps):
    cfg = qwen3_tts_1p7b() if size == "1p7b" else qwen3_tts_0p6b()
    dt = torch.bfloat16
    W = synth_weights(cfg, 0, dt, parts=("talker", "predictor"))
    Lmax = max(PREFIXES) + SUFFIX
    eng = Fq3Engine(cfg, W, device="cuda", dtype=dt, max_seq_len=Lmax + 8, max_frames=8)
    pool = eng.kv_pool((max(PREFIXES) + 63) // 64)
    entry = eng.spawn_pooled(pool)
    tie = synth_prompt(cfg, Lmax, 4, 0, dtype=dt)[0]
    xall = (tie * 30).to(dt)[0].cuda().contiguous()
    rows = []
    for P in PREFIXES:
        x = xall[:P + SUFFIX].contiguous()
        head, tail = x[:P].contiguous(), x[P:].contiguous()
        entry.kv_release(0)
        eng.prefill(head, want_logits=False)
        entry.kv_copy(eng, P)

        def plain():
            return eng.prefill(x)

        def hit():
            eng.kv_copy(entry, P)
            return eng.prefill_continue(tail, P)

        def miss():
            eng.prefill(head, want_logits=False)
            entry.kv_copy(eng, P)
            return eng.prefill_continue(tail, P)

        def copy():
            eng.kv_copy(entry, P)

        paths = {"plain": plain, "hit": hit, "miss": miss, "kv_copy": copy}
        for fn in paths.values():                  # warm-up (workspaces, code objects)
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        outs = {}
        for _ in range(reps):
            for k, fn in paths.items():            # alternating: every path sees the same clocks and cache state
                t, o = timed(fn)
                ms[k].append(t)
                outs[k] = o
        la, lb = outs["plain"][0].float(), outs["hit"][0].float()
        row = {"P": P, "suffix": SUFFIX, "splits": splits_of(P, SUFFIX, cfg.talker.num_attention_heads),
               **{f"{k}_ms": round(statistics.median(v), 4) for k, v in ms.items()},
               "hit_vs_plain_logits": float((lb - la).abs().max() / max(1.0, float(la.abs().max()))),
               "miss_equals_hit": bool(torch.equal(outs["miss"][0], outs["hit"][0]) and torch.equal(outs["miss"][1], outs["hit"][1]))}
        row["hit_over_plain"] = round(row["hit_ms"] / row["plain_ms"], 4)
        rows.append(row)
        print(f"{size} P={P:5d}: plain {row['plain_ms']:8.3f} ms  hit {row['hit_ms']:8.3f} ms  miss {row['miss_ms']:8.3f} ms  "
              f"kv_copy {row['kv_copy_ms']:.3f} ms  S={row['splits']}  |dlogits| {row['hit_vs_plain_logits']:.2e}  miss==hit {row['miss_equals_hit']}",
              flush=True)
    entry.close(); eng.close(); pool.close()
    return {"layers": cfg.talker.num_hidden_layers, "hidden": cfg.talker.hidden_size, "rows": rows}


PACK_SIZES = (8, 32)
PACK_PREFIXES = (64, 256, 1024)
PACK_MAX_SEQ = 4096


def probe_pack(size, reps):
    from fq3hip.engine import Fq3KvPool
    from fq3hip.prefix_cache import PrefixCache
    cfg = qwen3_tts_1p7b() if size == "1p7b" else qwen3_tts_0p6b()
    dt = torch.bfloat16
    W = synth_weights(cfg, 0, dt, parts=("talker", "predictor"))
    n_max, Lmax = max(PACK_SIZES), max(PACK_PREFIXES) + SUFFIX
    pool = Fq3KvPool(cfg, n_max * ((Lmax + 63) // 64), dtype=dt)
    first = Fq3Engine(cfg, W, device="cuda", dtype=dt, max_seq_len=PACK_MAX_SEQ, max_frames=8, pool=pool)
    engs = [first] + [Fq3Engine(cfg, W, device="cuda", dtype=dt, max_seq_len=PACK_MAX_SEQ, max_frames=8, share=first, pool=pool)
                      for _ in range(n_max - 1)]
    cache = PrefixCache(first, max(PACK_PREFIXES), min_rows=1)
    xall = (synth_prompt(cfg, Lmax, 4, 0, dtype=dt)[0] * 30).to(dt)[0].cuda().contiguous()
    rows = []
    for n in PACK_SIZES:
        es = engs[:n]
        for P in PACK_PREFIXES:
            x = xall[:P + SUFFIX].contiguous()
            xs, pads, notes = [x] * n, [0] * n, [(P, tuple(range(P)))] * n
            runs = PrefixCache._runs(list(range(n)), [P + SUFFIX] * n, PACK_MAX_SEQ)

            def plain():
                out = []
                for r in runs:
                    out += Fq3Engine.prefill_batch([es[i] for i in r], [xs[i] for i in r], [0] * len(r))
                return out

            def hits():
                return cache.prefill_pack(es, xs, pads, notes)

            def miss():
                cache.clear()
                return cache.prefill_pack(es, xs, pads, notes)

            def per_prompt():
                for e in es:
                    e.set_option("cont_pack", 0)
                try:
                    return cache.prefill_pack(es, xs, pads, notes)
                finally:
                    for e in es:
                        e.set_option("cont_pack", 1)

            paths = {"a_plain": plain, "c_miss": miss, "b_hits": hits, "d_per_prompt": per_prompt}      # (c) leaves the entry (b) and (d) use
            for fn in paths.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in paths}
            outs = {}
            for _ in range(reps):
                for k, fn in paths.items():
                    t, o = timed(fn)
                    ms[k].append(t)
                    outs[k] = o
            la, lb = outs["a_plain"][-1][0].float(), outs["b_hits"][-1][0].float()
            row = {"n": n, "P": P, "suffix": SUFFIX, "plain_runs": len(runs), **{f"{k}_ms": round(statistics.median(v), 4) for k, v in ms.items()},
                   "hits_vs_plain_logits": float((lb - la).abs().max() / max(1.0, float(la.abs().max()))),
                   "per_prompt_equals_pack": all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(outs["d_per_prompt"], outs["b_hits"])),
                   "miss_equals_hits": all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(outs["c_miss"], outs["b_hits"]))}
            row["b_over_a"] = round(row["b_hits_ms"] / row["a_plain_ms"], 4)
            row["c_over_a"] = round(row["c_miss_ms"] / row["a_plain_ms"], 4)
            row["d_over_b"] = round(row["d_per_prompt_ms"] / row["b_hits_ms"], 4)
            rows.append(row)
            print(f"{size} n={n:2d} P={P:5d}: (a) plain {row['a_plain_ms']:8.3f} ms in {len(runs)} run(s)  (b) hits {row['b_hits_ms']:8.3f}  (c) miss "
                  f"{row['c_miss_ms']:8.3f}  (d) per-prompt {row['d_per_prompt_ms']:8.3f}  b/a {row['b_over_a']:.3f}  d/b {row['d_over_b']:.3f}  "
                  f"|dlogits| {row['hits_vs_plain_logits']:.2e}  d==b {row['per_prompt_equals_pack']}  c==b {row['miss_equals_hits']}", flush=True)
    torch.cuda.synchronize()
    cache.close()
    for e in reversed(engs):
        e.close()
    pool.close()
    return {"layers": cfg.talker.num_hidden_layers, "hidden": cfg.talker.hidden_size, "max_seq_len": PACK_MAX_SEQ, "rows": rows}


def main_pack(argv):
    reps = max(5, int(argv[0])) if len(argv) > 0 else 7
    sizes = argv[1].split(",") if len(argv) > 1 else ["1p7b", "0p6b"]
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "reps": reps, "timing": "device events, median, paths alternating",
           "paths": {"a": "prefill_batch of the whole prompts", "b": "prefill_pack, all hits", "c": "prefill_pack, one shared miss + hits",
                     "d": "(b) with per-prompt attention launches (cont_pack 0)"},
           "sizes": {s: probe_pack(s, reps) for s in sizes}}
    rows = [r for s in out["sizes"].values() for r in s["rows"]]
    worth = [P for P in PACK_PREFIXES if all(r["b_hits_ms"] < r["a_plain_ms"] for r in rows if r["P"] == P)]
    out["smallest_P_where_hits_beat_plain_on_every_size_and_pack"] = min(worth) if worth else None
    path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "prefix_cache_batch.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {path}")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "pack":
        return main_pack(sys.argv[2:])
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    sizes = sys.argv[2].split(",") if len(sys.argv) > 2 else ["1p7b", "0p6b"]
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "reps": reps, "timing": "device events, median, paths alternating",
           "sizes": {s: probe(s, reps) for s in sizes}}
    worth = [P for P in PREFIXES if all(r["hit_ms"] < r["plain_ms"] for s in out["sizes"].values() for r in s["rows"] if r["P"] == P)]
    out["smallest_P_where_hit_beats_plain_on_every_size"] = min(worth) if worth else None
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "prefix_cache.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
