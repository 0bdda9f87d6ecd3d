#!/usr/bin/env python3
"""Times the prefix KV cache's paths against the plain prefill and writes profiles/prefix_cache.json.

Shapes: the 1.7B and the 0.6B talker dims at full depth, bf16, synthetic weights; a suffix of 128 rows behind a prefix of P rows,
P in {64, 256, 1024, 3968}.  Per P three paths, timed with device events after a warm-up, ALTERNATING within one process, median of
`reps` (>= 5):
  (a) plain     prefill(P + 128)                                  -- the path without the cache
  (b) hit       kv_copy(entry -> engine, P) + prefill_continue(x[P:], P)
  (c) miss      prefill(x[:P], no logits) + kv_copy(engine -> entry, P) + prefill_continue(x[P:], P)
and kv_copy alone, the key-split count S the continuation's attention takes, and max |logits(b) - logits(a)| over max(1, max |logits(a)|).
usage: prefix_cache_probe.py [reps = 7] [sizes = 1p7b,0p6b] [output = profiles/prefix_cache.json]       (development aid; bench.py is the contract)"""
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


def main():
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
