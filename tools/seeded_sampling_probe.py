#!/usr/bin/env python3
"""Times the seeded noise fill against torch's ``exponential_`` and the seeded decode loop against the unseeded one; writes
profiles/seeded_sampling.json.

Device events, median of `reps` (default 7) after a warm-up, the paths ALTERNATING within one process:
  (a) one lane's refill at the 0.6B dims, a 64-frame ring (64 x (3072 + 15 x 2048) elements), bf16 and fp32:
      torch's two ``exponential_`` calls against one ``Fq3Engine.noise_fill``
  (b) 128 lanes' refill: 256 ``exponential_`` calls against one ``Fq3Engine.noise_fill_many`` (four launches of 32 rings)
  (c) single-stream ``fast_generate`` of 200 frames at the 0.6B dims (full depth, bf16, synthetic weights, sampled), seeded against
      unseeded, three alternating runs each: ms per frame from the loop's own timing
usage: seeded_sampling_probe.py [reps = 7] [output = profiles/seeded_sampling.json]       (development aid; bench.py is the contract)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]
import torch
from fq3hip.config import qwen3_tts_0p6b
from fq3hip.engine import Fq3Engine
from fq3hip.generate import NOISE_RING, fast_generate
from fq3hip.weights import synth_prompt, synth_weights

LANES = 128


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(paths, reps):
    """{name: fn} -> {name: median ms}; one warm-up each, then the paths in turn, `reps` times."""
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            ms[k].append(timed(fn))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def refill_probe(cfg, dtype, reps):
    """Shallow contexts (the fill reads only the vocabularies and the dtype from the config)."""
    shallow = qwen3_tts_0p6b()
    shallow.talker.num_hidden_layers, shallow.predictor.num_hidden_layers = 1, 1
    W = synth_weights(shallow, 0, dtype, parts=("talker", "predictor"))
    eng = Fq3Engine(shallow, W, device="cuda", dtype=dtype, max_seq_len=64, max_frames=8)
    V, G1, Vp = cfg.talker.vocab_size, cfg.num_code_groups - 1, cfg.predictor.vocab_size
    rings = [(eng.new(NOISE_RING, V), eng.new(NOISE_RING, G1, Vp)) for _ in range(LANES)]
    tn, pn = rings[0]

    def torch_one():
        tn.exponential_(1)
        pn.exponential_(1)

    def torch_many():
        for t, p in rings:
            t.exponential_(1)
            p.exponential_(1)
    items = [(eng, t, p, 1000 + i, 64 * (i % 5), None) for i, (t, p) in enumerate(rings)]
    one = alternate({"torch_exponential_x2": torch_one, "noise_fill": lambda: eng.noise_fill(tn, pn, 1234, 64)}, reps)
    many = alternate({"torch_exponential_x256": torch_many, "noise_fill_many": lambda: Fq3Engine.noise_fill_many(items, NOISE_RING)}, reps)
    bytes_per_ring = NOISE_RING * (V + G1 * Vp) * (2 if dtype == torch.bfloat16 else 4)
    return {"ring_elements": NOISE_RING * (V + G1 * Vp), "ring_bytes": bytes_per_ring, "one_lane_ms": one, f"{LANES}_lanes_ms": many}


def decode_probe(cfg, frames=200, runs=3):
    from fq3hip.model import FasterQwen3TTS
    dt = torch.bfloat16
    W = synth_weights(cfg, 0, dt, parts=("talker", "predictor", "text"))
    model = FasterQwen3TTS.from_weights(cfg, W, device="cuda:0", dtype=dt, max_seq_len=512, max_frames=256)
    tie, tam, tth, tpe, _ = synth_prompt(cfg, 100, 32, 0, dtype=dt)
    m = model.model.model
    kw = dict(max_new_tokens=frames, min_new_tokens=frames, temperature=0.9, top_k=50, top_p=1.0, do_sample=True, repetition_penalty=1.05)

    def run(seed):
        codes, t = fast_generate(m.talker, tie.cuda(), tam.cuda(), tth.cuda(), tpe.cuda(), m.config.talker_config, model.predictor_graph,
                                 model.talker_graph, seed=seed, **kw)
        assert codes is not None and codes.shape[0] == frames
        return t["ms_per_step"], codes
    run(None), run(1)                                            # warm-up: graph capture, allocator
    out = {"unseeded_ms_per_frame": [], "seeded_ms_per_frame": []}
    first = None
    for i in range(runs):
        out["unseeded_ms_per_frame"].append(round(run(None)[0], 4))
        ms, codes = run(20240607)
        out["seeded_ms_per_frame"].append(round(ms, 4))
        first = codes if first is None else first
        assert torch.equal(codes, first), "the same seed gave different codes"
    u, s = statistics.median(out["unseeded_ms_per_frame"]), statistics.median(out["seeded_ms_per_frame"])
    out.update(frames=frames, unseeded_median=u, seeded_median=s, seeded_over_unseeded=round(s / u, 4))
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "seeded_sampling.json")
    cfg = qwen3_tts_0p6b()
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "timer": "device events, median, paths alternating in one process",
           "refill": {"bf16": refill_probe(cfg, torch.bfloat16, reps), "fp32": refill_probe(cfg, torch.float32, reps)},
           "fast_generate_0p6b_bf16": decode_probe(cfg)}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
