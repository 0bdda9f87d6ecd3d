#!/usr/bin/env python3
"""Times the loudness stage (fq3hip/loudness.py: fq3_loud_push, one lane per 100 ms hop; fq3_loud_finish, one workgroup;
fq3_loud_apply) ALONE, with HIP events, on a 370-frame utterance (710 400 samples at 24 kHz) and on a streaming chunk's worth
(8 frames, 15 360 samples), each beside the bf16x2 vocoder's time for the same audio in the same run and on the same stream: the full
decode of 370 frames, and the streaming-chunk decode (25 context + 8 new frames, the tail of 8 frames produced).  Stage and vocoder
ALTERNATE: every repeat times push, finish, apply, the three together and then the vocoder, each between its own event pair; the
figures are the medians over the repeats after a warm-up.  An event pair around ONE short launch includes what starting it costs, which
launches issued back to back hide: the three together can therefore read below push alone.  The share is taken from the SUM of the
three parts, the larger figure.  Also the worst hop-energy error of the device against the float64 measure
on the GPU tests' signal (tests/_loud_ref.py), next to the float32 emulation's.  Writes profiles/loudness_stage.json.
usage: loudness_probe.py [runs=60] [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from fq3hip import loudness as L

SAMPLES_PER_FRAME = 1920


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    return e0, e1


def alternate(fns, runs, warmup=8):
    """name -> median ms over `runs` repeats; within a repeat every fn runs once, in order, between its own events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    marks = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            marks[k].append(event_ms(fn))
        torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in marks.items()}


def speech_like(n, g):
    t = torch.arange(n, dtype=torch.float64) / 24000.0
    voiced = sum(0.25 / h * torch.sin(2 * torch.pi * 140.0 * h * t) for h in range(1, 9)) * torch.exp(-3.0 * (t % 0.16))
    return (voiced + 0.003 * torch.randn(n, generator=g)).float().cuda()


def device_error():
    import _loud_ref as R
    rows = []
    for rate in (24000, 8000, 44100):
        x, d = R.burst_signal(rate), L.design(rate)
        e64 = R.hop_energies64(x, rate)
        floor = R.ABS_GATE_POWER * d.H
        loud = e64 >= floor

        def worst(e):
            return float(np.where(loud, np.abs(e - e64) / np.maximum(e64, floor), np.abs(e - e64) / floor).max())
        m = L.LoudnessMeter(None, rate, "cuda")
        m.push(torch.from_numpy(x.copy()).cuda(), final=True)
        rows.append({"rate": rate, "hops": int(len(e64)), "loud_hops": int(loud.sum()),
                     "worst_hop_error_device": worst(m.hops().astype(np.float64) / R.SCALE),
                     "worst_hop_error_float32_emulation": worst(R.emulate_hops(x, d.coef32, d.H).astype(np.float64) / R.SCALE),
                     "device_lufs": round(m.stats().lufs, 5), "float64_lufs": round(R.measure64(x, rate), 5)})
    return rows


def main():
    runs = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 60
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "loudness_stage.json")
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    g = torch.Generator().manual_seed(3)
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "in_rate": 24000, "stage": [], "notes": [],
           "method": "HIP events around each call, stage and vocoder alternating inside every repeat, medians"}
    cases = (("utterance, 370 frames", 370, torch.randint(0, cfg.codec.codebook_size, (370, 16), generator=g).cuda(), 0,
              "full decode of 370 frames"),
             ("streaming chunk, 8 frames", 8, torch.randint(0, cfg.codec.codebook_size, (33, 16), generator=g).cuda(),
              tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME, "chunk decode: 25 context + 8 new frames, the tail of 8 produced"))
    for name, frames, codes, first, what in cases:
        n = frames * SAMPLES_PER_FRAME
        pcm = speech_like(n, g)
        out = torch.empty_like(pcm)
        meter = L.LoudnessMeter(None, 24000, "cuda")

        def push():
            meter.reset()
            meter.push(pcm, final=True)

        def finish():
            return meter.finish()

        def apply():
            return L.apply_gain(pcm, L.gain_of(meter._stats), out=out)

        def all_three():
            push(); finish(); apply()
        push(); finish()
        t = alternate({"push": push, "finish": finish, "apply": apply, "all": all_three,
                       "vocoder": lambda: tok.decode_tensor(codes, first)}, runs)
        res["stage"].append({"input": name, "n_in": n, "hops": n // 2400, "push_workgroups": -(-(n // 2400) // 64) + 1,
                             "push_ms": round(t["push"], 4), "finish_ms": round(t["finish"], 4), "apply_ms": round(t["apply"], 4),
                             "sum_of_parts_ms": round(t["push"] + t["finish"] + t["apply"], 4),
                             "push_finish_apply_back_to_back_ms": round(t["all"], 4), "vocoder": what, "vocoder_ms": round(t["vocoder"], 4),
                             "share_of_vocoder": round((t["push"] + t["finish"] + t["apply"]) / t["vocoder"], 5)})
    for r in res["stage"]:
        res["notes"].append(f"{r['input']}: measure + scale takes {100 * r['share_of_vocoder']:.2f} % of the vocoder's time for the same audio"
                            + ("" if r["share_of_vocoder"] <= 0.05 else " -- ABOVE 5 %"))
    res["notes"].append("share_of_vocoder = sum_of_parts_ms / vocoder_ms; push_finish_apply_back_to_back_ms times the three launches between ONE "
                        "event pair and may read below push_ms alone: a pair around a single short launch includes its start-up")
    res["hop_energy_error"] = device_error()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
