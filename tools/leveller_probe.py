#!/usr/bin/env python3
"""Times the leveller stage (fq3hip/leveller.py: fq3_level_push = the meter's launch, the target launch, the multiply) ALONE, with HIP
events, on a 370-frame utterance (710 400 samples at 24 kHz, one final push into a reset object) and on a streaming chunk's worth
(8 frames, 15 360 samples, one non-final push into a stream that is already running, as a streaming vocoder issues it), each beside
the bf16x2 vocoder's time for the same audio in the same run and on the same stream.  Stage and vocoder ALTERNATE: every repeat times
the whole push, then its parts -- the meter's push on a meter of its own (the launch the leveller makes first), and the plain gain
multiply ``fq3_loud_apply`` as the yardstick of the ramped multiply -- and then the vocoder, each between its own event pair; medians
over the repeats after a warm-up.  The two new launches have no entry point of their own: what they add is reported as the whole push
minus the meter's push.  Also p50 time to first audio of one streaming entry point (``generate_custom_voice_streaming`` on the
synthetic 0.6B model, chunks of 8 frames) with and without the ``leveller()`` context, in alternating runs.  Writes
profiles/leveller_stage.json; a ``bench`` section already in that file (written by the benchmark comparison) is kept.
With --group N: the stage of a lock-step GROUP -- N rows, one streaming chunk each (8 frames, 15 360 samples at 24 kHz), pushed into N
streams that are already running -- through ``leveller.push_group`` (at most THREE launches: the meters', the targets', the multiplies')
and through N single pushes (three launches a row: the path of the batch before the group form) IN THE SAME PROCESS, alternating, three
rounds of 40 repeats after a warm-up, HIP events around each call (the host side of the call included), medians; beside them the
bf16x2 vocoder's windowed chunk decode of the same N rows (``decode_tensor_batch``).  ``limiter_probe.py --group N`` does the same for
the limiter through ``group_probe`` below.  Both write their section of profiles/level_group.json and keep the others.
usage: leveller_probe.py [--group N] [runs=100] [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from fq3hip import leveller as M
from fq3hip import loudness as L
from loudness_probe import SAMPLES_PER_FRAME, alternate, speech_like


def ttfa(runs):
    """p50 ms from the call to the first chunk, with and without the context, alternating"""
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = qwen3_tts_0p6b()
    cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "0b6"
    cfg.spk_id, cfg.spk_is_dialect = {"synthetic": cfg.talker.vocab_size - 1024 + 300}, {"synthetic": False}
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("talker", "predictor", "codec", "text"), codec_normalized=True)
    model = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.bfloat16, max_seq_len=2048)
    text = "The quick brown fox jumps over the lazy dog, and then it rests beside the quiet river for a while."
    kw = dict(chunk_size=8, non_streaming_mode=False, max_new_tokens=40, min_new_tokens=40)

    def first_chunk():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen = model.generate_custom_voice_streaming(text, "synthetic", "English", **kw)
        next(gen)
        ms = (time.perf_counter() - t0) * 1e3
        for _ in gen:
            pass
        return ms
    marks = {"plain": [], "levelled": []}
    for i in range(runs + 3):
        with model.seeded(i):
            a = first_chunk()
            with model.leveller():
                b = first_chunk()
        if i >= 3:                                                    # (warm-up: graph capture, pools)
            marks["plain"].append(a); marks["levelled"].append(b)
    return {"entry_point": "generate_custom_voice_streaming, synthetic 0.6B, chunk_size 8", "runs": runs,
            "p50_ttfa_ms_plain": round(statistics.median(marks["plain"]), 3), "p50_ttfa_ms_levelled": round(statistics.median(marks["levelled"]), 3),
            "min_ttfa_ms_plain": round(min(marks["plain"]), 3), "min_ttfa_ms_levelled": round(min(marks["levelled"]), 3)}


def main():
    runs = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 100
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "leveller_stage.json")
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    g = torch.Generator().manual_seed(3)
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    spec = M.LevelSpec()
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "in_rate": 24000, "spec": {k: getattr(spec, k) for k in spec.__dataclass_fields__},
           "stage": [], "notes": [], "method": "HIP events around each call, stage, parts and vocoder alternating inside every repeat, medians"}
    cases = (("utterance, 370 frames", 370, torch.randint(0, cfg.codec.codebook_size, (370, 16), generator=g).cuda(), 0,
              "full decode of 370 frames", True),
             ("streaming chunk, 8 frames", 8, torch.randint(0, cfg.codec.codebook_size, (33, 16), generator=g).cuda(),
              tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME, "chunk decode: 25 context + 8 new frames, the tail of 8 produced", False))
    for name, frames, codes, first, what, whole in cases:
        n = frames * SAMPLES_PER_FRAME
        pcm = speech_like(n, g)
        out = torch.empty_like(pcm)
        lev = M.Leveller(spec, 24000, "cuda", capacity_hops=1 << 16)
        meter = L.LoudnessMeter(spec.loudness, 24000, "cuda", capacity_hops=1 << 16)
        one = torch.ones(1, device="cuda")
        if not whole:
            lev.push(speech_like(40 * SAMPLES_PER_FRAME, g))          # a stream that is running: 32 hops measured, the gain off its start
            meter.push(speech_like(40 * SAMPLES_PER_FRAME, g))

        def push():
            if whole:
                lev.reset()
            elif lev.n_in + n > 60000 * 2400:
                lev.reset()
            lev.push(pcm, final=whole, out=out)

        def meter_push():
            if whole or meter.n_in + n > 60000 * 2400:
                meter.reset()
            meter.push(pcm, final=whole)
        t = alternate({"push": push, "meter_push": meter_push, "plain_multiply": lambda: L.apply_gain(pcm, one, out=out),
                       "vocoder": lambda: tok.decode_tensor(codes, first)}, runs)
        hops_entered = n // 2400 + (1 if whole else 0)
        res["stage"].append({"input": name, "n_in": n, "hops_entered": hops_entered, "apply_workgroups": -(-n // 4096),
                             "push_ms": round(t["push"], 4), "meter_push_ms": round(t["meter_push"], 4),
                             "target_and_multiply_ms": round(t["push"] - t["meter_push"], 4), "plain_multiply_ms": round(t["plain_multiply"], 4),
                             "vocoder": what, "vocoder_ms": round(t["vocoder"], 4), "share_of_vocoder": round(t["push"] / t["vocoder"], 5)})
    for r in res["stage"]:
        res["notes"].append(f"{r['input']}: the stage takes {100 * r['share_of_vocoder']:.2f} % of the vocoder's time for the same audio; "
                            f"the meter's launch is {100 * r['meter_push_ms'] / r['push_ms']:.0f} % of it")
    res["notes"].append("target_and_multiply_ms = push_ms - meter_push_ms (the two new launches have no entry point of their own); "
                        "plain_multiply_ms is fq3_loud_apply over the same samples, between its own event pair")
    res["ttfa"] = ttfa(max(10, runs // 5))
    try:
        with open(out_path) as f:
            old = json.load(f)
        if "bench" in old:
            res["bench"] = old["bench"]
    except (OSError, ValueError):
        pass
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


def group_probe(kind, N, argv):
    """``kind`` = "leveller" | "limiter": N rows of one chunk as a group call and as N single pushes -> the section of level_group.json"""
    from fq3hip import limiter as LM
    runs = max(20, int(argv[0])) if argv else 40
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "level_group.json")
    g = torch.Generator().manual_seed(3)
    n = 8 * SAMPLES_PER_FRAME
    rows = torch.stack([speech_like(n, g) * (0.5 + 1.5 * b / N) for b in range(N)]).contiguous()       # (the louder rows pass the limiter's ceiling)
    outs = torch.empty_like(rows)
    if kind == "leveller":
        stages = [M.Leveller(M.LevelSpec(), 24000, "cuda", capacity_hops=1 << 15) for _ in range(N)]
        group = lambda: M.push_group(stages, list(rows), [False] * N, outs=list(outs))                  # noqa: E731
        singles = lambda: [st.push(rows[b], False, out=outs[b]) for b, st in enumerate(stages)]         # noqa: E731
        launches = {"push_group": 3 * -(-N // M.GROUP_MAX), "single pushes": 3 * N}
    else:
        stages = [LM.Limiter(LM.LimiterSpec(), 24000, "cuda") for _ in range(N)]
        group = lambda: LM.push_group(stages, list(rows), [False] * N)                                  # noqa: E731
        singles = lambda: [st.push(rows[b], False) for b, st in enumerate(stages)]                      # noqa: E731
        launches = {"push_group": -(-N // LM.GROUP_MAX), "single pushes": N}
    for st in stages:
        st.push(speech_like(40 * SAMPLES_PER_FRAME, g))               # streams that are running: 32 hops measured, the limiter's history full
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    codes = torch.randint(0, cfg.codec.codebook_size, (N, 33, 16), generator=g).cuda()
    first = tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME
    cases = {"push_group": group, f"{N} single pushes": singles, "vocoder decode_tensor_batch": lambda: tok.decode_tensor_batch(codes, first)}

    def events(fn):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
        for e0, e1 in pairs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in pairs]
    for fn in cases.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _round in range(3):                                           # alternating: the forms see the same machine
        for k, fn in cases.items():
            samples[k].append(events(fn))
    res = {"device": torch.cuda.get_device_name(0), "stage": kind, "rows": N, "runs_per_round": runs, "rounds": 3, "warmup": 10, "in_rate": 24000,
           "n_in_per_row": n, "launches": launches,
           "unit": "ms per group of rows, device events around the call (host side included): median over all repeats; per_round: each alternating round's median",
           "ms": {k: {"median": round(statistics.median(v for r in rs for v in r), 4), "per_round": [round(statistics.median(r), 4) for r in rs],
                      "min": round(min(v for r in rs for v in r), 4)} for k, rs in samples.items()}}
    gd, sd, vd = (res["ms"][k]["median"] for k in cases)
    res["notes"] = [f"the group call takes {gd:.3f} ms, the {N} single pushes {sd:.3f} ms: " +
                    (f"{sd / gd:.2f}x faster" if gd < sd else f"NOT faster ({gd / sd:.2f}x the singles' time)"),
                    f"the vocoder's chunk decode of the same {N} rows takes {vd:.3f} ms: the group call is {gd / vd:.3f} of it, the single pushes {sd / vd:.3f}"]
    try:
        with open(out_path) as f:
            whole = json.load(f)
    except (OSError, ValueError):
        whole = {}
    whole[f"{kind}_rows_{N}"] = res
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if "--group" in sys.argv[1:]:
        _i = sys.argv.index("--group")
        group_probe("leveller", int(sys.argv[_i + 1]), sys.argv[1:_i] + sys.argv[_i + 2:])
    else:
        main()
