#!/usr/bin/env python3
"""Measures long-form synthesis (fq3hip/long_form.py) and writes profiles/long_form.json.

(a) The join stage ALONE (fq3_join_*, one launch of join_kernel per push, one workgroup), with HIP events, median of `runs` after a
    warm-up, each run between its own events and the same pushes back to back under one pair: a streaming chunk (12 frames = 23 040
    samples = 96 hops) and a whole 200-frame segment (384 000 samples = 1 600 hops, seven rounds of 256 hops inside the one
    workgroup), once all loud (everything is copied) and once with silent ends (hops are dropped).  Beside each, from the same run and
    stream, the vocoder's time for the same audio -- the streaming-chunk decode (25 context + 12 new frames, the tail produced) and
    the 200-frame decode -- and the join's share of it.
(b) End to end at full depth (0.6B dims, bf16, synthetic weights, x-vector clone, sampling off, every sentence forced to FRAMES
    frames): a text of K = 4, 8, 16 equal sentences,
      long    generate_long_voice_clone_streaming(lanes=K): wall time to the first and to the last audio sample on the host
      serial  the same sentences one after another through generate_voice_clone_streaming -- what a caller has without this feature
    alternating in one process, median of `reps` (>= 5) after one warm-up of each, and the ratios.
usage: long_form_probe.py [reps = 7] [runs = 100] [output = profiles/long_form.json] [frames = 100]      (development aid; bench.py is the contract)

Long form for MANY texts -> profiles/long_form_batch.json:
    long_form_probe.py --group B[,B...] --texts T[,T...] [--reps 3] [--runs 50] [--frames 100] [--output FILE]
(c) --group: B rows of one 8-frame chunk (15 360 samples) pushed into RUNNING streams: one `push_group` (one launch of B workgroups,
    one copy of the B lengths) against B calls of `SegmentJoin.push` (B launches, B synchronisations -- all a caller had before).
    Wall clock around `runs` calls, the reading of the lengths included (it is part of either call); the sides alternate, median of
    `reps` alternations.  Once with the rows left on the device, once with the rows on the host (`push_host` per row against the
    group's rows gathered and copied once).
(d) --texts: T texts of 4 sentences of `frames` frames at lanes 16: `generate_long_voice_clone_batch[_streaming]` against the same
    texts one after another through `generate_long_voice_clone[_streaming]` at the same lanes: the time to every text's last sample
    and, in the streaming form, to each text's first audio, from the start of the whole job."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]
import torch
from fq3hip.long_form import LongFormSpec, SegmentJoin

SAMPLES_PER_FRAME = 1920
CHUNK_FRAMES, SEGMENT_FRAMES, CONTEXT_FRAMES = 12, 200, 25
SENTENCES = (4, 8, 16)


def timed(fn, runs, warmup=10):
    """(median ms of `runs` single calls, each between its own events; ms per call of `runs` calls between one pair)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for e0, e1 in pairs:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    single = statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(runs):
        fn()
    e1.record(); torch.cuda.synchronize()
    return single, e0.elapsed_time(e1) / runs


def build_model(max_seq_len, max_frames):
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.weights import synth_weights
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("talker", "predictor", "codec", "text"), codec_normalized=True)
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.bfloat16, max_seq_len=max_seq_len, max_frames=max_frames,
                                    codec_max_frames=max(256, SEGMENT_FRAMES + 8))
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    g = torch.Generator().manual_seed(5)
    vcp = dict(ref_code=[None], ref_spk_embedding=[torch.randn(cfg.talker.hidden_size, generator=g).to(torch.bfloat16).cuda()],
               x_vector_only_mode=[True], icl_mode=[False])
    return cfg, m, vcp


def probe_join(m, cfg, runs):
    tok = m.model.model.speech_tokenizer
    g = torch.Generator().manual_seed(3)
    spec = LongFormSpec()
    rows = []
    for name, frames in (("streaming chunk, 12 frames", CHUNK_FRAMES), ("segment, 200 frames", SEGMENT_FRAMES)):
        n = frames * SAMPLES_PER_FRAME
        if frames == CHUNK_FRAMES:
            codes = torch.randint(0, cfg.codec.codebook_size, (CONTEXT_FRAMES + frames, 16), generator=g).cuda()
            first = tok.num_samples_total(CONTEXT_FRAMES + frames) - n
        else:
            codes = torch.randint(0, cfg.codec.codebook_size, (frames, 16), generator=g).cuda()
            first = 0
        voc_single, voc_stream = timed(lambda: tok.decode_tensor(codes, first), runs)
        loud = (torch.rand(n, generator=g) * 1.6 - 0.8).cuda()
        ends = loud.clone()
        ends[: n // 4] *= 1e-4                                      # a quarter of silence in front, a quarter behind
        ends[n - n // 4:] *= 1e-4
        for kind, pcm in (("all loud", loud), ("silent ends", ends)):
            join = SegmentJoin.from_spec(spec, 24000, "cuda")
            out = torch.empty(join.bound(n, 0), dtype=torch.float32, device="cuda")
            n_dev = torch.zeros(1, dtype=torch.int64, device="cuda")

            def one():
                join.reset()                                        # host only
                join.push_into(pcm, 2, 0, out, n_dev)               # the launch alone, into a buffer that exists
            single, stream = timed(one, runs)
            rows.append({"input": name, "content": kind, "n_in": n, "hops": n // 240, "n_out": int(n_dev.item()),
                         "join_median_single_push_ms": round(single, 4), "join_back_to_back_per_push_ms": round(stream, 4),
                         "vocoder_median_single_call_ms": round(voc_single, 4), "vocoder_back_to_back_per_call_ms": round(voc_stream, 4),
                         "join_share_of_vocoder_back_to_back": round(stream / voc_stream, 4),
                         "join_GB_per_s_back_to_back": round((n + int(n_dev.item())) * 4 / (stream * 1e-3) / 1e9, 2)})
            print(rows[-1], flush=True)
    return rows


def run_stream(gen):
    """-> (seconds to the first audio sample, seconds to the last, samples)"""
    t0 = time.perf_counter()
    first, total = None, 0
    for audio, _sr, _tm in gen:
        if first is None and len(audio) > 0:
            first = time.perf_counter() - t0
        total += len(audio)
    return first, time.perf_counter() - t0, total


def probe_end_to_end(m, vcp, reps, frames):
    kw = dict(language="English", voice_clone_prompt=vcp, do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0,
              max_new_tokens=frames, min_new_tokens=frames, non_streaming_mode=False)
    spec = LongFormSpec(max_chars=64)
    rows = []
    for K in SENTENCES:
        sentences = [f"This is sentence number {i + 1:02d} of the long form probe." for i in range(K)]
        text = " ".join(sentences)
        assert [s.text for s in spec.split(text)] == sentences

        def long():
            return run_stream(m.generate_long_voice_clone_streaming(text, chunk_size=CHUNK_FRAMES, lanes=K, long_form=spec, **kw))

        def serial():
            t0 = time.perf_counter()
            first, total = None, 0
            for s in sentences:
                f, _last, n = run_stream(m.generate_voice_clone_streaming(text=s, chunk_size=CHUNK_FRAMES, **kw))
                if first is None:
                    first = f
                total += n
            return first, time.perf_counter() - t0, total

        paths = {"long": long, "serial": serial}
        for fn in paths.values():                                   # warm-up: contexts, graphs, workspaces, code objects
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in paths}
        for _ in range(reps):
            for k, fn in paths.items():                             # alternating: every path sees the same clocks and neighbours
                res[k].append(fn())
                torch.cuda.synchronize()
        row = {"sentences": K, "frames_per_sentence": frames, "lanes": K, "chunk_frames": CHUNK_FRAMES}
        for k, v in res.items():
            row[f"{k}_first_audio_ms"] = round(1000 * statistics.median(x[0] for x in v), 2)
            row[f"{k}_last_audio_ms"] = round(1000 * statistics.median(x[1] for x in v), 2)
            row[f"{k}_last_audio_ms_min_max"] = [round(1000 * min(x[1] for x in v), 2), round(1000 * max(x[1] for x in v), 2)]
            row[f"{k}_samples"] = v[0][2]
        row["serial_over_long_last_audio"] = round(row["serial_last_audio_ms"] / row["long_last_audio_ms"], 3)
        row["long_over_serial_first_audio"] = round(row["long_first_audio_ms"] / row["serial_first_audio_ms"], 3)
        row["ms_per_frame_long"] = round(row["long_last_audio_ms"] / frames, 3)
        row["ms_per_frame_serial"] = round(row["serial_last_audio_ms"] / (K * frames), 3)
        rows.append(row)
        print(row, flush=True)
    return rows


def probe_group(sizes, reps, runs):
    """(c) in the module text"""
    from fq3hip import long_form as lf
    g = torch.Generator().manual_seed(11)
    n = 8 * SAMPLES_PER_FRAME
    spec = LongFormSpec()
    rows = []
    for B in sizes:
        joins = [SegmentJoin.from_spec(spec, 24000, "cuda") for _ in range(B)]
        chunks = [(torch.rand(n, generator=g) * 1.6 - 0.8).cuda() for _ in range(B)]
        zeros = [0] * B
        for j, x in zip(joins, chunks):                             # running streams
            j.push(x)

        sides = {
            "group_device": lambda: lf.push_group(joins, chunks, zeros, zeros),
            "single_device": lambda: [j.push(x) for j, x in zip(joins, chunks)],
            "group_host": lambda: torch.cat(lf.push_group(joins, chunks, zeros, zeros)).cpu(),
            "single_host": lambda: [j.push_host(x) for j, x in zip(joins, chunks)],
        }
        for fn in sides.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        res = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():                             # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(runs):
                    fn()
                torch.cuda.synchronize()
                res[k].append(1000 * (time.perf_counter() - t0) / runs)
        row = {"rows": B, "samples_per_row": n, "hops_per_row": n // 240}
        for k, v in res.items():
            row[f"{k}_ms"] = round(statistics.median(v), 4)
            row[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["single_over_group_device"] = round(row["single_device_ms"] / row["group_device_ms"], 2)
        row["single_over_group_host"] = round(row["single_host_ms"] / row["group_host_ms"], 2)
        rows.append(row)
        print(row, flush=True)
    return rows


def probe_texts(m, vcp, counts, reps, frames, lanes=16):
    """(d) in the module text"""
    kw = dict(language="English", voice_clone_prompt=vcp, do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0,
              max_new_tokens=frames, min_new_tokens=frames, non_streaming_mode=False, lanes=lanes, long_form=LongFormSpec(max_chars=64))
    rows = []
    for T in counts:
        texts = [" ".join(f"This is sentence {i + 1} of text number {t + 1:02d} in the probe." for i in range(4)) for t in range(T)]
        assert all(len(kw["long_form"].split(x)) == 4 for x in texts)

        def batch_stream():
            t0 = time.perf_counter()
            first, last = [None] * T, [None] * T
            for t, a, _sr, _info in m.generate_long_voice_clone_batch_streaming(texts, chunk_size=CHUNK_FRAMES, **kw):
                now = time.perf_counter() - t0
                if first[t] is None and len(a) > 0:
                    first[t] = now
                last[t] = now
            return first, last

        def serial_stream():
            t0 = time.perf_counter()
            first, last = [None] * T, [None] * T
            for t, x in enumerate(texts):
                for a, _sr, _info in m.generate_long_voice_clone_streaming(x, chunk_size=CHUNK_FRAMES, **kw):
                    now = time.perf_counter() - t0
                    if first[t] is None and len(a) > 0:
                        first[t] = now
                    last[t] = now
            return first, last

        def batch_full():
            t0 = time.perf_counter()
            m.generate_long_voice_clone_batch(texts, **kw)
            return time.perf_counter() - t0

        def serial_full():
            t0 = time.perf_counter()
            for x in texts:
                m.generate_long_voice_clone(x, **kw)
            return time.perf_counter() - t0

        paths = {"batch_stream": batch_stream, "serial_stream": serial_stream, "batch_full": batch_full, "serial_full": serial_full}
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        res = {k: [] for k in paths}
        for _ in range(reps):
            for k, fn in paths.items():
                res[k].append(fn())
                torch.cuda.synchronize()
        med = lambda xs: round(1000 * statistics.median(xs), 2)     # noqa: E731
        row = {"texts": T, "sentences_per_text": 4, "frames_per_sentence": frames, "lanes": lanes, "chunk_frames": CHUNK_FRAMES}
        for k in ("batch_stream", "serial_stream"):
            row[f"{k}_last_sample_of_every_text_ms"] = med([max(l) for _f, l in res[k]])
            row[f"{k}_last_sample_per_text_ms"] = [med([l[t] for _f, l in res[k]]) for t in range(T)]
            row[f"{k}_first_audio_per_text_ms"] = [med([f[t] for f, _l in res[k]]) for t in range(T)]
        for k in ("batch_full", "serial_full"):
            row[f"{k}_ms"] = med(res[k])
            row[f"{k}_ms_min_max"] = [round(1000 * min(res[k]), 2), round(1000 * max(res[k]), 2)]
        row["serial_over_batch_stream_last_sample"] = round(row["serial_stream_last_sample_of_every_text_ms"] / row["batch_stream_last_sample_of_every_text_ms"], 3)
        row["serial_over_batch_full"] = round(row["serial_full_ms"] / row["batch_full_ms"], 3)
        rows.append(row)
        print(row, flush=True)
    return rows


def main_batch(argv):
    import argparse
    p = argparse.ArgumentParser(description="long form for many texts: the group push and the many-text entry points")
    p.add_argument("--group", default="", help="rows of the group push, e.g. 1,8,32")
    p.add_argument("--texts", default="", help="numbers of texts, e.g. 4,16")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--runs", type=int, default=50)
    p.add_argument("--frames", type=int, default=100)
    p.add_argument("--output", default=os.path.join(ROOT, "profiles", "long_form_batch.json"))
    a = p.parse_args(argv)
    reps = max(3, a.reps)
    sizes = [int(x) for x in a.group.split(",") if x]
    counts = [int(x) for x in a.texts.split(",") if x]
    out = {"device": torch.cuda.get_device_name(0), "reps": reps, "runs": a.runs,
           "timing": "wall clock on the host; the sides alternate in one process, median of `reps` alternations after a warm-up of each"}
    if sizes:
        out["group_push"] = probe_group(sizes, reps, a.runs)
    if counts:
        _cfg, m, vcp = build_model(max_seq_len=512, max_frames=max(256, a.frames + 8))
        out.update(dtype="bf16", model="0.6B dims, full depth, synthetic weights", many_texts=probe_texts(m, vcp, counts, reps, a.frames))
    out["not_measured"] = ["long form under the server's batch scheduler: not offered",
                           "texts of unequal length, and more texts than 16",
                           "real voices: threshold, pauses and max_chars are untuned defaults"]
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.output}")


def main():
    if any(x.startswith("--") for x in sys.argv[1:]):
        return main_batch(sys.argv[1:])
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    runs = max(50, int(sys.argv[2])) if len(sys.argv) > 2 else 100
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "long_form.json")
    frames = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    cfg, m, vcp = build_model(max_seq_len=512, max_frames=max(256, frames + 8))
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "model": "0.6B dims, full depth, synthetic weights", "reps": reps, "runs": runs,
           "join_timing": "device events; median of single pushes, and pushes back to back under one pair",
           "end_to_end_timing": "wall clock to the first / last audio sample on the host, median, paths alternating in one process",
           "join_defaults": {"threshold": 0.005, "lead_hops": 2, "tail_hops": 5, "hold_hops": 100},
           "join": probe_join(m, cfg, runs), "end_to_end": probe_end_to_end(m, vcp, reps, frames),
           "not_measured": ["the three-launch form of a whole-utterance push (peaks over a grid, decision, copy over a grid): not built",
                            "real voices: threshold, pauses and max_chars are untuned defaults",
                            "where the time of a K-lane run goes beyond the per-frame figure (admission, vocoder groups, host waits)"]}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
