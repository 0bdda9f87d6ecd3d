#!/usr/bin/env python3
"""Incremental text in the lock-step batch, measured (record, do not gate): profiles/text_stream_batch.json.

``--lanes N`` text streams on the synthetic 0.6B CustomVoice model (bench.py's model, chunk size and sampling), all in ONE run:

(a) one ``fq3_batch_text_append`` of N single ids against N ``fq3_decode_text_append`` calls (the single-lane path, unchanged): time on
    the stream (events around the calls) and host time of the calls;
(b) wall milliseconds per lock-step frame of N text-fed utterances whose text is never late (``stream_custom_voice_batch``, every
    feeder filled and closed up front) against the same N utterances as whole text
    (``generate_custom_voice_batch_streaming(non_streaming_mode=False)``), runs interleaved;
(c) N simultaneous streams fed one token every 1 / ``--rate`` seconds: p50 / max ``first_text_ms``, and the host's share of the delay
    from a token's arrival to the first frame that can read it -- arrival to the append being queued (``BatchDecoder.text_stats``);
    the device adds the frames queued ahead of the append, at most (look-ahead + 1) batches of ``poll_every`` frames.

Warm-up, then the median with min / max as the spread."""
import argparse
import json
import os
import sys
import threading
import time

ap = argparse.ArgumentParser()
ap.add_argument("--lanes", type=int, default=64)
ap.add_argument("--rate", type=float, default=50.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]

import numpy as np
import torch
import bench
from fq3hip.text_stream import TextFeeder

N, WARM, REPS, FRAMES, N_TOK = args.lanes, 2, max(3, args.reps), 120, 60
TEXT = ("the quick brown fox jumps over the lazy dog and keeps running " * 2)[:N_TOK]
dev = torch.device("cuda:0")
cfg, model = bench.build_model(dev, frames=FRAMES, model_type="custom_voice")
KW = dict(speaker=bench.SPEAKER, language="English", chunk_size=bench.CHUNK, max_new_tokens=FRAMES, min_new_tokens=FRAMES, lanes=N)
tok = model._text_tokenize()
IDS = tok(TEXT)
assert len(IDS) == N_TOK


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=round(float(np.median(xs)), 4), min=round(float(xs.min()), 4), max=round(float(xs.max()), 4), n=int(xs.size))


out = dict(model="synthetic 0.6B CustomVoice, bf16", lanes=N, text_tokens=N_TOK, frames=FRAMES, chunk_size=bench.CHUNK, warmup=WARM, reps=REPS,
           token_rate_per_s=args.rate, device=torch.cuda.get_device_name(0))


def whole():
    t0 = time.perf_counter()
    n = {}
    for i, _a, _sr, tm in model.generate_custom_voice_batch_streaming([TEXT] * N, non_streaming_mode=False, **KW):
        n[i] = tm["total_steps_so_far"]
    torch.cuda.synchronize()
    assert len(n) == N and all(v == FRAMES for v in n.values())
    return (time.perf_counter() - t0) * 1e3 / FRAMES


def streams(rate=None):
    feeders = [TextFeeder(tok) for _ in range(N)]
    stop = threading.Event()
    th = None
    if rate is None:
        for f in feeders:
            f.feed_ids(IDS)
            f.close()
    else:
        def produce():
            t0 = time.perf_counter()
            for k, t in enumerate(IDS):
                while time.perf_counter() - t0 < k / rate:
                    if stop.is_set():
                        break
                    time.sleep(0.0002)
                for f in feeders:
                    f.feed_ids([t])
            for f in feeders:
                f.close()
        th = threading.Thread(target=produce, daemon=True)
        th.start()
    t0 = time.perf_counter()
    n, first = {}, {}
    for i, _a, _sr, tm in model.stream_custom_voice_batch(feeders, **KW):
        n[i] = tm["total_steps_so_far"]
        if "first_text_ms" in tm:
            first[i] = tm["first_text_ms"]
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    stop.set()
    if th is not None:
        th.join(10)
    assert len(n) == N and all(v == FRAMES for v in n.values())
    return wall / FRAMES, [first[i] for i in sorted(first)], dict(model._batch_decoder(N).text_stats)


# (b) interleaved
for _ in range(WARM):
    whole(); streams()
w, s = [], []
for _ in range(REPS):
    w.append(whole()); s.append(streams()[0])
out["b_wall_ms_per_lockstep_frame"] = dict(whole_text=stats(w), text_fed_never_late=stats(s))

# (c)
streams(args.rate)
firsts, waits, held = [], [], []
for _ in range(max(2, REPS // 2)):
    _ms, first, st = streams(args.rate)
    firsts += first
    waits.append((st["append_wait_ms_sum"] / max(1, st["append_wait_n"]), st["append_wait_ms_max"]))
    held.append((st["polls_held"], st["idle_waits"], st["frames_calls"], st["appends"]))
dec = model._batch_decoder(N)
out["c_first_text_ms"] = dict(p50=round(float(np.percentile(firsts, 50)), 2), max=round(float(np.max(firsts)), 2), n=len(firsts),
                              floor_rows_of_first_chunk_ms=round(bench.CHUNK / args.rate * 1e3, 1))
out["c_token_arrival_to_append_queued_ms"] = dict(mean=round(float(np.mean([x[0] for x in waits])), 3), max=round(float(np.max([x[1] for x in waits])), 3))
out["c_frames_queued_ahead_bound"] = dict(lookahead=int(dec.lookahead), poll_every=int(dec.poll_every), frames=(int(dec.lookahead) + 1) * int(dec.poll_every))
out["c_runs_polls_held_idle_waits_frames_calls_appends"] = held

# (a) the lanes of the scheduler, armed on a one-token prompt, tables open
from fq3hip.generate import _prefill_and_arm
dec = model._batch_decoder(N)
model._bind_lane_prompt_weights(dec)
list(dec.run([]))                                         # (returns whatever an earlier run left on the lanes)
f0 = TextFeeder(tok); f0.feed_ids(IDS[:1])
with torch.inference_mode():
    m, talker, config, tie, tam, _tth, tpe = model._custom_prepare(None, bench.SPEAKER, "English", None, False, input_ids=model._text_session_ids(f0))
    for ln in dec.lanes:
        _prefill_and_arm(talker, tie, tam, tie.new_zeros(1, 0, tie.shape[-1]), tpe, config, ln.predictor_graph, ln.talker_graph, 1024, 2,
                         0.9, 50, 1.0, True, 1.05, use_graph=False)
        ln.engine.decode_text_open(1024)
engines = [ln.engine for ln in dec.lanes]


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), host


def batched():
    dec.batch.text_append([(l, [IDS[l % N_TOK]], False) for l in range(N)])


def per_lane():
    for l, e in enumerate(engines):
        e.decode_text_append([IDS[l % N_TOK]], False)


for _ in range(5):
    timed(batched); timed(per_lane)
rb, rp = [], []
for _ in range(20):
    rb.append(timed(batched)); rp.append(timed(per_lane))
out["a_append_of_one_id_per_lane"] = dict(
    batched=dict(stream_ms=stats([r[0] for r in rb]), host_ms=stats([r[1] for r in rb]), launches=5),
    per_lane=dict(stream_ms=stats([r[0] for r in rp]), host_ms=stats([r[1] for r in rp]), launches=4 * N))
rows = [e.decode_text_read() for e in engines[:2]]
torch.cuda.synchronize()
assert torch.equal(rows[0][0::2], rows[0][1::2]), "batched and per-lane rows of the same id differ"
for e in engines:
    e.decode_cancel()
    e.kv_release()
torch.cuda.synchronize()

print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
