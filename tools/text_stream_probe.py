#!/usr/bin/env python3
"""Incremental text, measured (record, do not gate): profiles/text_stream_ttfa.json.

For a 60-token text on the synthetic 0.6B CustomVoice model (bench.py's model, chunk size and sampling):

(a) first piece -> first audio of a text session (``stream_custom_voice`` fed by a ``TextFeeder``) whose tokens arrive at 20, 50 and
    200 per second (host timer, one id per tick through ``feed_ids``: the arrival of TOKENS is what is modelled; ``feed(str)`` would
    add the wait for the end of the first word);
(b) the same clock for the whole-text path, which can only start when the last token is there: arrival of the last token (computed:
    59 / rate) + the measured time to first audio of ``generate_custom_voice_streaming(non_streaming_mode=False)``;
(c) wall milliseconds per frame of a 120-frame utterance, the session with all text fed up front against the whole-text call, runs
    interleaved in one process -- and, with ``--parent-root DIR`` (a checkout of the parent commit with its library built), the
    whole-text call on that build and on this one in alternating child processes on the same device in the same run.

Warm-up 3, then the median of ``--reps`` (>= 10) with min / max as the spread.  ``--baseline-only`` prints the whole-text figures of
the tree given by ``--root`` (that is how the parent is measured)."""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--parent-root")
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]

import numpy as np
import torch
import bench

WARM, REPS, FRAMES, N_TOK = 3, max(10, args.reps), 120, 60
TEXT = ("the quick brown fox jumps over the lazy dog and keeps running " * 2)[:N_TOK]
dev = torch.device("cuda:0")
cfg, model = bench.build_model(dev, frames=FRAMES, model_type="custom_voice")
KW = dict(speaker=bench.SPEAKER, language="English", chunk_size=bench.CHUNK)


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=round(float(np.median(xs)), 3), min=round(float(xs.min()), 3), max=round(float(xs.max()), 3), n=int(xs.size))


def run(gen, until_first=False):
    """-> (ms to the first audio chunk, wall ms - prefill ms, frames)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first, prefill, n = None, 0.0, 0
    for _audio, _sr, tm in gen:
        if first is None:
            first, prefill = (time.perf_counter() - t0) * 1e3, tm["prefill_ms"]
            if until_first:
                gen.close()
                break
        n = tm["total_steps_so_far"]
    torch.cuda.synchronize()
    return first, (time.perf_counter() - t0) * 1e3 - prefill, n


def whole(seed, frames=FRAMES, **kw):
    torch.manual_seed(seed)
    return run(model.generate_custom_voice_streaming(TEXT, non_streaming_mode=False, max_new_tokens=frames, min_new_tokens=frames, **KW), **kw)


if args.baseline_only:
    for i in range(WARM):
        whole(i)
    rows = [whole(10 + i) for i in range(REPS)]
    print(json.dumps(dict(ttfa_ms=stats([r[0] for r in rows]), ms_per_step=stats([r[1] / r[2] for r in rows]))))
    sys.exit(0)

from fq3hip.text_stream import TextFeeder

tok = model._text_tokenize()
IDS = tok(TEXT)
assert len(IDS) == N_TOK


def session(seed, rate=None, frames=FRAMES, **kw):
    """rate None: all text up front; else one token every 1 / rate seconds from another thread, the first at t = 0."""
    torch.manual_seed(seed)
    f = TextFeeder(tok)
    if rate is None:
        f.feed_ids(IDS)
        f.close()
        th = None
    else:
        stop = threading.Event()

        def produce():
            t0 = time.perf_counter()
            for i, t in enumerate(IDS):
                while time.perf_counter() - t0 < i / rate:
                    if stop.is_set():
                        f.close()
                        return
                    time.sleep(0.0002)
                f.feed_ids([t])
            f.close()
        th = threading.Thread(target=produce, daemon=True)
        th.start()
    gen = model.stream_custom_voice(f, max_new_tokens=frames, min_new_tokens=frames, **KW)
    torch.cuda.synchronize()
    first_text = None
    t0 = time.perf_counter()
    n, prefill = 0, 0.0
    for _audio, _sr, tm in gen:
        if first_text is None:
            first_text, prefill = tm["first_text_ms"], tm["prefill_ms"]
            if kw.get("until_first"):
                gen.close()
                break
        n = tm["total_steps_so_far"]
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 - prefill
    if th is not None:
        stop.set()
        th.join(10)
    return first_text, wall, n


out = dict(model="synthetic 0.6B CustomVoice, bf16", text_tokens=N_TOK, frames=FRAMES, chunk_size=bench.CHUNK, warmup=WARM, reps=REPS,
           device=torch.cuda.get_device_name(0))
# identity first: a probe of a broken session would time something else
torch.manual_seed(5)
a = [x[0] for x in model.generate_custom_voice_streaming(TEXT, non_streaming_mode=False, max_new_tokens=24, min_new_tokens=24, **KW)]
torch.manual_seed(5)
f = TextFeeder(tok); f.feed_ids(IDS); f.close()
b = [x[0] for x in model.stream_custom_voice(f, max_new_tokens=24, min_new_tokens=24, **KW)]
assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), "the session's audio differs from the whole-text call"

# (c) interleaved
for i in range(WARM):
    whole(i); session(i)
w_rows, s_rows = [], []
for i in range(REPS):
    w_rows.append(whole(10 + i)); s_rows.append(session(10 + i))
out["c_ms_per_step"] = dict(whole_text=stats([r[1] / r[2] for r in w_rows]), session_text_up_front=stats([r[1] / r[2] for r in s_rows]))
out["whole_text_ttfa_ms"] = stats([r[0] for r in w_rows])
out["session_text_up_front_first_text_ms"] = stats([r[0] for r in s_rows])
# (a), (b)
out["a_b_first_piece_to_first_audio_ms"] = {}
for rate in (20, 50, 200):
    for i in range(WARM):
        session(i, rate, until_first=True)
    rows = [session(30 + i, rate, until_first=True) for i in range(REPS)]
    last_token_ms = (N_TOK - 1) / rate * 1e3
    out["a_b_first_piece_to_first_audio_ms"][f"{rate}_tokens_per_s"] = dict(
        a_session=stats([r[0] for r in rows]),
        a_floor_rows_of_first_chunk_ms=round(bench.CHUNK / rate * 1e3, 1),      # frame g needs token g + 1: the first chunk's last row is token CHUNK
        b_whole_text=round(last_token_ms + out["whole_text_ttfa_ms"]["median"], 3), b_last_token_arrives_ms=round(last_token_ms, 1))
if args.parent_root:
    # process-to-process spread is larger than any difference looked for here (clocks, allocation order): alternate child processes of
    # the two builds and report every one of them
    def child(root):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--root", root, "--reps", str(REPS)],
                           capture_output=True, text=True, timeout=900)
        return json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else dict(error=r.stderr[-400:])
    pairs = [dict(parent_commit=child(args.parent_root), this_tree=child(ROOT)) for _ in range(3)]
    out["c_whole_text_alternating_processes"] = pairs
print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
