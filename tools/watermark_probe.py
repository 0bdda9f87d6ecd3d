#!/usr/bin/env python3
"""Times the watermark stage (fq3hip/watermark.py: fq3_mark_push, one launch, a workgroup per 15 hops; fq3_mark_detect, two launches)
ALONE, with HIP events, beside the bf16x2 vocoder's streaming-chunk decode (25 context + 8 new frames, the tail of 8 produced) in the
same run and on the same stream: stage and vocoder ALTERNATE inside every repeat, each between its own event pair, and the figures are
medians over the repeats after a warm-up (``loudness_probe.alternate`` holds the method).
  push    an 8-frame streaming chunk (15 360 samples; one non-final push into a stream that is already running) and a 370-frame
          utterance (710 400 samples; reset + one final push)
  detect  over 3 s and over 30 s at 24 kHz
Also, so that one file holds them: the embed and detect error bounds of tests/test_gpu_watermark.py with the device's errors, and the
a = 0.1 repeat on the synthetic voiced signal of tests/_mark_ref.py -- SNR and the detector's max z for the marked signal behind s16,
cropped by 1000 samples, behind a 24 -> 8 -> 24 kHz round trip, unmarked and under another key.  Writes profiles/watermark.json.
usage: watermark_probe.py [runs=60] [out.json]
       watermark_probe.py --scan [runs=30] [out.json]    the scan against one-by-one detect (``scan_main``) -> profiles/mark_scan.json
       watermark_probe.py --group 1,8,32 [runs=60] [out.json]    the group push against single pushes (``group_main``) -> profiles/mark_group.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from fq3hip import watermark as W
from loudness_probe import SAMPLES_PER_FRAME, alternate, speech_like

KEY, A = 0x0123456789ABCDEF, float(np.float32(0.1))


def mark(x, strength=0.1):
    return W.Watermark(KEY, strength, "cuda").push(torch.from_numpy(np.array(x)).cuda(), final=True).cpu().numpy()


def accuracy():
    """the GPU test's bounds (4 x the numpy-float32 evaluation's deviation from float64) and the device's errors on the same inputs"""
    import _mark_ref as R
    rows = {"embed": [], "detect": []}
    for n in (1, 255, 256, 257, 511, 512, 513, 769, 4000):
        x = R.voiced(0.2)[300:300 + n]
        ref = R.embed(x, KEY, A)
        rows["embed"].append({"n": n, "bound": 4.0 * float(np.max(np.abs(R.embed(x, KEY, A, np.float32) - ref))),
                              "device_error": float(np.max(np.abs(mark(x).astype(np.float64) - ref)))})
    x = R.voiced(3.0)
    y = mark(x)
    s16 = (np.round(y.astype(np.float64) * 32767.0) / 32767.0).astype(np.float32)
    for drop in (0, 1000):
        ref = R.detect_table(s16[drop:], KEY)
        z = W.detect_table(s16[drop:], 24000, KEY).cpu().numpy()
        rows["detect"].append({"drop": drop, "bound": 4.0 * float(np.max(np.abs(R.detect_table(s16[drop:], KEY, np.float32) - ref))),
                               "device_error": float(np.max(np.abs(z - ref))), "max_z_device": float(z.max()), "max_z_ref64": float(ref.max())})
    from fq3hip.audio_out import resample_device
    back = resample_device(resample_device(s16, 24000, 8000, "cuda"), 8000, 24000, "cuda")
    noise = x.astype(np.float64) - y
    rows["repeat_a_0p1"] = {
        "signal": "tests/_mark_ref.voiced(3.0): harmonic stack, moving f0, 2.3 Hz envelope, noise floor; NOT a real voice",
        "snr_db": float(10 * np.log10(np.sum(x.astype(np.float64) ** 2) / np.sum(noise ** 2))),
        "max_z": {"marked_s16": W.detect(s16, 24000, KEY).z, "cropped_1000": W.detect(s16[1000:], 24000, KEY).z,
                  "round_trip_24_8_24": W.detect(back, 24000, KEY).z, "at_8_khz": W.detect(resample_device(s16, 24000, 8000, "cuda"), 8000, KEY).z,
                  "unmarked": W.detect(x, 24000, KEY).z, "other_key": W.detect(s16, 24000, KEY + 1).z,
                  "marked_6s": W.detect(mark(R.voiced(6.0)), 24000, KEY).z},
        "threshold": W.THRESHOLD}
    return rows


def main():
    runs = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 60
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "watermark.json")
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    g = torch.Generator().manual_seed(3)
    cfg = qwen3_tts_0p6b()
    wts = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, wts, "cuda", max_frames=400, precision="bf16x2")
    codes = torch.randint(0, cfg.codec.codebook_size, (33, 16), generator=g).cuda()
    first = tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME
    chunk, utt = speech_like(8 * SAMPLES_PER_FRAME, g), speech_like(370 * SAMPLES_PER_FRAME, g)
    sec3, sec30 = speech_like(3 * 24000, g), speech_like(30 * 24000, g)
    running, whole = W.Watermark(KEY, 0.1, "cuda"), W.Watermark(KEY, 0.1, "cuda")
    running.push(chunk)                                            # the stream is running: the history is full from here on

    def utterance():
        whole.reset()
        return whole.push(utt, final=True)
    t = alternate({"push chunk": lambda: running.push(chunk), "push utterance": utterance,
                   "detect 3 s": lambda: W.detect_table(sec3, 24000, KEY), "detect 30 s": lambda: W.detect_table(sec30, 24000, KEY),
                   "vocoder": lambda: tok.decode_tensor(codes, first)}, runs)
    voc = t["vocoder"]
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "rate": 24000, "frame": W.N, "hop": W.H, "strength": A,
           "method": "HIP events around each call, the stage's calls and the vocoder alternating inside every repeat, medians",
           "yardstick": "bf16x2 vocoder, streaming-chunk decode: 25 context + 8 new frames, the tail of 8 produced",
           "vocoder_chunk_ms": round(voc, 4),
           "push": [{"input": "streaming chunk, 8 frames", "n_in": int(chunk.numel()), "push": "one push of a running stream",
                     "workgroups": -(-(int(chunk.numel()) // W.H) // 15) + 1, "ms": round(t["push chunk"], 4),
                     "share_of_vocoder_chunk": round(t["push chunk"] / voc, 5)},
                    {"input": "utterance, 370 frames", "n_in": int(utt.numel()), "push": "reset + one final push",
                     "workgroups": -(-(-(-int(utt.numel()) // W.H)) // 15) + 1, "ms": round(t["push utterance"], 4),
                     "share_of_vocoder_chunk": round(t["push utterance"] / voc, 5)}],
           "detect": [{"seconds": s, "n": int(x.numel()), "launches": 2, "ms": round(t[k], 4), "share_of_vocoder_chunk": round(t[k] / voc, 5)}
                      for s, x, k in ((3, sec3, "detect 3 s"), (30, sec30, "detect 30 s"))],
           "hold_back_ms": [round(1000 * W.H / 24000, 2), round(1000 * (2 * W.H - 1) / 24000, 2)],
           "notes": ["an event pair around ONE short launch includes what starting it costs, and the Python wrapper's output allocation "
                     "lies inside it too; detect's figures include its workspace and table allocations",
                     "NOT measured: audibility on real voices, robustness to lossy codecs, to a change of time scale after marking "
                     "(refused by the model: speed != 1 with the mark), and to deliberate removal; the strength 0.1 is not tuned on real voices"]}
    res["accuracy"] = accuracy()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


def scan_main(argv):
    """--scan: 1, 8 and 32 clips of 3 s and of 30 s through ``scan`` (fq3_mark_scan: two launches and one pinned copy per call)
    against the same clips through ``detect`` one by one, in the same run: HIP events, the two paths alternating inside every repeat,
    medians.  'host' rows end with the verdicts on the host (scan's pinned copy; detect's table copy per clip); 'device' rows only
    enqueue (``scan_blocks_device`` against ``detect_table`` per clip).  Writes profiles/mark_scan.json."""
    runs = max(10, int(argv[0])) if argv else 30
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "mark_scan.json")
    g = torch.Generator().manual_seed(3)
    win, hop = W.scan_blocks(3.0, 1.0)
    rows = []
    for seconds in (3, 30):
        pool = [speech_like(seconds * 24000, g) for _ in range(32)]
        for B in (1, 8, 32):
            clips = pool[:B]
            t = alternate({"scan host": lambda: W.scan(clips, 24000, KEY),
                           "detect host": lambda: [W.detect(c, 24000, KEY) for c in clips],
                           "scan device": lambda: W.scan_blocks_device(clips, [KEY] * B, win, hop),
                           "detect device": lambda: [W.detect_table(c, 24000, KEY) for c in clips]}, runs)
            rows.append({"clips": B, "seconds": seconds, "windows_per_clip": W.scan_windows(seconds * 24000, win, hop),
                         "scan_launches": 2, "detect_launches": 2 * B, **{k.replace(" ", "_") + "_ms": round(v, 4) for k, v in t.items()}})
            print(rows[-1], flush=True)
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "rate": 24000, "win_blocks": win, "hop_blocks": hop,
           "method": "HIP events around each path, scan and one-by-one detect alternating inside every repeat, medians",
           "rows": rows,
           "notes": ["scan answers a verdict per window (and per clip), detect one per clip: the same DFT work, more answers",
                     "the event pairs include the Python wrappers' allocations; the 'host' rows include a stream synchronise",
                     "NOT measured: detection of short marked passages in real speech; whether 3 s is the right window"]}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def group_main(argv):
    """--group 1,8,32: for every row count B, one 8-frame chunk (15 360 samples) per row pushed into B running streams, each under
    its own key -- ``push_group`` (fq3_mark_push_group: one launch) against the same chunks through ``Watermark.push`` row by row on
    a second set of streams, in the same run: HIP events, the two paths alternating inside every repeat, medians and quartiles (the
    quartiles are the run's own spread).  Writes profiles/mark_group.json."""
    import statistics
    from loudness_probe import event_ms
    counts = [int(v) for v in argv[0].split(",")]
    runs = max(20, int(argv[1])) if len(argv) > 1 else 60
    out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "mark_group.json")
    g = torch.Generator().manual_seed(3)
    pool = [speech_like(8 * SAMPLES_PER_FRAME, g) for _ in range(max(counts))]
    rows = []
    for B in counts:
        chunks = pool[:B]
        grouped, singles = [[W.Watermark(KEY + b, 0.1, "cuda") for b in range(B)] for _ in range(2)]
        fns = {"group": lambda: W.push_group(grouped, chunks, [False] * B),
               "single": lambda: [m.push(c) for m, c in zip(singles, chunks)]}
        for _ in range(8):                                         # warm-up; the streams are running from here on
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        marks = {k: [] for k in fns}
        for _ in range(runs):
            for k, fn in fns.items():
                marks[k].append(event_ms(fn))
            torch.cuda.synchronize()
        row = {"rows": B, "n_in_per_row": int(chunks[0].numel()), "group_launches": 1, "single_launches": B,
               "group_workgroups": B * (-(-(int(chunks[0].numel()) // W.H) // 15) + 1)}
        for k, v in marks.items():
            ms = sorted(a.elapsed_time(b) for a, b in v)
            q = statistics.quantiles(ms, n=4)
            row.update({k + "_ms": round(statistics.median(ms), 4), k + "_p25_ms": round(q[0], 4), k + "_p75_ms": round(q[2], 4)})
        row["single_over_group"] = round(row["single_ms"] / row["group_ms"], 3)
        rows.append(row)
        print(row, flush=True)
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "rate": 24000,
           "method": "HIP events around each path, the group call and the row-by-row pushes alternating inside every repeat; medians, "
                     "with the quartiles as the run's own spread",
           "rows": rows,
           "notes": ["the event pairs include the Python wrappers' output allocations: one per group call, one per single push",
                     "at 32 rows every workgroup streams the 512 KB of DFT tables from L2",
                     "NOT measured: the end-to-end factor of a 128-lane batch with watermark="]}
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if "--group" in sys.argv[1:]:
        at = sys.argv.index("--group")
        group_main(sys.argv[at + 1:])
    elif "--scan" in sys.argv[1:]:
        scan_main([a for a in sys.argv[1:] if a != "--scan"])
    else:
        main()
