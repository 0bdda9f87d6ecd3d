#!/usr/bin/env python3
"""Times the device audio output stage (fq3hip/audio_out.py, one launch of audio_out_kernel per push) ALONE, with HIP events:
8 kHz mu-law and 48 kHz s16 out of 24 kHz float32, for a streaming chunk (8 frames = 15 360 samples) and a 370-frame utterance, the
median of the timed runs after a warm-up -- each run its own event pair around one push, and the same pushes back to back under one
pair (the first includes what an event pair around a single short launch costs).  The yardstick, in the same run: the bf16x2
vocoder's streaming-chunk decode (25 context + 8 new frames, the tail of 8 frames produced) at the real codec shapes.  Also the bytes
copied to the host with and without the stage.  Writes profiles/audio_out.json.
With --speed: the time-scale stage (fq3_tsm_*, one launch of tsm_kernel per push, one workgroup walking the chunk's segments) ALONE at
speeds 0.5, 1.25 and 2.0 on the streaming chunk, per push and per segment, next to the same vocoder yardstick from the same run and the
same stream, and as a fraction of it.  Writes profiles/tsm_stage.json.
With --encoding flac: the FLAC stage (fq3_flac_*, a launch pair per push: one workgroup per block, then the gather) ALONE on the
streaming chunk's 15 360 s16 samples at 24 kHz -- speech-like input (a decaying harmonic tone under a little noise) and full-scale noise,
which ends VERBATIM -- next to the s16 output stage (the code of the parent commit, unchanged) and the same vocoder yardstick from
the same run, and bytes out over s16 bytes.  With --recordings DIR (CPU only, no GPU touched): bytes out over s16 bytes of the numpy
reference encoder (tests/_flac_ref.py, the same bytes as the device's) over every integer-PCM WAV under DIR, one ratio per file.  Both
halves keep what the other wrote.  Writes profiles/flac_stage.json.
With --group B: the output chain of a lock-step GROUP -- B rows (at most 32 a library call), one streaming chunk each, 8 kHz mu-law at
speed 1.25 -- through ``audio_out.push_group`` (ONE fq3_tsm_push_group launch + ONE fq3_audio_out_push_group launch) and through B single
``AudioOut.push`` calls (2 B launches: the parent commit's code path), alternating in the same run, each repeat between its own event
pair, plus both forms with the rows landing on the host (one pinned copy against B copies; host clock around the call, which ends in a
synchronise), next to the bf16x2 vocoder's windowed chunk decode for the same group (``decode_tensor_batch`` over B x [25 + 8] frames,
the protocol of profiles/codec_stream.json).  The two forms' bytes are compared before anything is timed.  Writes
profiles/stage_group.json.
With --encoding flac --group B: the FLAC stage of a lock-step group.  (a) The stage ALONE: 1, 8 and B rows, one streaming chunk of s16
samples each, pushed into running streams as ONE fq3_flac_push_group (a launch pair) and as single fq3_flac_push calls (a launch pair per
row), each repeat between its own event pair.  (b) The whole chain with the rows landing on the host, ``push_group_host`` on 8 and B flac
rows, with the group entry and with the per-row launch sequence it replaces (host clock; the call ends in a synchronise).  The forms
alternate in three rounds; the medians, every round's median and their spread are written to profiles/flac_group.json.  The forms' bytes
are compared before anything is timed.
usage: audio_out_probe.py [--speed | --encoding flac [--recordings DIR | --group B] | --group B] [runs=100] [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd"))
import torch
from fq3hip import audio_out as ao

SAMPLES_PER_FRAME = 1920
SETTINGS = (("8 kHz mulaw", 8000, "mulaw"), ("48 kHz s16", 48000, "s16"))
SIZES = (("streaming chunk, 8 frames", 8 * SAMPLES_PER_FRAME), ("utterance, 370 frames", 370 * SAMPLES_PER_FRAME))


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


SPEEDS = (500, 1250, 2000)


def vocoder_chunk(g, runs):
    """the yardstick: (median single call, back to back per call) ms of the bf16x2 vocoder's streaming-chunk decode"""
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    codes = torch.randint(0, cfg.codec.codebook_size, (33, 16), generator=g).cuda()
    first = tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME
    return timed(lambda: tok.decode_tensor(codes, first), runs)


def main_speed(argv):
    runs = max(50, int(argv[0])) if argv else 100
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "tsm_stage.json")
    g = torch.Generator().manual_seed(3)
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "in_rate": 24000, "stage": [], "notes": []}
    voc_single, voc_stream = vocoder_chunk(g, runs)
    res["vocoder_bf16x2_streaming_chunk_ms"] = {"median_single_call": round(voc_single, 4), "back_to_back_per_call": round(voc_stream, 4)}
    n = 8 * SAMPLES_PER_FRAME
    pcm = (torch.rand(n, generator=g) * 2 - 1).cuda()
    N, Hs, D, _ = ao.tsm_design(24000, SPEEDS[0], window=False)
    for P in SPEEDS:
        stage = ao.AudioOut(ao.AudioOutSpec(speed=P / 1000), 24000, "cuda")
        n_out = ao.tsm_count(24000, P, n, True)
        out = torch.empty(n_out, dtype=torch.float32, device="cuda")

        def one():
            # the launch alone: reset (host only) + one final push of the chunk into a buffer that exists
            stage.reset()
            return stage.push_into(pcm, True, out)
        single, stream = timed(one, runs)
        segs = -(-n_out // Hs)
        res["stage"].append({
            "speed_permille": P, "input": "streaming chunk, 8 frames", "n_in": n, "n_out": n_out, "segments": segs,
            "candidates_per_segment": 2 * D + 1, "window": N,
            "median_single_push_ms": round(single, 4), "back_to_back_per_push_ms": round(stream, 4),
            "us_per_segment_back_to_back": round(1000 * stream / segs, 3),
            "fraction_of_vocoder_chunk_back_to_back": round(stream / voc_stream, 4), "flop": 2 * N * (2 * D + 1) * (segs - 1)})
    worst = max(r["fraction_of_vocoder_chunk_back_to_back"] for r in res["stage"])
    res["notes"].append(f"the time-scale stage takes at most {worst:.3f} of the bf16x2 vocoder's chunk decode (back-to-back figures, same stream); "
                        + ("ABOVE 1: with speed on, this stage and not the vocoder bounds the streamed real-time factor" if worst > 1 else
                           "below 1: the vocoder still bounds the streamed chunk, the stage adds this fraction to it"))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


def _merge(out_path, update):
    """the JSON at out_path with `update` laid over it (each half of the flac probe keeps the other's keys)"""
    res = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            res = json.load(f)
    res.update(update)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(update, indent=1))


def _flac_ratio_of_file(path):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _flac_ref as R
    from fq3hip import audio_io
    audio, sr = audio_io.read_wav(path)
    x = np.frombuffer(audio_io.to_pcm16(audio), dtype="<i2")
    stats = []
    data = R.encode(x, sr, stats=stats)
    kinds = [s[0] for s in stats]
    orders = [s[1] for s in stats if s[0] == "fixed"]
    return {"file": os.path.basename(path), "sample_rate": sr, "seconds": round(len(x) / sr, 2), "flac_bytes": len(data),
            "s16_bytes": 2 * len(x), "ratio": round(len(data) / (2 * len(x)), 4), "frames": len(stats),
            "constant": kinds.count("constant"), "verbatim": kinds.count("verbatim"),
            "fixed_by_order": [orders.count(o) for o in range(5)]}


def main_flac_recordings(root, out_path):
    """CPU side: the reference encoder over recordings (the device writes the same bytes; tests/test_gpu_flac.py)"""
    from concurrent.futures import ProcessPoolExecutor
    from fq3hip import audio_io
    paths = []
    for d, _, files in sorted(os.walk(root)):
        paths += [os.path.join(d, f) for f in sorted(files) if f.lower().endswith(".wav")]
    readable = []
    for p in paths:
        try:
            audio_io.read_wav(p)
            readable.append(p)
        except ValueError:
            pass
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        rows = list(ex.map(_flac_ratio_of_file, readable))
    ratios = sorted(r["ratio"] for r in rows)
    _merge(out_path, {"cpu_reference_encoder_over_recordings": {
        "side": "CPU (numpy reference encoder; byte-identical to the device stage by tests/test_gpu_flac.py)",
        "files": rows, "n_files": len(rows), "ratio_min": ratios[0], "ratio_median": ratios[len(ratios) // 2], "ratio_max": ratios[-1],
        "ratio_total": round(sum(r["flac_bytes"] for r in rows) / sum(r["s16_bytes"] for r in rows), 4)}})


def main_flac(argv):
    runs = max(50, int(argv[0])) if argv else 100
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "flac_stage.json")
    g = torch.Generator().manual_seed(3)
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "rate": 24000, "stage": [], "notes": []}
    voc_single, voc_stream = vocoder_chunk(g, runs)
    res["vocoder_bf16x2_streaming_chunk_ms"] = {"median_single_call": round(voc_single, 4), "back_to_back_per_call": round(voc_stream, 4)}
    n = 8 * SAMPLES_PER_FRAME
    t = torch.arange(n, dtype=torch.float64) / 24000.0
    voiced = sum(0.25 / h * torch.sin(2 * torch.pi * 140.0 * h * t) for h in range(1, 9)) * torch.exp(-3.0 * (t % 0.16))
    inputs = (("speech-like: decaying harmonics of 140 Hz, noise at -50 dB", (voiced + 0.003 * torch.randn(n, generator=g)).float().cuda()),
              ("full-scale uniform noise", (torch.rand(n, generator=g) * 2 - 1).cuda()))
    # the s16 stage alone: the parent commit's code and launch, measured in this run
    s16 = ao.AudioOut(ao.AudioOutSpec(None, "s16"), 24000, "cuda")
    s16_out = torch.empty(n, dtype=torch.int16, device="cuda")

    def s16_one():
        s16.reset()
        return s16.push_into(inputs[0][1], True, s16_out)
    s16_single, s16_stream = timed(s16_one, runs)
    res["s16_stage_24k_streaming_chunk_ms"] = {"median_single_push": round(s16_single, 4), "back_to_back_per_push": round(s16_stream, 4),
                                               "note": "fq3_audio_out_push alone; this code is the parent commit's, unchanged"}
    lib = ao._lib.load()
    import ctypes as C
    for name, pcm in inputs:
        stage = ao.AudioOut(ao.AudioOutSpec(None, "flac"), 24000, "cuda")
        pcm16 = ao.AudioOut(ao.AudioOutSpec(None, "s16"), 24000, "cuda").push(pcm, final=True)
        frames = ao.flac_count(24000, stage.flac_block, n, True)
        buf = torch.empty(8 + frames * stage.flac_bound, dtype=torch.uint8, device="cuda")
        got = C.c_int64()

        def one():
            # the launch pair alone: reset (host only) + one final push of the chunk's s16 samples into a buffer that exists
            lib.fq3_flac_reset(stage._flac, None)
            rc = lib.fq3_flac_push(stage._flac, C.c_void_p(pcm16.data_ptr()), n, 1, C.c_void_p(buf.data_ptr() + 8), buf.numel() - 8,
                                   C.byref(got), C.c_void_p(buf.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        single, stream = timed(one, runs)
        nbytes = int(buf[:8].view(torch.int64).item())
        res["stage"].append({
            "input": name, "n_in": n, "block": stage.flac_block, "frames": frames, "launches_per_push": 2,
            "median_single_push_ms": round(single, 4), "back_to_back_per_push_ms": round(stream, 4),
            "fraction_of_vocoder_chunk_back_to_back": round(stream / voc_stream, 4),
            "times_the_s16_stage_back_to_back": round(stream / s16_stream, 2),
            "flac_bytes": nbytes, "s16_bytes": 2 * n, "bytes_ratio": round(nbytes / (2 * n), 4)})
    worst = max(r["fraction_of_vocoder_chunk_back_to_back"] for r in res["stage"])
    res["notes"].append(f"the FLAC stage takes at most {worst:.3f} of the bf16x2 vocoder's chunk decode (back-to-back figures, same stream): "
                        + ("a small fraction, the stage is cheap next to the vocoder" if worst < 0.1 else
                           "NOT a small fraction: the stage is not cheap next to the vocoder"))
    res["notes"].append("CRC-16 form kept: every lane takes a slice of the frame, slices combined in a tree by CRC linearity.  The serial table walk "
                        "was not built: one lane reading up to 2 n + 16 bytes through a dependent LDS load per byte is bounded below by the "
                        "LDS round trip: a 2322-byte frame x two dependent LDS reads per byte (the byte, the table entry) x 64 clocks or more "
                        "each is about 0.12 ms at 2.4 GHz, several times what the whole launch pair measured here takes (an estimate from the commonly quoted LDS latency, not a measurement)")
    _merge(out_path, res)


def main_group(B, argv):
    import time
    runs = max(20, int(argv[0])) if argv else 40
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "stage_group.json")
    g = torch.Generator().manual_seed(3)
    n = 8 * SAMPLES_PER_FRAME
    spec = ao.AudioOutSpec(8000, "mulaw", 1.25)
    t = torch.arange(n, dtype=torch.float64) / 24000.0
    voiced = sum(0.25 / h * torch.sin(2 * torch.pi * 140.0 * h * t) for h in range(1, 9)) * torch.exp(-3.0 * (t % 0.16))
    rows = [(voiced * (0.5 + 0.5 * b / B) + 0.003 * torch.randn(n, generator=g)).float().cuda() for b in range(B)]
    stages = [ao.AudioOut(spec, 24000, "cuda") for _ in range(B)]
    finals = [True] * B

    def reset():
        for st in stages:
            st.reset()                                            # host only

    def group():
        reset()
        return ao.push_group(stages, rows, finals)

    def singles():
        reset()
        return [st.push(x, True) for st, x in zip(stages, rows)]

    def group_host():
        reset()
        return ao.push_group_host(stages, rows, finals)

    def singles_host():
        reset()
        return [st.push_host(x, True) for st, x in zip(stages, rows)]

    a, b = group(), singles()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "the group form and the single pushes must write the same bytes"
    n_out = int(a[0].numel())

    def events(fn):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
        for e0, e1 in pairs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in pairs]

    def clock(fn):
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1000)
        return out

    res = {"device": torch.cuda.get_device_name(0), "rows": B, "runs_per_round": runs, "rounds": 3, "warmup": 10, "in_rate": 24000,
           "spec": "8 kHz mu-law, speed 1.25", "n_in_per_row": n, "n_out_per_row": n_out,
           "unit": "ms per group of rows: median over all repeats; per_round: the median of each alternating round",
           "launches": {"push_group": 2 * -(-B // ao.GROUP_MAX), "single pushes": 2 * B}}
    voc_single, voc_stream = vocoder_group(g, B, runs)
    res["vocoder_bf16x2_windowed_chunk_group_ms"] = {"median_single_call": round(voc_single, 4), "back_to_back_per_call": round(voc_stream, 4)}
    cases = {"push_group (device rows)": (group, events), "single pushes (device rows)": (singles, events),
             "push_group_host (one pinned copy)": (group_host, clock), "single push_host calls": (singles_host, clock)}
    for fn, _how in cases.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _round in range(3):                                       # alternating: the forms see the same machine
        for k, (fn, how) in cases.items():
            samples[k].append(how(fn))
    res["stage"] = {k: {"how": "device events around the call" if cases[k][1] is events else "host clock around the call (it ends in a synchronise)",
                        "median_ms": round(statistics.median(v for r in rs for v in r), 4),
                        "per_round_ms": [round(statistics.median(r), 4) for r in rs],
                        "min_ms": round(min(v for r in rs for v in r), 4)} for k, rs in samples.items()}
    gd, sd = res["stage"]["push_group (device rows)"]["median_ms"], res["stage"]["single pushes (device rows)"]["median_ms"]
    gh, sh = res["stage"]["push_group_host (one pinned copy)"]["median_ms"], res["stage"]["single push_host calls"]["median_ms"]
    res["notes"] = [
        f"device rows: the group form takes {gd:.3f} ms, the {B} single pushes {sd:.3f} ms: " +
        (f"{sd / gd:.2f}x faster" if gd < sd else f"NOT faster ({gd / sd:.2f}x the singles' time)"),
        f"rows on the host: {gh:.3f} ms against {sh:.3f} ms: " + (f"{sh / gh:.2f}x faster" if gh < sh else f"NOT faster ({gh / sh:.2f}x the singles' time)"),
        f"the vocoder's chunk decode for the same group takes {voc_stream:.3f} ms back to back: the group form is {gd / voc_stream:.3f} of it, "
        f"the single pushes {sd / voc_stream:.3f}",
        "every figure includes the host side of the call (Python, ctypes, the output allocations); the pushes are final pushes from a reset "
        "stage, as in the other modes of this probe"]
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


class _PerRowFlac:
    """the library with fq3_flac_push_group answered by one fq3_flac_push per row: the launch sequence of the commit before the group
    form (a launch pair per flac row behind the grouped s16 launch), rebuilt in this run so that both forms see the same machine"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def fq3_flac_push_group(self, objs, B, pcm, n_in, final, out, caps, n_frames, n_bytes, sp):
        import ctypes as C
        for b in range(B):
            got = C.c_int64()
            rc = self._lib.fq3_flac_push(objs[b], pcm[b], n_in[b], final[b], out[b], caps[b], C.byref(got), n_bytes[b], sp)
            if rc:
                return rc
            n_frames[b] = got.value
        return 0


def main_flac_group(N, argv):
    """(a) the FLAC stage alone: B rows, one streaming chunk of s16 samples each, pushed into RUNNING streams (never final: the tails
    carry over, a push completes 13 or 14 frames of 1152), as B fq3_flac_push calls and as ONE fq3_flac_push_group, device time between
    events; (b) the whole chain with the rows on the host, ``push_group_host`` on flac rows, against the per-row launch sequence."""
    import ctypes as C
    import time
    runs = max(20, int(argv[0])) if argv else 40
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "flac_group.json")
    rounds = 3
    g = torch.Generator().manual_seed(3)
    n = 8 * SAMPLES_PER_FRAME
    lib = ao._lib.load()
    t = torch.arange(n, dtype=torch.float64) / 24000.0
    voiced = sum(0.25 / h * torch.sin(2 * torch.pi * 140.0 * h * t) for h in range(1, 9)) * torch.exp(-3.0 * (t % 0.16))
    rows_f32 = [(voiced * (0.5 + 0.5 * b / N) + 0.003 * torch.randn(n, generator=g)).float().cuda() for b in range(N)]
    rows_s16 = [ao.AudioOut(ao.AudioOutSpec(None, "s16"), 24000, "cuda").push(x, final=True) for x in rows_f32]
    block, bound = ao.flac_design(24000)
    cap = (n // block + 1) * bound
    sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def events(fn):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
        for e0, e1 in pairs:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in pairs]

    def clock(fn):
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1000)
        return out

    def measure(cases, how):
        for fn in cases.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in cases}
        for _round in range(rounds):                              # alternating: the forms see the same machine
            for k, fn in cases.items():
                samples[k].append(how(fn))
        out = {}
        for k, rs in samples.items():
            per_round = [statistics.median(r) for r in rs]
            out[k] = {"median_ms": round(statistics.median(v for r in rs for v in r), 4), "per_round_ms": [round(v, 4) for v in per_round],
                      "spread_ms": round(max(per_round) - min(per_round), 4), "min_ms": round(min(v for r in rs for v in r), 4)}
        return out

    res = {"device": torch.cuda.get_device_name(0), "runs_per_round": runs, "rounds": rounds, "warmup": 10, "rate": 24000, "block": block,
           "n_in_per_row": n, "input": "speech-like: decaying harmonics of 140 Hz, noise at -50 dB, another level per row",
           "unit": "ms per group of rows: median over all repeats; per_round: the median of each alternating round; spread: the largest "
                   "minus the smallest round median", "stage_alone": [], "whole_chain_rows_on_host": [], "notes": []}

    # (a)
    for B in sorted({1, 8, N}):
        objs = [[ao.AudioOut(ao.AudioOutSpec(None, "flac"), 24000, "cuda") for _ in range(B)] for _form in range(2)]
        bufs = [torch.zeros(B * (8 + cap), dtype=torch.uint8, device="cuda") for _form in range(2)]
        outs = [[buf.data_ptr() + b * (8 + cap) for b in range(B)] for buf in bufs]
        h_group = (C.c_void_p * B)(*[st._flac.value for st in objs[0]])
        pcm = (C.c_void_p * B)(*[x.data_ptr() for x in rows_s16[:B]])
        lens, finals, caps, got = (C.c_int64 * B)(*([n] * B)), (C.c_int * B)(*([0] * B)), (C.c_int64 * B)(*([cap] * B)), (C.c_int64 * B)()
        g_out, g_nb = (C.c_void_p * B)(*[p + 8 for p in outs[0]]), (C.c_void_p * B)(*outs[0])

        def group():
            assert lib.fq3_flac_push_group(h_group, B, pcm, lens, finals, g_out, caps, got, g_nb, sp()) == 0

        def singles():
            one, s = C.c_int64(), sp()
            for b, st in enumerate(objs[1]):
                assert lib.fq3_flac_push(st._flac, pcm[b], n, 0, C.c_void_p(outs[1][b] + 8), cap, C.byref(one), C.c_void_p(outs[1][b]), s) == 0

        group(); singles()
        torch.cuda.synchronize()
        assert torch.equal(bufs[0], bufs[1]), "the group form and the single pushes must write the same bytes"
        m = measure({"fq3_flac_push_group": group, "single fq3_flac_push calls": singles}, events)
        gm, sm = m["fq3_flac_push_group"], m["single fq3_flac_push calls"]
        spread = max(gm["spread_ms"], sm["spread_ms"])
        res["stage_alone"].append({"rows": B, "how": "device events around the call(s)", "launches": {"group": 2, "singles": 2 * B},
                                   "forms": m, "spread_ms": spread, "singles_over_group": round(sm["median_ms"] / gm["median_ms"], 2)})
        if B == N:
            ok = sm["median_ms"] - gm["median_ms"] > spread
            res["notes"].append(f"B = {B}: the group form takes {gm['median_ms']:.3f} ms, the single pushes {sm['median_ms']:.3f} ms, spread {spread:.3f} ms: "
                                + ("faster by more than the spread" if ok else "NOT faster by more than the spread"))
        if B == 1:
            ok = gm["median_ms"] - sm["median_ms"] <= spread
            res["notes"].append(f"B = 1: the group form takes {gm['median_ms']:.3f} ms, the single push {sm['median_ms']:.3f} ms, spread {spread:.3f} ms: "
                                + ("not slower by more than the spread" if ok else "SLOWER by more than the spread: a bucket of one row belongs to the single push"))

    # (b)
    for B in sorted({8, N} - {1}):
        stages = [[ao.AudioOut(ao.AudioOutSpec(None, "flac"), 24000, "cuda") for _ in range(B)] for _form in range(2)]
        stages[1][0]._lib = _PerRowFlac(lib)                      # ``_push_group`` takes the library from its first stage
        pcms, no = rows_f32[:B], [False] * B
        a, b = ao.push_group_host(stages[0], pcms, no), ao.push_group_host(stages[1], pcms, no)
        assert all((u == v).all() for u, v in zip(a, b)), "both launch sequences must give the same bytes"
        m = measure({"push_group_host, fq3_flac_push_group": lambda: ao.push_group_host(stages[0], pcms, no),
                     "push_group_host, one fq3_flac_push per row": lambda: ao.push_group_host(stages[1], pcms, no)}, clock)
        gm, sm = m["push_group_host, fq3_flac_push_group"], m["push_group_host, one fq3_flac_push per row"]
        res["whole_chain_rows_on_host"].append({"rows": B, "how": "host clock around the call (it ends in a synchronise)",
                                                "launches": {"group": 3, "per row": 1 + 2 * B}, "forms": m,
                                                "per_row_over_group": round(sm["median_ms"] / gm["median_ms"], 2)})
    res["notes"].append("every figure includes the host side of the call (ctypes; in the whole chain also Python and the allocations); the per-row "
                        "form of the whole chain is the earlier launch sequence rebuilt in this run (the library's group entry answered by one "
                        "single push per row), not a second build")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


def vocoder_group(g, B, runs):
    """the yardstick for a group: (median single call, back to back per call) ms of the bf16x2 vocoder's windowed chunk decode of B rows"""
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    codes = torch.randint(0, cfg.codec.codebook_size, (B, 33, 16), generator=g).cuda()
    first = tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME
    return timed(lambda: tok.decode_tensor_batch(codes, first), runs)


def main():
    args = sys.argv[1:]
    if "--group" in args:
        i = args.index("--group")
        B, rest = int(args[i + 1]), args[:i] + args[i + 2:]
        if "--encoding" in rest:
            j = rest.index("--encoding")
            assert rest[j + 1] == "flac", "--encoding flac is the only encoding with a probe of its own"
            return main_flac_group(B, rest[:j] + rest[j + 2:])
        return main_group(B, rest)
    if "--encoding" in args:
        i = args.index("--encoding")
        assert args[i + 1] == "flac", "--encoding flac is the only encoding with a probe of its own"
        rest = args[:i] + args[i + 2:]
        if "--recordings" in rest:
            j = rest.index("--recordings")
            root, rest = rest[j + 1], rest[:j] + rest[j + 2:]
            return main_flac_recordings(root, rest[-1] if rest and rest[-1].endswith(".json") else os.path.join(ROOT, "profiles", "flac_stage.json"))
        return main_flac(rest)
    if "--speed" in sys.argv[1:]:
        return main_speed([a for a in sys.argv[1:] if a != "--speed"])
    runs = max(50, int(sys.argv[1])) if len(sys.argv) > 1 else 100
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "audio_out.json")
    g = torch.Generator().manual_seed(3)
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "in_rate": 24000, "stage": [], "notes": []}

    voc_single, voc_stream = vocoder_chunk(g, runs)
    res["vocoder_bf16x2_streaming_chunk_ms"] = {"median_single_call": round(voc_single, 4), "back_to_back_per_call": round(voc_stream, 4)}

    for size_name, n in SIZES:
        pcm = (torch.rand(n, generator=g) * 2 - 1).cuda()
        for name, rate, enc in SETTINGS:
            spec = ao.AudioOutSpec(rate, enc)
            stage = ao.AudioOut(spec, 24000, "cuda")
            L, M, K, _ = ao.design(24000, rate, bank=False)
            n_out = ao.count(24000, rate, n, True)
            out = torch.empty(n_out, dtype=stage.dtype, device="cuda")

            def one():
                # the launch alone: reset (host only) + one final push into a buffer that exists
                stage.reset()
                return stage.push_into(pcm, True, out)
            single, stream = timed(one, runs)
            bytes_out, bytes_plain = n_out * out.element_size(), n * 4
            res["stage"].append({
                "setting": name, "input": size_name, "n_in": n, "n_out": n_out, "L": L, "M": M, "taps_per_output": K,
                "median_single_push_ms": round(single, 4), "back_to_back_per_push_ms": round(stream, 4),
                "share_of_vocoder_chunk_back_to_back": round(stream / voc_stream, 5) if n == 8 * SAMPLES_PER_FRAME else None,
                "flop": 2 * K * n_out, "bytes_to_host_with_stage": bytes_out, "bytes_to_host_float32_24k": bytes_plain,
                "bytes_ratio": round(bytes_out / bytes_plain, 4)})
    chunk = [r for r in res["stage"] if r["n_in"] == 8 * SAMPLES_PER_FRAME]
    worst = max(r["share_of_vocoder_chunk_back_to_back"] for r in chunk)
    res["notes"].append(f"streaming chunk: the stage is at most {100 * worst:.2f} % of the bf16x2 vocoder's chunk decode (back-to-back figures); "
                        + ("launch-bound as expected (well under 1 %)" if worst < 0.01 else "NOT under 1 %: the expectation of a stage well under 1 % of the chunk does not hold here"))
    for name, _rate, _enc in SETTINGS:
        small, large = (next(r for r in res["stage"] if r["setting"] == name and r["n_in"] == n) for _, n in SIZES)
        growth = large["back_to_back_per_push_ms"] / small["back_to_back_per_push_ms"]
        res["notes"].append(f"{name}: {large['n_in'] // small['n_in']}x the input takes {growth:.2f}x the time per push"
                            + (": the figure is what issuing one push costs (Python, ctypes, one launch), not kernel work" if growth < 1.5 else ""))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
