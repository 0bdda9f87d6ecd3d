#!/usr/bin/env python3
"""What exact streaming (codec stream states) costs and what it buys, on one MI355X, at the real codec shapes with the
synthetic normalised weights, bf16x2 vocoder, HIP events, medians after a warm-up:

timing    a steady-state chunk of 8 new frames both ways, in the same run and alternating (two rounds each, so that the run's own spread
          shows): EXACT = one ``stream_push`` behind >= 71 cached rows; WINDOWED = the phase-2 decode of [25 context + 8 new] frames with
          the context's samples dropped (``decode_tensor(codes33, first)``) -- single and in groups of 32 utterances per launch set.
          And the first chunk of 8 frames behind a 170-frame ICL reference: EXACT = ``reset`` to the voice's prefix state (the copy) + push;
          WINDOWED = the phase-1 decode of 178 frames behind that prefix state, the last chunk's samples kept.
distance  the default (windowed) StreamingVocoder at chunk 8 over 200 frames against the one-pass decode of the same codes: every chunk is
          compared with the one-pass samples that END where the chunk's frames end (a phase-2 chunk is shorter than 8 frames of audio: the
          deficit is reported too); largest and RMS difference overall, per chunk, and over the first 20 ms behind every chunk boundary.
          The exact vocoder's distance is asserted to be 0.

Writes profiles/codec_stream.json.   usage: codec_stream_probe.py [runs=60] [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd"))
import numpy as np
import torch

SPF = 1920


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
    return round(single, 4), round(e0.elapsed_time(e1) / runs, 4)


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "codec_stream.json")
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.model import StreamingVocoder
    cfg = qwen3_tts_0p6b()
    from fq3hip.weights import synth_weights
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    g = torch.Generator().manual_seed(21)
    nq, cb = cfg.codec.num_quantizers, cfg.codec.codebook_size
    rnd = lambda *shape: torch.randint(0, cb, shape + (nq,), generator=g).cuda()
    res = {"device": torch.cuda.get_device_name(0), "precision": "bf16x2", "runs": runs, "warmup": 10,
           "unit": "ms per chunk of 8 frames: [median of single calls between their own events, per call back to back]"}

    # ---- timing: steady-state chunk ---------------------------------------------------------------------------------------------
    G = 32
    hist, new1, newG = rnd(80), rnd(1, 8), rnd(G, 8)
    win1, winG = rnd(33), rnd(G, 33)
    first = tok.num_samples(33) - 8 * SPF

    def streams(n):
        out = []
        for _ in range(n):
            st = tok.stream_open()
            tok.stream_push([st], hist.unsqueeze(0))
            out.append(st)
        return out

    def pusher(sts, codes):
        budget = tok.stream_positions - 16

        def fn():
            if sts[0].frames > budget:                  # (never within the default number of runs)
                for st in sts:
                    st.reset()
                    tok.stream_push([st], hist.unsqueeze(0))
            tok.stream_push(sts, codes)
        return fn
    s1, sG = streams(1), streams(G)
    cases = {"exact, single": pusher(s1, new1), "windowed, single": lambda: tok.decode_tensor(win1, first),
             f"exact, group of {G}": pusher(sG, newG), f"windowed, group of {G}": lambda: tok.decode_tensor_batch(winG, first)}
    steady = {k: [] for k in cases}
    for _round in range(2):
        for k, fn in cases.items():
            steady[k].append(timed(fn, runs))
    for k in (f"exact, group of {G}", f"windowed, group of {G}"):
        steady[k + ", per utterance"] = [[round(v / G, 4) for v in r] for r in steady[k]]
    res["steady_state_chunk"] = steady
    assert s1[0].frames >= 71

    # ---- timing: first chunk behind a 170-frame reference -------------------------------------------------------------------------
    ref, gen8 = rnd(170), rnd(8)
    pf = tok.prefix_for(ref)
    both = torch.cat([ref, gen8])
    n178 = tok.num_samples_total(178)
    st = tok.stream_open(ref)

    def exact_first():
        st.reset(ref)
        tok.stream_push([st], gen8.unsqueeze(0))
    firsts = {"exact (reset to the prefix + push)": exact_first,
              "windowed (phase 1: 178 frames behind the prefix state)": lambda: tok.decode_tensor(both, n178 - 8 * SPF, prefix=pf)}
    fc = {k: [] for k in firsts}
    for _round in range(2):
        for k, fn in firsts.items():
            fc[k].append(timed(fn, runs))
    res["first_chunk_behind_170_frames"] = fc

    # ---- distance ---------------------------------------------------------------------------------------------------------------------
    from fq3hip.streams import concurrent_stream
    side = concurrent_stream(torch.device("cuda"))
    codes = rnd(200)
    torch.cuda.synchronize()
    one = tok.decode_tensor(codes).cpu().numpy().astype(np.float64)
    chunks = {}
    for name, kw in (("windowed", {}), ("exact", dict(exact=True))):
        voc = StreamingVocoder(tok, None, 8, "cuda", side, **kw)
        chunks[name] = [np.asarray(voc.push(codes[i:i + 8].contiguous())[0]).astype(np.float64) for i in range(0, 200, 8)]
    assert np.array_equal(np.concatenate(chunks["exact"]), one), "the exact stream must BE the one-pass decode"
    edge = int(0.020 * tok.sample_rate)
    per, diffs, edges = [], [], []
    for k, a in enumerate(chunks["windowed"]):
        end = tok.num_samples(8 * (k + 1))
        d = a - one[end - len(a):end]
        diffs.append(d)
        if k > 0:
            edges.append(d[:edge])
        per.append(dict(chunk=k, samples=len(a), deficit=(end - (tok.num_samples(8 * k) if k else 0)) - len(a),
                        max=float(np.abs(d).max()), rms=float(np.sqrt(np.mean(d * d))),
                        max_first_20ms=float(np.abs(d[:edge]).max()), rms_first_20ms=float(np.sqrt(np.mean(d[:edge] ** 2)))))
    alld, alle = np.concatenate(diffs), np.concatenate(edges)
    res["distance_windowed_vs_one_pass"] = dict(
        frames=200, chunk=8, signal_rms=float(np.sqrt(np.mean(one * one))),
        overall=dict(max=float(np.abs(alld).max()), rms=float(np.sqrt(np.mean(alld * alld)))),
        first_20ms_behind_boundaries=dict(max=float(np.abs(alle).max()), rms=float(np.sqrt(np.mean(alle * alle)))),
        samples_missing=int(len(one) - sum(len(a) for a in chunks["windowed"])), per_chunk=per, exact=dict(max=0.0, rms=0.0))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    brief = {k: v for k, v in res.items() if k != "distance_windowed_vs_one_pass"}
    brief["distance"] = {k: v for k, v in res["distance_windowed_vs_one_pass"].items() if k != "per_chunk"}
    print(json.dumps(brief, indent=1))
    tok.close()


if __name__ == "__main__":
    main()
