#!/usr/bin/env python3
"""Times the limiter stage (fq3hip/limiter.py: fq3_limit_push, one launch, a workgroup per tile of output samples) ALONE, with HIP
events, on a 370-frame utterance (710 400 samples at 24 kHz) and on a streaming chunk's worth (8 frames, 15 360 samples), each
beside the bf16x2 vocoder's time for the same audio in the same run and on the same stream: the full decode of 370 frames, and the
streaming-chunk decode (25 context + 8 new frames, the tail of 8 frames produced).  Stage and vocoder ALTERNATE: every repeat times
the push at every tile size and then the vocoder, each between its own event pair; the figures are the medians over the repeats after
a warm-up.  The utterance is one final push into a reset object; the chunk is one non-final push into a stream that is already
running (its history full), as a streaming vocoder issues it.  The input is driven 12 dB over the ceiling in places, so that the
limiter works; its time does not depend on the data.  Also the detector's figures on the GPU tests' signals (tests/_limit_ref.py):
the under-read against the 32x float64 yardstick and the true-peak overshoot of the limited output -- CPU measurements, taken here so
that one file holds them.  Writes profiles/limiter_stage.json.
With --group N: N rows of one streaming chunk into N running streams through ``limiter.push_group`` (ONE launch) and through N single
pushes, alternating in the same process, beside the bf16x2 vocoder's chunk decode of the same rows (``leveller_probe.group_probe``
holds the method); writes its section of profiles/level_group.json.
usage: limiter_probe.py [--group N] [runs=60] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "faster-qwen3-tts_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from fq3hip import limiter as M
from loudness_probe import SAMPLES_PER_FRAME, alternate, speech_like

TILES = (256, 512, 1024, 2048, 4096)


def detector_figures():
    import _limit_ref as R
    rows, worst_u, worst_o = [], 0.0, 0.0
    for rate in R.RATES:
        for db in R.CEILINGS:
            for k, v in R.measured(rate, db).items():
                rows.append({"rate": rate, "ceiling_db": db, "signal": k, "under_read": round(v["under_read"], 6),
                             "output_overshoot": round(v["overshoot"], 6)})
                worst_u, worst_o = max(worst_u, v["under_read"]), max(worst_o, v["overshoot"])
    return {"worst_under_read": worst_u, "worst_overshoot": worst_o, "margin_on_overshoot": R.MARGIN,
            "yardstick": "32x windowed-sinc oversampling in float64, 48 taps each side, Kaiser beta 10", "signals": rows}


def main():
    runs = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 60
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "limiter_stage.json")
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    g = torch.Generator().manual_seed(3)
    cfg = qwen3_tts_0p6b()
    W = synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True)
    tok = HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=400, precision="bf16x2")
    d = M.design(24000)
    res = {"device": torch.cuda.get_device_name(0), "runs": runs, "in_rate": 24000, "attack": d.A, "hold": d.H, "halo": d.history,
           "default_tile": d.tile, "stage": [], "notes": [],
           "method": "HIP events around each call, every tile size and the vocoder alternating inside every repeat, medians"}
    cases = (("utterance, 370 frames", 370, torch.randint(0, cfg.codec.codebook_size, (370, 16), generator=g).cuda(), 0,
              "full decode of 370 frames", True),
             ("streaming chunk, 8 frames", 8, torch.randint(0, cfg.codec.codebook_size, (33, 16), generator=g).cuda(),
              tok.num_samples_total(33) - 8 * SAMPLES_PER_FRAME, "chunk decode: 25 context + 8 new frames, the tail of 8 produced", False))
    for name, frames, codes, first, what, whole in cases:
        n = frames * SAMPLES_PER_FRAME
        pcm = (speech_like(n, g) * 6.0).contiguous()
        fns = {}
        for tile in TILES:
            lim = M.Limiter(None, 24000, "cuda", tile=tile)
            if whole:
                def push(lim=lim):
                    lim.reset()
                    return lim.push(pcm, final=True)
            else:
                lim.push(pcm)                                       # the stream is running: the history is full from here on

                def push(lim=lim):
                    return lim.push(pcm)
            fns[f"tile {tile}"] = push
        fns["vocoder"] = lambda: tok.decode_tensor(codes, first)
        t = alternate(fns, runs)
        row = {"input": name, "n_in": n, "push": "reset + one final push" if whole else "one push of a running stream",
               "push_ms_by_tile": {str(tile): round(t[f"tile {tile}"], 4) for tile in TILES},
               "workgroups_by_tile": {str(tile): -(-n // tile) + 1 for tile in TILES},
               "push_ms": round(t[f"tile {d.tile}"], 4), "vocoder": what, "vocoder_ms": round(t["vocoder"], 4),
               "share_of_vocoder": round(t[f"tile {d.tile}"] / t["vocoder"], 5)}
        res["stage"].append(row)
        res["notes"].append(f"{name}: the limiter takes {100 * row['share_of_vocoder']:.2f} % of the vocoder's time for the same audio"
                            + ("" if row["share_of_vocoder"] <= 0.05 else " -- ABOVE 5 %"))
    res["notes"].append("push_ms and share_of_vocoder are taken at the default tile; an event pair around ONE short launch includes what "
                        "starting it costs, and the Python wrapper's output allocation lies inside it too")
    res["detector"] = detector_figures()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if "--group" in sys.argv[1:]:
        from leveller_probe import group_probe
        _i = sys.argv.index("--group")
        group_probe("limiter", int(sys.argv[_i + 1]), sys.argv[1:_i] + sys.argv[_i + 2:])
    else:
        main()
