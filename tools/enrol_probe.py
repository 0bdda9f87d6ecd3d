"""Voice enrolment for many clips: what one encoder group call costs beside that many single calls.

    python tools/enrol_probe.py [--out profiles/enrol_group.json]

Real encoder shapes (64..1024 channels, strides 4 5 6 8, 8 x 512-d layers, window 250, 16 x 2048 codes), seeded weights.  For 1, 8
and 32 clips of 3 s and of 10 s: one ``fq3_refenc_encode_group`` call against that many ``fq3_refenc_encode`` calls in the same
process, HIP events around each, the two alternated, medians after a warm-up.  The launches per call are DERIVED from the
configuration by the structure of the two chains, not traced.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]

from fq3hip.config import RefAudioConfig                                    # noqa: E402
from fq3hip.refenc import HipRefAudioAnalyzer                               # noqa: E402
from fq3hip.weights import synth_ref_audio_weights                          # noqa: E402
from tests.test_refenc_oracle_pins import make_wave                         # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(rc, n_samples):
    """(group call, single call of a clip of n_samples): the front conv, the residual blocks and strided convs, the last conv, the
    transformer, the stride-2 conv with its padding, the projection and the RVQ.  The group call clears gap rows after every residual
    block and strided conv and the attention buffer once; the single call clears a strided conv's tail only where there is one."""
    res, layers = rc.num_residual_layers, rc.num_hidden_layers
    group = 1 + len(rc.ratios) * (3 * res + 2) + 1 + 1 + 8 * layers + 4
    single, t = 1 + len(rc.ratios) * (2 * res + 1) + 1 + 8 * layers + 4, n_samples
    for r in rc.ratios:
        single += 1 if t % r else 0
        t = -(-t // r)
    return group, single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enrol_group.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    rc = RefAudioConfig()
    W = {k: v for k, v in synth_ref_audio_weights(rc, 1).items() if k.startswith("encoder.")}
    an = HipRefAudioAnalyzer(rc, W)
    calls, call = [0], an._encode_group_call

    def counted(*a):                                                        # encode_many cuts a list where the call's cap on packed rows is reached
        calls[0] += 1
        call(*a)
    an._encode_group_call = counted
    rows = []
    for seconds in (3, 10):
        clips = [an._wave(make_wave(seconds * 24000, seed=50 + i)) for i in range(32)]
        n_group, n_single = launches(rc, seconds * 24000)
        for n in (1, 8, 32):
            part = clips[:n]
            group = lambda: an.encode_many(part)
            single = lambda: [an.encode(x) for x in part]
            for _ in range(2):
                group(), single()
            tg, ts = [], []
            for _ in range(args.reps):
                tg.append(timed(group))
                ts.append(timed(single))
            g, s = statistics.median(tg), statistics.median(ts)
            calls[0] = 0
            same = all(bool(torch.equal(a, b)) for a, b in zip(group(), single()))
            rows.append(dict(clips=n, seconds_each=float(seconds), group_ms=round(g, 4), singles_ms=round(s, 4), singles_over_group=round(s / g, 3),
                             group_calls=calls[0], group_launches_derived=calls[0] * n_group, singles_launches_derived=n * n_single,
                             bit_identical_to_singles=same))
            print(rows[-1], flush=True)
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, timing="HIP events around the Python call, median, the two forms alternated",
               rows=rows, launches="derived from the configuration by the structure of the two chains, not traced",
               not_measured=["kernel-only times", "the share of each stage", "real voices"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
