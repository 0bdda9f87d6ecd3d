"""Speaker check for many clips: what one group call costs beside that many single calls.

    python tools/speaker_probe.py [--out profiles/speaker_group.json]

Real speaker-encoder shapes (128 mel bins, n_fft 1024, hop 256, 512 / 1536 channels), seeded weights, clips of 3 s.  For 1, 8 and 32
clips: one ``fq3_refenc_speaker_group`` call against that many ``fq3_refenc_speaker`` calls, HIP events around each, the two
alternated, medians after a warm-up; beside them the bf16x2 vocoder's decode of the same group (38 frames = 3.04 s per clip, random
codes, sets of up to 16 as the lock-step batch vocodes them), of which the group call's time is reported as a share.  The launches
per call are DERIVED from the configuration by the structure of the two chains, not traced (the first group call after a finalize
found its two table-packing launches done by the finalize).  The float64 part repeats, on the small configuration and the clips of tests/test_gpu_speaker_group.py's kind, the figures
the test's bound is made of: the single call's and the group call's largest error against the oracle's float64 encoder.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]

from fq3hip.config import RefAudioConfig, tiny_ref_audio_config            # noqa: E402
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


def launches(rc):
    """(group call, single call): the front end, layer 0, the SE-Res2Net blocks, aggregation and pooling"""
    blocks, s = len(rc.enc_channels) - 2, rc.enc_res2net_scale
    group = 1 + 2 + blocks * (7 + 2 * (s - 1)) + 8
    single = 4 + 2 + blocks * (7 + 2 * (s - 1)) + 7
    return group, single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speaker_group.json"))
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    rc = RefAudioConfig()
    W = {k: v for k, v in synth_ref_audio_weights(rc, 2).items() if k.startswith("speaker_encoder.")}
    an = HipRefAudioAnalyzer(rc, W)
    clips = [an._wave(make_wave(3 * 24000, seed=50 + i)) for i in range(32)]
    n_group, n_single = launches(rc)
    from fq3hip.codec import HipSpeechTokenizer
    from fq3hip.config import qwen3_tts_0p6b
    from fq3hip.weights import synth_weights
    cfg = qwen3_tts_0p6b()
    tok = HipSpeechTokenizer(cfg.codec, synth_weights(cfg, 0, torch.bfloat16, parts=("codec",), codec_normalized=True), "cuda", max_frames=64,
                             precision="bf16x2")
    codes = torch.randint(0, cfg.codec.codebook_size, (32, 38, cfg.codec.num_quantizers), generator=torch.Generator().manual_seed(21)).cuda()

    def vocode(n):
        for lo in range(0, n, 16):
            part = codes[lo:min(n, lo + 16)]
            tok.decode_tensor(part[0], 0) if part.shape[0] == 1 else tok.decode_tensor_batch(part, 0)
    rows = []
    for n in (1, 8, 32):
        part = clips[:n]
        group = lambda: an.speaker_embeddings(part)
        single = lambda: [an.speaker_embedding(x) for x in part]
        for _ in range(3):
            group(), single(), vocode(n)
        tg, ts, tv = [], [], []
        for _ in range(args.reps):
            tg.append(timed(group))
            ts.append(timed(single))
            tv.append(timed(lambda: vocode(n)))
        g, s, v = statistics.median(tg), statistics.median(ts), statistics.median(tv)
        same = bool(torch.equal(an.speaker_embeddings(part), torch.stack(single())))
        rows.append(dict(clips=n, seconds_each=3.0, group_ms=round(g, 4), singles_ms=round(s, 4), singles_over_group=round(s / g, 3),
                         vocoder_bf16x2_ms=round(v, 4), group_share_of_vocoder=round(g / v, 3),
                         group_launches_derived=n_group, singles_launches_derived=n * n_single, bit_identical_to_singles=same))
        print(rows[-1])
    # the float64 figures behind the test's bound (small configuration)
    from oracle import refenc_oracle as RO
    tc = tiny_ref_audio_config()
    tw = synth_ref_audio_weights(tc, 2)
    ta = HipRefAudioAnalyzer(tc, tw)
    lengths = [2917, 2048, 2112, 257] + [300 + 97 * i for i in range(27)]
    tclips = [make_wave(n, seed=1000 + i) for i, n in enumerate(lengths)]
    ref = [RO.speaker_embedding(tw, tc, x, torch.float64)[0] for x in tclips]
    err = lambda got: max(float((g.double().cpu() - r).abs().max()) for g, r in zip(got, ref))
    e_single, e_group = err([ta.speaker_embedding(x) for x in tclips]), err(list(ta.speaker_embeddings(tclips)))
    # ... and at the real shapes, over the clips of the test's real-shape case
    rclips = [make_wave(n, seed=n) for n in (131 * 256 + 77, 5000)]
    ref = [RO.speaker_embedding(W, rc, x, torch.float64)[0] for x in rclips]
    r_single, r_group = err([an.speaker_embedding(x) for x in rclips]), err(list(an.speaker_embeddings(rclips)))
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, timing="HIP events around the Python call, median, the two forms alternated",
               rows=rows, float64=dict(config="tiny_ref_audio_config", clips=len(tclips), single_path_max_abs_err=e_single, bound=4 * e_single,
                                       group_max_abs_err=e_group),
               float64_real_shapes=dict(config="RefAudioConfig", clips=len(rclips), single_path_max_abs_err=r_single, bound=4 * r_single,
                                        group_max_abs_err=r_group),
               launches="derived from the configuration by the structure of the two chains, not traced",
               not_measured=["kernel-only times", "the end-to-end cost of verify=True in a 128-lane batch"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["float64"]))


if __name__ == "__main__":
    main()
