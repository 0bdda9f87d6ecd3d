"""Host model of a seeded decode trajectory: the CPU oracle (oracle/qwen3tts_oracle.py) fed the noise rows of the seeded-noise
contract as tests/_noise_ref.py restates it in numpy.  Together they compute what ``fast_generate(seed=...)`` must return and share no
code with the device path.  The reference of tests/test_traj_reference_cpu.py and tests/test_gpu_long_trajectory.py.

The policy is that of tests/test_gpu_seeded_decode.py (T 0.9, top-k 20, repetition penalty 1.05, a sampling predictor at T 0.9 / top-k 20,
``min_new = max_new = frames``), and ``host_prompt`` builds what that file's ``_prompt`` builds, on the host.

With ``min_new = max_new = frames`` EOS is suppressed at every sampled frame, so a run of n frames is the first n frames of any longer
run of the same (prompt, policy, seed): the mutants of the CPU test run only as far as they need to.
"""
import collections

import numpy as np
import torch

import _noise_ref as NR

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_prompt, synth_weights
from oracle import qwen3tts_oracle as O

PRED_POLICY = dict(do_sample=True, top_k=20, top_p=1.0, temperature=0.9)
MAX_SEQ = 256

Case = collections.namedtuple("Case", "frames plen n_pad trailing top_p text_scale")
# A: positions 33..233 cross the 64-key blocks at 64, 128 and 192; the trailing text runs out at frame 40; three ring refills
# B: nucleus sampling; starts four rows below the first block boundary
# S: a short request (the lane of the batch test that frees early) whose trailing text and tts_pad are scaled like the embeddings.  The
#    synthetic text rows are 0.02 N(0, 1) beside a sum of sixteen N(0, 1) embedding rows: unscaled, as in A and B, a pad switch one frame
#    early or late changes no id in 200 frames (measured on the host model for every combination below), so A and B cannot see one.
#    S can: the switch is at frame 10 and both one-row mutants change its ids (tests/test_traj_reference_cpu.py).
CASES = {"A": Case(200, 33, 4, 40, 1.0, 1), "B": Case(140, 60, 0, 4, 0.8, 1), "S": Case(30, 20, 2, 10, 1.0, 30)}
# the (case, seed) combinations the GPU tests use; tests/test_traj_reference_cpu.py holds each to fp32 == fp64
COMBOS = [("A", 7), ("B", 20240607), ("A", 2 ** 63 + 5), ("S", 99)]


def policy(frames, top_p=1.0):
    return dict(temperature=0.9, top_k=20, top_p=top_p, do_sample=True, repetition_penalty=1.05, min_new_tokens=frames,
                max_new_tokens=frames)


def host_prompt(cfg, dtype, seed, plen, n_pad=0, trailing=4, text_scale=1):
    """(embeds x 30 [1, plen, H], mask with its first ``n_pad`` entries zeroed, trailing text [1, trailing, H], tts_pad [1, 1, H]); the
    last two times ``text_scale``."""
    tie, tam, tth, tpe, _ = synth_prompt(cfg, plen, trailing, 0, dtype=dtype, seed=seed)
    tam = tam.clone()
    tam[0, :n_pad] = 0
    return (tie * 30).to(dtype), tam, (tth * text_scale).to(dtype), (tpe * text_scale).to(dtype)


def case_prompt(cfg, name, seed, dtype=torch.float32):
    c = CASES[name]
    return host_prompt(cfg, dtype, seed & 0xFFFF, c.plen, c.n_pad, c.trailing, c.text_scale)


def noise(cfg, seed, frames, frame_of=lambda f: f):
    """(talker_noise [frames + 1, V], pred_noise [frames, G - 1, Vp]) in fp32.  ``frame_of`` maps the frame a row is used at to the
    frame it is drawn for: the identity is the contract, anything else a mutant."""
    V, G1, Vp = cfg.talker.vocab_size, cfg.num_code_groups - 1, cfg.predictor.vocab_size
    tn = np.stack([NR.first_row(seed, V)] + [NR.talker_row(seed, frame_of(f), V) for f in range(frames)])
    pn = np.stack([NR.pred_rows(seed, frame_of(f), G1, Vp) for f in range(frames)])
    return torch.from_numpy(tn), torch.from_numpy(pn)


def model_codes(cfg, W, prompt, policy, seed, frames, dtype=torch.float32, frame_of=lambda f: f):
    """The ids [frames, G] of a seeded run.  ``W`` and ``prompt`` are fp32; ``dtype=torch.float64`` casts weights, prompt and noise."""
    tn, pn = noise(cfg, seed, frames, frame_of)
    tie, tam, tth, tpe = prompt
    orc = O.OracleTTS(cfg, {k: v.to(dtype) for k, v in W.items()}, max_seq_len=MAX_SEQ)
    orc.pred_sampling = dict(PRED_POLICY)
    with torch.inference_mode():
        codes = orc.generate(tie.to(dtype), tam, tth.to(dtype), tpe.to(dtype), O.SamplingParams(**policy), tn.to(dtype), pn.to(dtype))
    assert codes is not None and codes.shape == (frames, cfg.num_code_groups), None if codes is None else codes.shape
    return codes


_cfg_w = []
_codes = {}


def tiny():
    """(cfg, fp32 weights) of the tiny config, built once."""
    if not _cfg_w:
        cfg = tiny_test_config()
        _cfg_w.append((cfg, synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor"))))
    return _cfg_w[0]


def case_codes(name, seed, dtype=torch.float32):
    """``model_codes`` of a (case, seed) on the tiny config, computed once per process and never written to by its users."""
    key = (name, seed, dtype)
    if key not in _codes:
        cfg, W = tiny()
        c = CASES[name]
        _codes[key] = model_codes(cfg, W, case_prompt(cfg, name, seed), policy(c.frames, c.top_p), seed, c.frames, dtype)
    return _codes[key]


def first_diff(a, b):
    """(frame, group) of the first differing id of two [n, G] id arrays over their common frames, or None."""
    n = min(a.shape[0], b.shape[0])
    bad = (torch.as_tensor(a)[:n] != torch.as_tensor(b)[:n]).nonzero()
    return None if bad.numel() == 0 else (int(bad[0, 0]), int(bad[0, 1]))
