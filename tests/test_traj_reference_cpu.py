"""CPU: the host model of a seeded trajectory (tests/_traj_ref.py) is fit to be held against the device path with ``torch.equal``.

* Robust: for every (case, seed) of tests/test_gpu_long_trajectory.py the oracle with weights, prompt and noise in float64 gives the ids
  of the oracle in float32, over the whole run.  That is the condition under which exact equality is a fair demand on an fp32 device
  path; a combination that fails it is replaced by another seed, never tolerated.
* The runs meet the events: more than 64 distinct first-codebook ids, the end of the trailing text, the key blocks at 64, 128 and 192,
  the noise-ring refills at 64, 128 and 192.
* The ids notice the faults the long runs are there for: each host-side mutant changes them, no earlier than its event.

Measured once on the host model, and not asserted: with the unscaled text rows of cases A and B, a trailing text one row longer or
shorter changes no id in the whole run for any of their three combinations.  The pad switch is therefore checked on case S, whose text
rows are scaled like the prompt embeddings (see tests/_traj_ref.py).
"""
import pytest
import torch

import _traj_ref as T
from oracle import qwen3tts_oracle as O

KV_BLOCK = 64
NOISE_RING = 64


def _ids(c):
    return f"{c[0]}-{c[1]}"


@pytest.mark.parametrize("combo", T.COMBOS, ids=_ids)
def test_float32_model_equals_float64_model(combo):
    name, seed = combo
    a, b = T.case_codes(name, seed), T.case_codes(name, seed, torch.float64)
    assert a.shape == (T.CASES[name].frames, 16)
    assert torch.equal(a, b), f"case {name} seed {seed}: fp32 and fp64 part at (frame, group) {T.first_diff(a, b)}; choose another seed"


def test_gpu_set_is_small_and_seeds_are_the_checked_ones():
    assert len(T.COMBOS) <= 4 and len(set(T.COMBOS)) == len(T.COMBOS)
    assert {s for _n, s in T.COMBOS} <= {7, 20240607, 2 ** 63 + 5, 99, 123456789012345}
    a, b = T.CASES["A"], T.CASES["B"]
    assert a == (200, 33, 4, 40, 1.0, 1) and b == (140, 60, 0, 4, 0.8, 1)


@pytest.mark.parametrize("combo", [c for c in T.COMBOS if c[0] in "AB"], ids=_ids)
def test_long_runs_meet_the_events(combo):
    name, seed = combo
    c, codes = T.CASES[name], T.case_codes(name, seed)
    distinct = int(codes[:, 0].unique().numel())
    print(f"case {name} seed {seed}: {distinct} distinct first-codebook ids")
    assert distinct > 64                                              # a history kept as a short list of ids would overflow
    assert c.frames - 1 > c.trailing                                  # gen_step passes the trailing length: frames on tts_pad
    first, last = c.plen, c.plen + c.frames - 1                       # the key slots the decode steps write
    for edge in (KV_BLOCK, 2 * KV_BLOCK, 3 * KV_BLOCK):
        assert first < edge < last
    assert last < T.MAX_SEQ - 1                                       # and the position limit is not what ends the run
    assert c.frames > 2 * NOISE_RING                                  # at least two refills after the first fill
    if name == "A":
        assert c.frames > 3 * NOISE_RING and c.n_pad > 0


def test_short_case_meets_the_pad_switch():
    c = T.CASES["S"]
    assert 0 < c.trailing < c.frames - 2 and c.text_scale == 30 and c.n_pad > 0


def _mutant(name, seed, frames, prompt=None, **kw):
    cfg, W = T.tiny()
    c = T.CASES[name]
    return T.model_codes(cfg, W, prompt or T.case_prompt(cfg, name, seed), T.policy(frames, c.top_p), seed, frames, **kw)


def test_noise_rows_of_the_first_fill_again_after_a_refill_are_noticed():
    """A refill that passes a wrong frame counter: rows from frame 64 on are those of ``frame - 64``."""
    ref = T.case_codes("A", 7)
    d = T.first_diff(_mutant("A", 7, 100, frame_of=lambda f: f - NOISE_RING if f >= NOISE_RING else f), ref)
    print("noise of frame - 64 from frame 64 on: first difference at (frame, group)", d)
    assert d is not None and d[0] >= NOISE_RING


def test_noise_rows_shifted_by_one_frame_are_noticed():
    ref = T.case_codes("A", 7)
    d = T.first_diff(_mutant("A", 7, 30, frame_of=lambda f: f + 1), ref)
    print("noise shifted by one frame: first difference at (frame, group)", d)
    assert d is not None


@pytest.mark.parametrize("delta", [-1, 1], ids=["one_row_shorter", "one_row_longer"])
def test_pad_switch_one_frame_off_is_noticed(delta):
    """Loop step s adds text row s (or tts_pad) to the input that decides the ids of frame s + 1.  One row fewer: step trailing - 1 takes
    tts_pad, frames from ``trailing`` on can differ.  One row more (a text row again): step trailing does not take tts_pad, frames from
    ``trailing + 1`` on can differ."""
    cfg, _W = T.tiny()
    c, seed = T.CASES["S"], 99
    ref = T.case_codes("S", seed)
    tie, tam, tth, tpe = T.case_prompt(cfg, "S", seed)
    tth = tth[:, :-1] if delta < 0 else torch.cat([tth, tth[:, :1]], dim=1)
    d = T.first_diff(_mutant("S", seed, c.frames, prompt=(tie, tam, tth, tpe)), ref)
    print(f"trailing text {delta:+d} row: first difference at (frame, group)", d)
    assert d is not None and d[0] >= c.trailing + (1 if delta > 0 else 0)


def test_penalty_history_cut_to_its_last_64_ids_is_noticed(monkeypatch):
    """The history at loop step s holds s + 1 ids: the cut first bites at step 64, which decides frame 65."""
    name, seed = "A", 2 ** 63 + 5
    ref = T.case_codes(name, seed)
    whole = O.apply_repetition_penalty
    monkeypatch.setattr(O, "apply_repetition_penalty", lambda logits, history, penalty: whole(logits, history[-64:], penalty))
    d = T.first_diff(_mutant(name, seed, 120), ref)
    print("penalty history of the last 64 ids only: first difference at (frame, group)", d)
    assert d is not None and d[0] >= 65
