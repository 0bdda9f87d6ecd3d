"""GPU: long seeded decode runs against the host model of tests/_traj_ref.py (the CPU oracle fed numpy-drawn noise), not against one
another.  fp32 ids must equal the model's exactly -- tests/test_traj_reference_cpu.py holds every (case, seed) used here to
fp32 == fp64 on the host, and shows that the ids of these runs move when a noise refill takes a wrong frame counter, when the penalty
history forgets ids after 64, and (case S) when the switch from trailing text to ``tts_pad`` is a frame off.  The long runs write key
slots across the 64-key block edges at 64, 128 and 192 and refill the 64-frame noise ring three times.

Legs: single stream through the graph, direct launches, streaming in chunks of 12, the lock-step batch with a re-armed lane; and bf16
teacher-forced over 200 frames at the project's frozen K_ULP, where no floor is set on the matched count (that number would come from
the code under test) and the scores go to parity_long_trajectory.json, beside the full-depth parity notes.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _traj_ref as T
from test_gpu_fulldepth import _note
from test_gpu_seeded_decode import POLICY, Solo, _generate

K_ULP = 3.0                 # the project's frozen bound (tests/test_gpu_fulldepth.py)
MAX_SEQ, MAX_FRAMES = 256, 208
A1, B1, A2, S1 = T.COMBOS


@pytest.fixture(scope="module")
def solo():
    cfg, _W = T.tiny()
    return Solo(cfg, torch.float32, max_seq=MAX_SEQ, max_frames=MAX_FRAMES)


def _prompt(cfg, combo):
    return tuple(t.cuda() for t in T.case_prompt(cfg, *combo))


def _kw(combo):
    c = T.CASES[combo[0]]
    return T.policy(c.frames, c.top_p)


def _check(got, combo, what):
    """Exact equality with the host model; on a mismatch name the first differing id and the talker step that fed its frame."""
    name, seed = combo
    want, c = T.case_codes(name, seed), T.CASES[name]
    got = got.cpu()
    assert got.shape == want.shape, f"{what}: case {name} seed {seed}: {tuple(got.shape)} ids, the model has {tuple(want.shape)}"
    d = T.first_diff(got, want)
    if d is not None:
        f, g = d
        step = f - 1            # loop step f - 1 (gen_step f - 1, key slot plen + f - 1) produced the hidden and the first id of frame f
        raise AssertionError(f"{what}: case {name} seed {seed}: first difference at frame {f} group {g} (device {int(got[f, g])}, model "
                             f"{int(want[f, g])}); fed by gen_step {step} at position {c.plen + step}; trailing text ends at {c.trailing}, "
                             f"{int((got != want).any(dim=1).sum())} of {c.frames} frames differ")
    assert torch.equal(got, want)


@pytest.mark.parametrize("combo", T.COMBOS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_single_stream_equals_host_model(solo, combo):
    _check(_generate(solo, _prompt(solo.cfg, combo), combo[1], **_kw(combo)), combo, "fast_generate")


@pytest.mark.parametrize("combo", [A1, S1], ids=lambda c: f"{c[0]}-{c[1]}")
def test_direct_launches_equal_host_model(solo, combo):
    _check(_generate(solo, _prompt(solo.cfg, combo), combo[1], parity_mode=True, **_kw(combo)), combo, "fast_generate(parity_mode=True)")


@pytest.mark.parametrize("combo", [A1, S1], ids=lambda c: f"{c[0]}-{c[1]}")
def test_streaming_equals_host_model(solo, combo):
    from fq3hip.streaming import fast_generate_streaming
    tie, tam, tth, tpe = _prompt(solo.cfg, combo)
    chunks = [c.cpu() for c, _tm in fast_generate_streaming(solo.talker, tie, tam, tth, tpe, solo.config, solo.pg, solo.tg, chunk_size=12,
                                                            seed=combo[1], **_kw(combo))]
    assert all(c.shape[0] == 12 for c in chunks[:-1])
    _check(torch.cat(chunks), combo, "fast_generate_streaming(chunk_size=12)")


def test_batch_lanes_equal_host_model(solo):
    """Two lanes, four requests: A and B start; the short request takes the lane B frees, and A under another seed re-arms the lane the
    short one frees while the first A is still running.  Every request against its own model run."""
    from fq3hip.batching import BatchDecoder, BatchRequest
    lanes = [Solo(solo.cfg, torch.float32, max_seq=MAX_SEQ, max_frames=MAX_FRAMES, share=solo) for _ in range(2)]
    dec = BatchDecoder([l.eng for l in lanes], predictor_policy=dict(POLICY))
    order = [A1, B1, S1, A2]
    assert T.CASES["B"].frames + T.CASES["S"].frames < T.CASES["A"].frames
    batch = []
    for i, combo in enumerate(order):
        tie, tam, tth, tpe = _prompt(solo.cfg, combo)
        batch.append(BatchRequest(i, solo.talker, tie, tam, tth, tpe, solo.config, _kw(combo), seed=combo[1]))
    got = {}
    for rid, codes, timing in dec.run(batch):
        assert "error" not in timing, timing
        got[rid] = codes
    assert sorted(got) == list(range(len(order)))
    for i, combo in enumerate(order):
        _check(got[i], combo, f"batch request {i}")


def test_bf16_teacher_forced_over_200_frames():
    """The oracle with bf16 weights decodes case A's prompt greedily (penalty 1.0) for 200 frames, here, in this process; the device
    loop replays those frames teacher-forced.  A device decision may differ from the oracle's only where the oracle's own top-2 margin
    is at most K_ULP bf16 ulps of the winning logit, at frame 199 as at frame 0, through the graph and through direct launches alike."""
    from fq3hip.engine import Fq3Engine
    from fq3hip.weights import synth_weights
    from oracle import qwen3tts_oracle as O
    from oracle import teacher_forced as TF
    cfg, _W = T.tiny()
    name, seed = A1
    c, dtype = T.CASES[name], torch.bfloat16
    frames = c.frames
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor"))
    tie, tam, tth, tpe = T.case_prompt(cfg, name, seed, dtype)
    orc = O.OracleTTS(cfg, W, max_seq_len=MAX_SEQ)
    orc.pred_sampling = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0)
    sp = O.SamplingParams(max_new_tokens=frames, **{**O.GREEDY, "min_new_tokens": frames})
    with torch.inference_mode():
        codes = orc.generate(tie, tam, tth, tpe, sp, record_margins=True)
    assert codes.shape == (frames, 16)
    case = dict(codes=codes.numpy().astype(np.int32), t_margin=np.asarray(orc.margins, np.float32), t_top1=np.asarray(orc.top1, np.float32),
                p_margin=np.asarray(orc.pred_margins, np.float32).reshape(frames, 15),
                p_top1=np.asarray(orc.pred_top1, np.float32).reshape(frames, 15))
    eng = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=MAX_SEQ, max_frames=MAX_FRAMES)
    eng.set_predictor_sampling(do_sample=False, top_k=0, top_p=1.0, temperature=1.0)
    res, decs = {}, {}
    for graph in (True, False):
        tag = "graph" if graph else "direct"
        decs[tag] = TF.forced_decisions(eng, cfg, tie, tth, tpe, case["codes"], graph=graph, n_pad=c.n_pad)
        res[tag] = dict(TF.score(decs[tag], case, K_ULP), near_ties=TF.near_ties(case, K_ULP))
        print(f"[parity] long trajectory bf16 {tag}: {res[tag]}")
    _note("tiny_bf16_caseA_200", res, "parity_long_trajectory.json")
    eng.close()
    for tag, s in res.items():
        bad = np.argwhere(decs[tag] != case["codes"].astype(np.int64))
        assert s["unexplained"] == 0, (tag, s, "mismatches at (frame, group):", bad[:8].tolist())
    assert np.array_equal(decs["graph"], decs["direct"]), "graph replay and direct launches decide differently"
