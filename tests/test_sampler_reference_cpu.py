"""The float64 sampler reference and its checker (tests/_sampler_ref.py) checked on the CPU, without a GPU:

* the reference equals oracle.sample_logits / apply_repetition_penalty (Torch on the CPU) on every stateless case of the GPU suite,
  by the checker's own rule (equal on decided cases, one of the three scalings' tokens otherwise), and reproduces `token` of every
  case of tests/golden/sampler.npz and the penalised vectors stored there;
* the signed-zero cases, where Torch's choice of the k-th value among +-0 is arbitrary, are checked against a scalar loop instead;
* every family's list stays inside the cap on undecided cases;
* the checker rejects every named mutant on at least one DECIDED case of the lists.
"""
import os

import numpy as np
import pytest
import torch

import _sampler_ref as R
from oracle import qwen3tts_oracle as O

TDT = {"bf16": torch.bfloat16, "f32": torch.float32}


def oracle_token(c: R.Case) -> int:
    x = torch.from_numpy(c.logits).to(TDT[c.dt])
    if c.seen is not None:
        x = O.apply_repetition_penalty(x.clone(), torch.from_numpy(np.flatnonzero(c.seen)), c.cfg.rep_penalty)
    ids = np.arange(c.V)
    sup = ((ids >= c.cfg.sup_lo) & (ids < c.cfg.sup_hi) & (ids != c.cfg.keep_id)) | (ids == c.cfg.sup_extra)
    noise = torch.from_numpy(c.noise).to(TDT[c.dt]) if c.noise is not None else None
    return int(O.sample_logits(x, temperature=c.cfg.temperature, top_k=c.cfg.top_k, top_p=c.cfg.top_p, do_sample=c.cfg.do_sample,
                               suppress_mask=torch.from_numpy(sup), noise=noise))


def test_reference_equals_the_oracle_on_every_stateless_case():
    cases, vs = R.verdicts("stateless")
    n = 0
    for c, v in zip(cases, vs):
        if "zero" in c.tags and c.cfg.do_sample:
            continue
        msg = R.check(v, oracle_token(c), c.name)
        assert msg == "", msg
        n += 1
    assert n > 1000


def test_penalised_vector_equals_the_oracle():
    cases, _ = R.verdicts("stateless")
    n = 0
    for c in cases:
        if c.seen is None or c.cfg.do_sample:
            continue
        want = O.apply_repetition_penalty(torch.from_numpy(c.logits).to(TDT[c.dt]), torch.from_numpy(np.flatnonzero(c.seen)), c.cfg.rep_penalty)
        got = torch.from_numpy(R.penalised(c)).to(TDT[c.dt])
        assert torch.equal(got, want), c.name
        n += 1
    assert n >= 7 * len(R.VS) * 2


def test_signed_zero_cases_against_a_scalar_loop():
    """top-k with ties kept, written out: the k-th largest by float comparison, everything strictly below it dropped."""
    cases, vs = R.verdicts("stateless")
    n = 0
    for c, v in zip(cases, vs):
        if "zero" not in c.tags or not c.cfg.do_sample:
            continue
        T = R.f32(c.cfg.temperature)
        x = [float(R.rnd(float(t) / T, c.dt)[0]) for t in c.logits]
        kth = sorted(x, reverse=True)[min(c.cfg.top_k, c.V) - 1]
        assert kth == 0.0
        keep = [i for i in range(c.V) if not x[i] < kth]
        got, _ = R.filtered(c)
        assert list(np.flatnonzero(~np.isneginf(got))) == keep, c.name
        assert any(np.signbit(got[i]) for i in keep) and any(not np.signbit(got[i]) and got[i] == 0.0 for i in keep)
        if R.f32(c.cfg.top_p) >= 1.0:                      # the noise favours a -0.0 entry, which the key-ordered filter loses
            assert v.decided and np.signbit(got[v.token]) and got[v.token] == 0.0, c.name
            assert R.sample(c, "topk_key").token != v.token
        n += 1
    assert n == 4 * len(R.VS) * 2


def test_reference_reproduces_the_golden_file(golden_dir):
    g = np.load(os.path.join(golden_dir, "sampler.npz"), allow_pickle=True)
    for i, case in enumerate(g["cases"]):
        dt = "bf16" if case["bf16"] else "f32"
        V = int(case["V"])
        keep = int(case["eos"]) if not case["sup_eos"] else -1
        cfg = R.Cfg(float(case["temperature"]), int(case["top_k"]), float(case["top_p"]), bool(case["do_sample"]), 1.0, max(0, V - 1024), V, keep)
        c = R.Case(f"golden {i}", dt, V, R.rnd(case["logits"], dt), cfg, R.rnd(case["noise"], dt))
        msg = R.check(R.sample(c), int(case["token"]), c.name)
        assert msg == "", msg
    for i, case in enumerate(g["penalty"]):
        dt = "bf16" if case["bf16"] else "f32"
        x = R.rnd(case["logits"], dt)
        seen = np.zeros(x.shape[0], np.uint8)
        seen[np.asarray(case["hist"]).reshape(-1)] = 1
        c = R.Case(f"golden penalty {i}", dt, x.shape[0], x, R.Cfg(rep_penalty=float(case["p"])), seen=seen)
        assert np.array_equal(R.penalised(c), R.rnd(case["out"], dt)), c.name
        assert R.sample(c).token == int(np.argmax(R.rnd(case["out"], dt)))


@pytest.mark.parametrize("which", ["stateless", "graph"])
def test_undecided_share_is_within_the_cap(which):
    cases, vs = R.verdicts(which)
    fam = {}
    for c, v in zip(cases, vs):
        if v is not None:
            fam.setdefault(R.family_of(c), []).append(v)
    for name, lst in fam.items():
        share = R.undecided_share(lst)
        print(f"{name}: {len(lst)} cases, {sum(v.decided for v in lst)} decided, undecided share {share:.4f}")
        assert share <= R.UNDECIDED_CAP, (name, share)
    # the nucleus cases alone (the path whose cut can move) stay inside the cap too
    nuc = [v for c, v in zip(cases, vs) if v is not None and "nucleus" in c.tags and "tie" not in c.tags]
    assert R.undecided_share(nuc) <= R.UNDECIDED_CAP


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_checker_rejects_the_mutant_on_a_decided_case(mut):
    graph_only = mut in ("min_new_le", "noise_nomod", "noise_G")
    cases, vs = R.verdicts("graph" if graph_only else "stateless")
    for c, v in zip(cases, vs):
        if v is None or not v.decided:
            continue
        tok = (R.graph_sample(c, mut) if graph_only else R.sample(c, mut)).token
        if R.check(v, tok, c.name) != "":
            return
    pytest.fail(f"no decided case of the list rejects the mutant {mut}: the list is incomplete")
