"""Self-test of the continuation reference and its checkers (tests/_prefill_cont_ref.py), CPU only, on the case list of the GPU module
(tests/test_gpu_prefill_cont_reference.py): the unmutated float32 models pass every case -- which also shows that the inputs leave the
reference inside its own bound -- and each deliberate defect is rejected on every case it can change:
causal bound off by one in either direction, keys below start dropped, the key tile looked up by local instead of absolute index, the
V rows of a past tile swapped (attention); the RoPE position without start, the K / V write at the local row (norm kernel).
The defects are judged on the "which key" operands (an output dim is the probability of one key, so a dropped, doubled or misplaced
key moves an element by its whole value); the unmutated models on both operand sets."""
import pytest
import torch

import _prefill_cont_ref as R
import _prefill_attn_ref as P

DTS = ("f32", "bf16")
ATTN_MUTANTS = ("causal_minus", "causal_plus", "drop_past", "tile_local", "v_tile_swap")
NORM_MUTANTS = ("rope_local", "kv_local_row")


def test_case_list_is_what_the_issue_sets():
    assert set(R.BASE_CASES) == {(s, n) for s in (0, 1, 63, 64, 65, 130, 200, 448) for n in (1, 16, 17, 63, 64, 65, 130)}
    assert max(s + n for s, n in R.CASES) <= R.L_BIG and max(s for s, _ in R.CASES) <= 1100
    chosen = {R.splits(s, n) for s, n in R.CASES}
    reachable = {R.splits(s, n) for s in range(0, 1101, 8) for n in R.NS}
    assert chosen == reachable == {1, 2, 3, 4, 5}                # every split count the launcher can choose up to there
    ragged = [(s, n) for s, n in R.CASES if any(0 < hi - lo < blk[0][1] - blk[0][0] for blk in R.split_ranges(s, n, R.splits(s, n)) for lo, hi in blk)]
    assert (760, 17) in ragged
    assert any(hi <= lo for blk in R.split_ranges(200, 17, 5) for lo, hi in blk)                  # a forced split without a tile


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_float32_model_passes_every_attention_case(dt, kind):
    worst = 0.0
    for start, n in R.CASES:
        ref = R.case_reference(dt, kind, start, n)
        got = R.attn_model(dt, kind, start, n)
        for kernel, S in (("wave", 1), ("flash", R.splits(start, n))) if dt == "bf16" else (("wave", 1),):
            v = R.check_attn_cont(got, ref, start, dt, kernel, S, what=f"{dt} {kind} start {start} n {n} {kernel}")
            assert v, v.msg
            worst = max(worst, v.ratio)
    print(f"\nfloat32 model, {dt} {kind}: largest err / bound {worst:.3f}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mutant", ATTN_MUTANTS)
def test_attention_defects_are_rejected(dt, mutant):
    n_rej = 0
    for start, n in R.CASES:
        if not R.mutant_applies(mutant, start, n):
            continue
        ref = R.case_reference(dt, "which", start, n)
        got = R.attn_model(dt, "which", start, n, mutant=mutant)
        for kernel, S in (("wave", 1), ("flash", R.splits(start, n))) if dt == "bf16" else (("wave", 1),):
            assert not R.check_attn_cont(got, ref, start, dt, kernel, S), f"{mutant} passed: {dt} start {start} n {n} {kernel}"
            n_rej += 1
    assert n_rej >= 30                                           # (every defect applies to at least the 35 cases with start >= 64)


@pytest.mark.parametrize("dt", DTS)
def test_norm_model_passes_and_defects_are_rejected(dt):
    for i, (start, n) in enumerate(R.BASE_CASES):
        delta = R.ROPE_DELTAS[i % 3]
        rows = 64 * ((start + n + 63) // 64) + 64
        ref = R.norm_reference(dt, start, n, delta)
        v = R.check_norm_cont(*R.norm_model(dt, start, n, delta, rows), ref, start, n, dt, what=f"{dt} start {start} n {n}")
        assert v, v.msg
        for mutant in NORM_MUTANTS:
            if R.mutant_applies(mutant, start, n, delta):
                assert not R.check_norm_cont(*R.norm_model(dt, start, n, delta, rows, mutant=mutant), ref, start, n, dt), (mutant, start, n)
    # both ends of the RoPE clamp are met by the list
    assert min(s + d for (s, _), d in zip(R.BASE_CASES, (R.ROPE_DELTAS * 20))) < 0
    assert max(s + n - 1 + d for (s, n), d in zip(R.BASE_CASES, (R.ROPE_DELTAS * 20))) > R.ROPE_LEN - 1
