"""CPU: the float64 GEMV reference of tests/_gemv_ref.py against scalar loops, a float32 model of every kernel's summation order inside
every bound and above every exact-fraction floor at every case of the GPU suite, and the checker against the named mutants."""
import math

import pytest
import torch

import _gemm_ref as G
import _gemv_ref as R
from _gemv_ref import (Case, EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, PRO_COMBINE, PRO_NORM, PRO_PLAIN, F64)


def r1(v, dt):
    return float(G.rnd(torch.tensor(v, dtype=F64), dt))


def scalar_reference(c: Case):
    """Plain Python loops over Python floats (float64), roundings through r1."""
    R.build(c)
    dt, K, N = c.dt, c.K, c.N
    W = c.W.tolist()
    ys, xns = [], []
    for t in range(c.B):
        if c.pro == PRO_COMBINE:
            xn = []
            for k in range(K):
                head, d = divmod(k, R.HD)
                ms = [float(c.m[t, head, s, 0]) for s in range(c.n_part)]
                M = max(ms)
                num = den = 0.0
                for s in range(c.n_part):
                    w = math.exp(ms[s] - M)
                    num += w * float(c.num[t, head, s, 0, d])
                    den += w * float(c.l[t, head, s, 0])
                xn.append(r1(num / den if den > 0 else 0.0, dt))
        elif c.pro == PRO_NORM:
            x = c.x[t].tolist()
            ss = 0.0
            for v in x:
                ss += v * v
            rs = 1.0 / math.sqrt(ss / K + R.EPS)
            xn = [r1(r1(x[k] * rs, dt) * float(c.gain[k]), dt) for k in range(K)]
        else:
            xn = c.x[t].tolist()
        xns.append(xn)

        def dot(row):
            a = 0.0
            for k in range(K):
                a += W[row][k] * xn[k]
            return a
        y = []
        for n in range(N):
            if c.epi == EPI_SWIGLU:
                g, u = r1(dot(n), dt), r1(dot(n + c.up_off), dt)
                y.append(r1(r1(g / (1.0 + math.exp(-g)), dt) * u, dt))
            else:
                v = r1(dot(n) + (float(c.bias_v[n]) if c.bias_v is not None else 0.0), dt)
                if c.epi == EPI_RESIDUAL:
                    v = r1(v + float(c.res[t, n]), dt)
                y.append(v)
        ys.append(y)
    return torch.tensor(ys, dtype=F64), torch.tensor(xns, dtype=F64)


TINY = [
    Case("gemv", "bf16", PRO_NORM, EPI_SWIGLU, 3, 24, 2, up_gap=2, seed=1),
    Case("gemv", "f32", PRO_NORM, EPI_STORE, 5, 16, 2, bias=True, seed=2),
    Case("batch", "bf16", PRO_PLAIN, EPI_RESIDUAL, 5, 40, 3, bias=True, seed=3),
    Case("gemv", "f32", PRO_PLAIN, EPI_STORE, 2, 8, 1, seed=4),
    Case("gemv", "bf16", PRO_COMBINE, EPI_RESIDUAL, 3, 128, 2, bias=True, n_part=3, rep=1, seed=5),
    Case("gemv", "f32", PRO_COMBINE, EPI_RESIDUAL, 2, 256, 1, n_part=8, rep=2, seed=6),
]


@pytest.mark.parametrize("c", TINY, ids=lambda c: c.name)
def test_reference_equals_scalar_loops(c):
    ref = R.reference(c)
    y, xn = scalar_reference(c)
    # the loop's float64 sums run in another order: equal after the rounding except where a sum sits within 1e-12 of a tie
    assert torch.equal(xn, ref.xn) or float((xn - ref.xn).abs().max()) <= 1e-12 * float(ref.xn.abs().max())
    close = (y - ref.y).abs() <= G.ulp(ref.y, c.dt) * (1.0 if c.dt == "bf16" else 2.0)
    assert bool(close.all()) and float((y == ref.y).double().mean()) >= (0.9 if c.dt == "bf16" else 0.0), (y, ref.y)
    if c.pro == PRO_COMBINE:
        # the slot image holds the head-major values: group g, slot s, head hh of the group
        g, s, hh = (c.K // R.HD // c.rep) - 1, c.n_part - 1, c.rep - 1
        head = g * c.rep + hh
        assert torch.equal(c.slots[0, g, s, hh, :R.HD], c.num[0, head, s, 0])
        assert float(c.slots[0, g, s, hh, R.HD]) == float(c.m[0, head, s, 0]) and float(c.slots[0, g, s, hh, R.HD + 1]) == float(c.l[0, head, s, 0])
        assert bool(torch.isnan(c.slots[:, :, c.n_part:]).all())


ALL = R.all_cases()


def test_case_list_covers_the_issue():
    names = {(c.kind, c.dt, c.pro, c.epi) for c in ALL}
    assert len(ALL) > 800 and len(names) == 2 * 5 + 2 * 4 + 2 + 2 + 1
    gemv = [c for c in ALL if c.kind == "gemv"]
    assert {c.K for c in gemv} >= set(R.GEMV_K) | set(R.COMBINE_K) and {c.N for c in gemv} >= set(R.GEMV_N_SMALL + R.GEMV_N_BIG)
    assert {(c.n_part, c.rep) for c in gemv if c.pro == PRO_COMBINE} == {(p, r) for p in R.COMBINE_PARTS for r in R.COMBINE_REPS}
    batch = [c for c in ALL if c.kind == "batch"]
    assert {c.B for c in batch} == set(R.BATCH_B) and {c.group for c in batch} >= set(R.BATCH_GROUPS)
    assert any(c.group and c.B % c.group for c in batch) and any(c.K == 6144 for c in batch if c.dt == "f32")
    for kind, Bs in (("norm", R.MFMA_B), ("plain", R.MFMA_B)):
        assert {c.B for c in ALL if c.kind == kind} == set(Bs)
    assert {c.K for c in ALL if c.kind == "plain"} == set(R.PLAIN_K) and {c.K // 128 for c in ALL if c.kind == "norm"} == set(R.NORM_KSTEPS)
    for c in ALL:                                   # every bias / no-bias and up_off = N / > N variant appears per family
        assert c.K % 8 == 0
    for kind in ("gemv", "batch", "plain"):
        assert {c.bias for c in ALL if c.kind == kind} == {False, True}
    assert {c.up_gap > 0 for c in ALL if c.epi == EPI_SWIGLU and c.kind == "gemv"} == {False, True}


def _models(c):
    if c.kind in ("gemv", "batch"):
        return [("valu", R.model_valu(c))]
    if c.kind == "norm":
        return [("mfma4", R.model_mfma(c, 4))]
    if c.kind == "plain":
        return [("mfma", R.model_mfma(c))]
    return [("rmsnorm", R.prologue32(R.build(c)))]


@pytest.mark.parametrize("part", range(8))
def test_float32_models_pass_at_every_gpu_case(part):
    """The proof that the bounds and the exact-fraction rule are satisfiable without the code under test: a float32 emulation of each
    kernel's summation order (lane-strided fma chain + wave tree; four or eight K shares of 16x16x32 blocks added in fixed order), with
    an fp32 rs in the norm, passes the checker at every case -- 0.99 exact over the scored rows of every case of MIN_SCORED elements,
    and the pool of the smaller ones; every input is tie-free."""
    pool = R.ExactPool()
    for c in ALL[part::8]:
        ref = R.reference(c)
        if c.dt == "bf16":
            assert float(ref.ex.max()) == 0.0, f"{c.name}: the prologue input is not tie-free"
        for name, got in _models(c):
            if c.kind == "rmsnorm":
                v = R.check_xn(got, ref, c, what=f"{c.name} [{name}]")
            else:
                v = R.check_y(got, ref, c, what=f"{c.name} [{name}]")
                pool.add(v)
                vx = R.check_xn(R.prologue32(c), ref, c)
                assert vx.ok, vx.msg
            assert v.ok, v.msg
        c.W = c.x = c.res = c.slots = c.num = None              # (the list is shared: drop the operands again)
    assert pool.n >= 200
    pool.check(f"float32 models, part {part}")


def test_scored_rows_and_pool():
    c = Case("gemv", "bf16", PRO_NORM, EPI_SWIGLU, 24, 64, 1, up_gap=3, seed=1)
    ok = R.scored_rows(c)
    assert [n for n in range(24) if not ok[n]] == [1, 6, 9, 14, 17, 22]          # gate rows 1, 9, 17; up rows n + 27 = 33, 41, 49
    assert bool(R.scored_rows(Case("gemv", "bf16", PRO_PLAIN, EPI_STORE, 24, 64, 1, cancel=False)).all())
    pool = R.ExactPool()
    v = G.Verdict(True, 0.0, 1.0, (), "")
    v.n_scored, v.n_exact = 100, 97
    pool.add(v)
    assert pool.n == 100 and abs(pool.floor - (0.99 - 3 * math.sqrt(0.0099 / 100))) < 1e-12
    pool.check()                                             # 0.97 >= 0.9602
    v.n_exact = 95
    pool.add(v)
    with pytest.raises(AssertionError):
        pool.check()                                         # 0.96 < 0.9689
    v.n_scored = R.MIN_SCORED                                # a case that answers for itself is not pooled
    pool.add(v)
    assert pool.n == 200


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
def _big(kind, pro, epi, **kw):
    """A bf16 case of MIN_SCORED scored elements or more, with bias: one-ulp defects stay inside the 2-ulp bound, the exact fraction
    over the scored rows rejects them."""
    shape = dict(gemv=(1029, 2), batch=(1029, 4), norm=(48, 128), plain=(24, 128))[kind]
    K = kw.pop("K", {"gemv": 520, "batch": 264, "norm": 1024, "plain": 768}[kind])
    return Case(kind, "bf16", pro, epi, shape[0], K, shape[1], bias=epi != EPI_SWIGLU, up_gap=16 if epi == EPI_SWIGLU else 0, **kw)


def _mutant_cases():
    out = []
    add = lambda mutant, c, by=("y",): out.append((mutant, c, by))
    for dt in R.DTS:
        add("drop_last_chunk", Case("gemv", dt, PRO_PLAIN, EPI_STORE, 5, 520, 2, seed=1))
        add("drop_last_chunk", Case("gemv", dt, PRO_PLAIN, EPI_RESIDUAL, 1029, 3080, 2, seed=2))
        add("token_shift", Case("batch", dt, PRO_PLAIN, EPI_STORE, 5, 2056, 5, seed=3))
        add("token_shift", Case("batch", dt, PRO_NORM, EPI_STORE, 3, 1032, 9, seed=4))
        for K in (264, 520, 1032):
            add("norm_pad512", Case("gemv", dt, PRO_NORM, EPI_STORE, 5, K, 2, seed=K), ("y", "xn"))
        add("no_eps", Case("gemv", dt, PRO_NORM, EPI_SWIGLU, 5, 520, 2, seed=10), ("y", "xn"))       # token 1: mean(x^2) below eps
        for gap in (0, 3):
            c = Case("gemv", dt, PRO_NORM, EPI_SWIGLU, 5, 520, 2, up_gap=gap, seed=40 + gap)
            add("up_off_by_one", c)
            add("swap_gate_up", c)
    for K in (256, 1024, 6144):
        add("drop_wave_share", Case("plain", "bf16", PRO_PLAIN, EPI_RESIDUAL, 24, K, 17, seed=5))
        add("tile_copy", Case("plain", "bf16", PRO_PLAIN, EPI_STORE, 16, K, 33, seed=6))
    add("drop_wave_share", Case("norm", "bf16", PRO_NORM, EPI_SWIGLU, 16, 2048, 17, seed=7))
    add("tile_copy", Case("norm", "bf16", PRO_NORM, EPI_STORE, 24, 512, 80, seed=8))
    add("token_shift", Case("norm", "bf16", PRO_NORM, EPI_STORE, 24, 512, 80, seed=8))
    add("no_eps", Case("norm", "bf16", PRO_NORM, EPI_STORE, 16, 256, 5, seed=9), ("y", "xn"))
    c = Case("norm", "bf16", PRO_NORM, EPI_SWIGLU, 16, 512, 17, up_gap=16, seed=42)
    add("up_off_by_one", c)
    add("swap_gate_up", c)
    add("gain_before_round", Case("gemv", "bf16", PRO_NORM, EPI_STORE, 5, 1024, 2, seed=11), ("xn",))
    add("gain_before_round", Case("rmsnorm", "bf16", PRO_NORM, EPI_STORE, 1, 520, 5, seed=12), ("xn",))
    # the one-ulp defects, at every epilogue that has the rounding in question, VALU and matrix-core alike
    every = [("gemv", PRO_NORM, EPI_STORE, {}), ("gemv", PRO_NORM, EPI_SWIGLU, {}), ("gemv", PRO_PLAIN, EPI_STORE, {}),
             ("gemv", PRO_PLAIN, EPI_RESIDUAL, dict(K=3080)), ("gemv", PRO_COMBINE, EPI_RESIDUAL, dict(K=1024, n_part=3, rep=2)),
             ("batch", PRO_NORM, EPI_STORE, {}), ("batch", PRO_PLAIN, EPI_RESIDUAL, {}), ("norm", PRO_NORM, EPI_STORE, {}),
             ("norm", PRO_NORM, EPI_SWIGLU, {}), ("plain", PRO_PLAIN, EPI_STORE, {}), ("plain", PRO_PLAIN, EPI_RESIDUAL, {}),
             ("plain", PRO_PLAIN, EPI_RESIDUAL, dict(K=6144))]
    for i, (kind, pro, epi, kw) in enumerate(every):
        c = _big(kind, pro, epi, seed=60 + i, **kw)
        add("trunc", c)
        if epi != EPI_SWIGLU:
            add("bias_after_round", c)
        if epi == EPI_RESIDUAL:
            add("res_before_round", c)
    return out


MUTANT_CASES = _mutant_cases()


def test_every_named_mutant_has_a_case():
    assert {m for m, _, _ in MUTANT_CASES} == set(R.MUTANTS)
    with pytest.raises(ValueError):
        R.reference(TINY[3], "no_such_mutant")
    for m in ("bias_after_round", "res_before_round"):          # every epilogue with a bias / a residual, VALU and matrix-core
        kinds = {(c.kind, c.epi) for mm, c, _ in MUTANT_CASES if mm == m}
        want = {("gemv", EPI_RESIDUAL), ("batch", EPI_RESIDUAL), ("plain", EPI_RESIDUAL)}
        assert kinds >= (want if m == "res_before_round" else want | {("gemv", EPI_STORE), ("batch", EPI_STORE), ("norm", EPI_STORE), ("plain", EPI_STORE)})


@pytest.mark.parametrize("mutant,c,by", MUTANT_CASES, ids=[f"{m}-{c.name}" for m, c, _ in MUTANT_CASES])
def test_checker_rejects_mutant(mutant, c, by):
    ref = R.reference(c)
    assert R.check_y(ref.y, ref, c).ok and R.check_xn(ref.xn, ref, c).ok
    mut = R.reference(c, mutant)
    vy, vx = R.check_y(mut.y, ref, c), R.check_xn(mut.xn, ref, c)
    hit = [n for n, v in (("y", vy), ("xn", vx)) if not v.ok]
    assert set(by) <= set(hit), f"{mutant} at {c.name}: rejected by {hit}, expected {by}: {vy.msg}"
    c.W = c.x = c.res = c.slots = c.num = None


def test_image_check_rejects_a_shifted_or_stray_row():
    B, N, ld = 3, 5, 9
    img = torch.full((B + 2, ld), float("nan"), dtype=F64)
    img[:B, :N] = 1.0
    assert R.check_image(img, B, N) == ""
    shifted = img.clone()                                   # row N - 1 written to row N
    shifted[:B, N], shifted[:B, N - 1] = 1.0, float("nan")
    assert "not written" in R.check_image(shifted, B, N)
    stray = img.clone()
    stray[:B, N] = 1.0                                      # the clamped duplicate of row N - 1 stored
    assert "outside" in R.check_image(stray, B, N)
    tok = img.clone()
    tok[B, :N] = 1.0                                        # the duplicated token of a column >= B stored
    assert "outside" in R.check_image(tok, B, N)
    nan = img.clone()
    nan[1, 2] = float("nan")
    assert "NaN" in R.check_image(nan, B, N)
