"""Self-test of the float64 prefill / windowed attention reference and its checkers (tests/_prefill_attn_ref.py), CPU only.

The reference must agree with a naive scalar emulation (python math, bit-level bf16 rounding) at tiny cases; a plain float32 model of
each operation must stay inside the checker's bound at every case the GPU module launches (the bound is not tighter than fp32
arithmetic allows); the generated inputs must be tie-free with a bounded number of redraws; and the checker must reject each named
defect of a correct output at the case chosen for it."""
import math

import pytest
import torch

import _attn_ref as A
import _prefill_attn_ref as P
from _prefill_attn_ref import HD, KS, N_KV
from test_attn_reference_cpu import RND

F64 = torch.float64
DTS = ("f32", "bf16")


# ---- an independent scalar emulation ---------------------------------------------------------------------------------------------
def naive_attention(q, K, V, keys_of, scale):
    """q [rows][NH][hd], K / V [n_kv][rows][hd] as nested lists; keys_of(t) the key range of row t."""
    rows, NH, n_kv = len(q), len(q[0]), len(K)
    rep = NH // n_kv
    out = []
    for t in range(rows):
        row = []
        for h in range(NH):
            g = h // rep
            ks = list(keys_of(t))
            if not ks:
                row.append([0.0] * len(q[t][h]))
                continue
            sc = []
            for j in ks:
                acc = 0.0
                for d in range(len(q[t][h])):
                    acc += q[t][h][d] * K[g][j][d]
                sc.append(scale * acc)
            m = max(sc)
            p = [math.exp(s - m) for s in sc]
            l = sum(p)
            row.append([sum(p[i] * V[g][j][d] for i, j in enumerate(ks)) / l for d in range(len(q[t][h]))])
        out.append(row)
    return out


@pytest.mark.parametrize("kind,rep,L,n_pad", [("random", 1, 1, 0), ("random", 2, 5, 0), ("which", 2, 6, 2), ("random", 4, 4, 3)])
def test_causal_reference_equals_naive_scalar_loop(kind, rep, L, n_pad):
    s = P.Seq("bf16", kind, N_KV, rep, L, n_pad, 3)
    K, V = s.KV
    r = P.attn_reference(s.q, K, V, n_pad)
    o = torch.tensor(naive_attention(s.q.tolist(), K.tolist(), V.tolist(), lambda t: range(n_pad, t + 1) if t >= n_pad else (), P.SCALE), dtype=F64)
    assert float((r.out - o).abs().max()) <= 1e-13 * max(1.0, float(o.abs().max()))
    assert bool((r.A + 1e-15 >= r.out.abs()).all()) and bool((r.out[:n_pad] == 0).all())
    assert r.n_keys.tolist() == [max(0, t - n_pad + 1) for t in range(L)]


@pytest.mark.parametrize("hd,Tn,window,nb", [(32, 5, 2, 1), (32, 6, 3, 2), (64, 4, 8, 1), (32, 3, 1, 1)])
def test_windowed_reference_equals_naive_scalar_loop(hd, Tn, window, nb):
    x = P.win_input("f32", "random", hd, nb, Tn, seed=2)
    scale = 1.0 / math.sqrt(hd)
    r = P.win_reference(x, window, scale)
    for b in range(nb):
        q = x[b, :, 0].tolist()
        K, V = x[b, :, 1].transpose(0, 1).tolist(), x[b, :, 2].transpose(0, 1).tolist()          # one kv head per q head
        o = torch.tensor(naive_attention(q, K, V, lambda t: range(max(0, t - window + 1), t + 1), scale), dtype=F64)
        assert float((r.out[b] - o).abs().max()) <= 1e-13 * max(1.0, float(o.abs().max()))
    assert r.nk.tolist() == [min(t + 1, window) for t in range(Tn)]


@pytest.mark.parametrize("dt", DTS)
def test_norm_reference_equals_naive_scalar_loop(dt):
    rd = RND[dt]
    L, n_pad, delta, rope_len, rep = 4, 1, -2, 3, 2
    x = P.norm_input(dt, rep, L)
    qw, kw = A.base_gains(dt, "random")
    r = P.norm_reference(x, qw, kw, N_KV, n_pad, delta, dt, rope_len=rope_len)
    NH = N_KV * rep
    for t in range(n_pad, L):
        rp = min(max(t + delta, 0), rope_len - 1)
        cos, sin = [[float(v) for v in row] for row in P.rope_row(rp)]
        for h in range(NH + N_KV):
            xv = [float(v) for v in x[t, h]]
            w = [float(v) for v in (qw if h < NH else kw)]
            rs = 1.0 / math.sqrt(sum(v * v for v in xv) / HD + P.EPS)
            n = [rd(w[d] * rd(xv[d] * rs)) for d in range(HD)]
            want = [0.0] * HD
            for d in range(64):
                want[d] = rd(rd(n[d] * cos[d]) + rd(-n[d + 64] * sin[d]))
                want[d + 64] = rd(rd(n[d + 64] * cos[d]) + rd(n[d] * sin[d]))
            got = r.q[t, h] if h < NH else r.k[h - NH, t]
            assert torch.equal(got, torch.tensor(want, dtype=F64)), (t, h)
    assert bool(torch.isnan(r.q[:n_pad]).all()) and bool(torch.isnan(r.k[:, :n_pad]).all()) and bool(torch.isnan(r.v[:, :n_pad]).all())
    assert torch.equal(r.v[:, n_pad:], x[n_pad:, NH + N_KV:].transpose(0, 1))


@pytest.mark.parametrize("dt", DTS)
def test_rope_rows_reference_equals_naive_scalar_loop(dt):
    rd = RND[dt]
    hd, Tn, nb = 32, 3, 2
    x = P.win_input(dt, "random", hd, nb, Tn)
    cos, sin = P.win_rope_table(Tn, hd)
    out, ab = P.rope_rows_reference(x, cos, sin, dt)
    for b in range(nb):
        for t in range(Tn):
            for part in range(2):
                for h in range(P.W_NH):
                    v = [float(e) for e in x[b, t, part, h]]
                    for j in range(hd // 2):
                        cs, sn = float(cos[t, j]), float(sin[t, j])
                        assert float(out[b, t, part, h, j]) == rd(rd(v[j] * cs) + rd(-v[j + hd // 2] * sn))
                        assert float(out[b, t, part, h, j + hd // 2]) == rd(rd(v[j + hd // 2] * cs) + rd(v[j] * sn))
    assert bool((ab + 1e-300 >= out.abs() * (1 - 2.0 ** -7)).all())


def test_pool_round_trip_through_a_shuffled_table():
    s = P.Seq("bf16", "random", N_KV, 2, 200, 70)
    K, _ = s.dead_rows(finite=True)
    table = P.shuffled_table(4, 7, 1)
    pool = P.to_pool(K, table, 7)
    assert torch.equal(P.from_pool(pool, table, 256), K)
    assert table != sorted(table) and bool(torch.isnan(pool[[b for b in range(7) if b not in table]]).all())
    assert bool(torch.isfinite(K).all()) and float(K[:, :70].abs().max()) == A.BIG and float(K[:, 200:].abs().max()) == A.BIG
    Kn, Vn = s.dead_rows(finite=False)
    assert bool(torch.isnan(Kn[:, :70]).all()) and bool(torch.isnan(Vn[:, 200:]).all()) and torch.equal(Kn[:, 70:200], s.KV[0][:, 70:])


# ---- tie-free inputs -------------------------------------------------------------------------------------------------------------
def test_generator_stays_within_max_redraws_and_rows_are_tie_free():
    x, worst = P.norm_rows("bf16", P.N_NORM_ROWS)
    assert worst <= P.MAX_REDRAWS
    for t in (0, 1, 63, 64, 200, 320, P.N_NORM_ROWS - 1):
        for h in range(P.NH_MAX + N_KV):
            assert A.tie_margin(x[t, h], P.EPS) > A.TAU


# ---- the float32 model stays inside every bound the GPU module applies ----------------------------------------------------------------
def attention_cases():
    """(L, n_pad, seed) of every sequence the GPU module launches (sequence q of a pack draws from seed q % 4)."""
    seen = set()
    packed = [(L, p, q % 4) for pk in P.PACKS.values() for q, (L, p, _) in enumerate(pk)]
    for c in [(L, p, 0) for L, p in P.WAVE_CASES + P.PAIRED4_CASES + P.PAIRED8_CASES] + packed:
        if c not in seen:
            seen.add(c)
            yield c


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_float32_model_of_causal_attention_is_inside_both_bounds(dt, kind):
    worst = {"wave": 0.0, "flash": 0.0}
    floors = []
    for rep in P.REPS:
        for L, n_pad, seed in attention_cases():
            s = P.Seq(dt, kind, N_KV, rep, L, n_pad, seed)
            r = P.seq_reference(s)
            got = P.attn_float32_model(s.q, *s.KV, n_pad, dt)
            for kernel in ("wave",) + (("flash",) if dt == "bf16" else ()):
                v = P.check_attn(got, r, dt, kernel, what=f"{dt} {kind} rep {rep} L {L} n_pad {n_pad} {kernel}")
                assert v, v.msg
                worst[kernel] = max(worst[kernel], v.ratio)
            if dt == "bf16":
                floors.append(P.flash_floor(r))
            if kind == "which" and L > 1:
                assert float(r.Bmax.max()) * P.C_SP * P.U32 < 1e-4          # all scores within a unit of each other
    print(f"float32 model, {dt} {kind}: largest err / bound {worst}; flash exact-fraction floors {min(floors or [1]):.3f} .. {max(floors or [1]):.3f}")


@pytest.mark.parametrize("dt", DTS)
def test_float32_model_of_the_norm_is_inside_the_bound(dt):
    qw, kw = A.base_gains(dt, "random")
    worst = 0.0
    for rep in P.REPS:
        for i, (L, n_pad) in enumerate(P.WAVE_CASES):
            delta = P.ROPE_DELTAS[i % 3]
            x = P.norm_input(dt, rep, L)
            r = P.norm_reference(x, qw, kw, N_KV, n_pad, delta, dt)
            v = P.check_norm(*P.norm_float32_model(x, qw, kw, N_KV, n_pad, delta, dt), r, dt, what=f"{dt} rep {rep} L {L} n_pad {n_pad}")
            assert v, v.msg
            worst = max(worst, v.ratio)
        for pack in P.PACKS.values():                       # the packed sequences: their own rows of the pool, n_pad and rope_delta
            start = 0
            for L, n_pad, delta in pack:
                x = P.norm_input(dt, rep, L, start=start)
                start += L
                r = P.norm_reference(x, qw, kw, N_KV, n_pad, delta, dt)
                v = P.check_norm(*P.norm_float32_model(x, qw, kw, N_KV, n_pad, delta, dt), r, dt, what=f"{dt} rep {rep} pack L {L} n_pad {n_pad}")
                assert v, v.msg
                worst = max(worst, v.ratio)
    print(f"float32 model of norm + RoPE, {dt}: largest err / bound {worst:.3g}")


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_float32_model_of_windowed_attention_is_inside_the_bound(dt, kind):
    worst = 0.0
    for hd in (32, 64, 128):
        scale = 1.0 / math.sqrt(hd)
        for Tn in P.SWA_TN:
            for nb in (1, 3):
                x = P.win_input(dt, kind, hd, nb, Tn)
                for w in P.SWA_WINDOWS:
                    v = P.check_win(P.win_float32_model(x, w, scale, dt), P.win_reference(x, w, scale), dt, 0, P.EXP_REL,
                                    what=f"swa {dt} {kind} hd {hd} Tn {Tn} window {w}")
                    assert v, v.msg
                    worst = max(worst, v.ratio)
        if dt == "f32":
            for Tn, w in sorted({c for np_ in (1, 2, 3, 4) for c in P.win_cases(np_)}):
                x = P.win_input(dt, kind, hd, 1, Tn)
                v = P.check_win(P.win_float32_model(x, w, scale, dt), P.win_reference(x, w, scale), dt, 0, P.EXPF_REL,
                                what=f"win {kind} hd {hd} Tn {Tn} window {w}")
                assert v, v.msg
                worst = max(worst, v.ratio)
    print(f"float32 model of windowed attention, {dt} {kind}: largest err / bound {worst:.3g}")


@pytest.mark.parametrize("dt", DTS)
def test_float32_model_of_rope_rows_is_inside_the_bound(dt):
    for hd in (32, 64, 128):
        x = P.win_input(dt, "random", hd, 3, 65)
        cos, sin = P.win_rope_table(65, hd)
        want, ab = P.rope_rows_reference(x, cos, sin, dt)
        v = P.check_rope_rows(P.rope_rows_float32_model(x, cos, sin, dt), want, ab, dt, 0)
        assert v, v.msg
        # fp32: a product fused into the sum (one rounding fewer) is inside the bound as well
        if dt == "f32":
            half = hd // 2
            qk = x[:, :, :2]
            cs, sn = cos[None, :, None, None, :], sin[None, :, None, None, :]
            fused = torch.cat([P.rnd(qk[..., :half] * cs + P.rnd(-qk[..., half:] * sn, dt), dt),
                               P.rnd(P.rnd(qk[..., half:] * cs, dt) + qk[..., :half] * sn, dt)], dim=-1)
            assert P.check_rope_rows(fused, want, ab, dt, 0)


# ---- the checker rejects each named mutant at the case chosen for it -------------------------------------------------------------------
def stored(x, dt):
    return P.rnd(x, dt)


def rejects(seq, kernel, *, mutant="", K=None, V=None):
    good = P.seq_reference(seq)
    v = P.check_attn(stored(good.out, seq.dt), good, seq.dt, kernel)
    assert v, "the correct output must pass: " + v.msg
    Kl, Vl = seq.KV
    bad = P.attn_reference(seq.q, Kl if K is None else K, Vl if V is None else V, seq.n_pad, mutant=mutant)
    return not P.check_attn(stored(bad.out, seq.dt), good, seq.dt, kernel)


def kernels(dt):
    return ("wave", "flash") if dt == "bf16" else ("wave",)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_key_off_by_one_at_the_causal_edge(dt, kind):
    for kernel in kernels(dt):
        for L in (65, 321):          # at a tile border; the longest row (one key of 321 moves a probability by 0.3 %)
            assert rejects(P.Seq(dt, kind, N_KV, 2, L, 0), kernel, mutant="causal_minus"), (kernel, L)
        # key t + 1 taken: the last row has no such key, so every row but the last one is wrong
        assert rejects(P.Seq(dt, kind, N_KV, 2, 321, 0), kernel, mutant="causal_plus"), kernel


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_pad_mask_gt_instead_of_ge(dt, kind):
    for kernel in kernels(dt):
        for L, n_pad in ((200, 64), (321, 65), (65, 64)):
            assert rejects(P.Seq(dt, kind, N_KV, 2, L, n_pad), kernel, mutant="pad_gt"), (kernel, L, n_pad)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_wrong_kv_head_under_gqa(dt, kind):
    for kernel in kernels(dt):
        for rep in (2, 4):
            if kind == "which":      # both kv heads hold the same V there: the K rows differ, the probabilities move only a little
                continue
            assert rejects(P.Seq(dt, kind, N_KV, rep, 129, 0), kernel, mutant="kv_head"), (kernel, rep)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_identity_block_table(dt, kind):
    """The cache is read through the identity table instead of the shuffled one: rows of other tiles, or the NaN of an unowned block."""
    for kernel in kernels(dt):
        s = P.Seq(dt, kind, N_KV, 2, 200, 0)
        table = [2, 0, 3, 1]
        Kp, Vp = (P.to_pool(X, table, 6) for X in s.dead_rows(finite=True))
        ident = list(range(4))
        assert rejects(s, kernel, K=P.from_pool(Kp, ident, 200), V=P.from_pool(Vp, ident, 200)), kernel
        assert not rejects(s, kernel, K=P.from_pool(Kp, table, 200), V=P.from_pool(Vp, table, 200)), kernel


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_second_sequence_reading_the_first_ones_table(dt, kind):
    for kernel in kernels(dt):
        s0, s1 = (P.Seq(dt, kind, N_KV, 2, L, p, seed) for seed, (L, p, _) in enumerate(P.PACK3[:2]))
        t0, t1 = [5, 1, 3, 0], [4, 2]
        pools = []
        for X0, X1 in zip(s0.dead_rows(finite=True), s1.dead_rows(finite=True)):
            pool = P.to_pool(X0, t0, 8)
            own = P.to_pool(X1, t1, 8)
            pool[t1] = own[t1]
            pools.append(pool)
        assert rejects(s1, kernel, K=P.from_pool(pools[0], t0, s1.L), V=P.from_pool(pools[1], t0, s1.L)), kernel
        assert not rejects(s1, kernel, K=P.from_pool(pools[0], t1, s1.L), V=P.from_pool(pools[1], t1, s1.L)), kernel


@pytest.mark.parametrize("kind", P.KINDS)
def test_checker_rejects_swapped_keys_of_the_transposed_v_word(kind):
    for L in (64, 200):
        assert rejects(P.Seq("bf16", kind, N_KV, 2, L, 0), "flash", mutant="v_pair_swap"), L


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_window_off_by_one(dt, kind):
    for hd, Tn, w, exp_rel in ((64, 130, 72, P.EXP_REL), (32, 130, 128, P.EXP_REL), (128, 65, 64, P.EXP_REL), (64, 300, 250, P.EXPF_REL)):
        if exp_rel == P.EXPF_REL and dt != "f32":
            continue
        x = P.win_input(dt, kind, hd, 1, Tn)
        scale = 1.0 / math.sqrt(hd)
        good = P.win_reference(x, w, scale)
        assert P.check_win(stored(good.out, dt), good, dt, 0, exp_rel)
        for mutant in ("window_plus", "window_minus"):
            bad = P.win_reference(x, w, scale, mutant=mutant)
            assert not P.check_win(stored(bad.out, dt), good, dt, 0, exp_rel), (hd, Tn, w, mutant)


@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_unclamped_rope_position(dt):
    qw, kw = A.base_gains(dt, "random")
    for L, delta in ((17, -7), (321, 40)):             # t + delta below 0; beyond rope_len - 1
        x = P.norm_input(dt, 2, L)
        good = P.norm_reference(x, qw, kw, N_KV, 0, delta, dt)
        assert P.check_norm(good.q, good.k, good.v, good, dt)
        bad = P.norm_reference(x, qw, kw, N_KV, 0, delta, dt, mutant="rope_unclamped")
        assert not P.check_norm(bad.q, good.k, good.v, good, dt), "q"
        assert not P.check_norm(good.q, bad.k, good.v, good, dt), "K rows"
        assert not P.check_norm(good.q, good.k, good.v + 2.0 ** -20, good, dt), "V rows not a copy"


@pytest.mark.parametrize("dt", DTS)
def test_checker_rejects_interleaved_rope_rows(dt):
    x = P.win_input(dt, "random", 64, 1, 5)
    cos, sin = P.win_rope_table(5, 64)
    want, ab = P.rope_rows_reference(x, cos, sin, dt)
    assert P.check_rope_rows(want, want, ab, dt, 0)
    bad, _ = P.rope_rows_reference(x, cos, sin, dt, mutant="interleaved")
    assert not P.check_rope_rows(bad, want, ab, dt, 0)


@pytest.mark.parametrize("kind", P.KINDS)
def test_checker_rejects_truncated_output(kind):
    s = P.Seq("bf16", kind, N_KV, 4, 200, 0)
    good = P.seq_reference(s)
    for kernel in ("wave", "flash"):
        v = P.check_attn(A.rnd_trunc(good.out, "bf16"), good, "bf16", kernel)
        assert not v and v.exact < 0.9, kernel


def test_pad_rows_must_be_exact_zeros():
    s = P.Seq("bf16", "random", N_KV, 2, 200, 130)
    good = P.seq_reference(s)
    out = stored(good.out, "bf16")
    assert P.check_attn(out, good, "bf16", "flash")
    bad = out.clone()
    bad[5, 1, 7] = 2.0 ** -100
    assert not P.check_attn(bad, good, "bf16", "flash")
    bad = out.clone()
    bad[150, 0, 0] = float("nan")
    assert not P.check_attn(bad, good, "bf16", "wave")
