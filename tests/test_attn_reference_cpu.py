"""Self-test of the float64 attention reference and its checker (tests/_attn_ref.py), CPU only.

The reference must agree with a naive scalar emulation (python math, bit-level bf16 rounding) at tiny cases; a plain float32 model of
the same operation must stay inside the checker's bound at every case the GPU module launches (the bound is not tighter than fp32
arithmetic allows); the generated inputs must be tie-free with a bounded number of redraws; and the checker must reject each deliberate
defect of a correct output at the case named for it."""
import math
import struct

import pytest
import torch

import _attn_ref as A
from _attn_ref import HD

F64 = torch.float64


# ---- an independent scalar emulation ---------------------------------------------------------------------------------------------
def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def bf16(x):
    u = struct.unpack("<I", struct.pack("<f", f32(x)))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


RND = {"bf16": bf16, "f32": f32}


def naive(c):
    rd = RND[c.dt]
    nq = c.n_kv * c.rep
    row = [float(v) for v in c.qkv]
    cos, sin = [float(v) for v in c.cos], [float(v) for v in c.sin]

    def norm_rope(x, w):
        ss = 0.0
        for v in x:
            ss += v * v
        rs = 1.0 / math.sqrt(ss / HD + c.eps)
        n = [rd(float(w[d]) * rd(x[d] * rs)) for d in range(HD)]
        out = [0.0] * HD
        for d in range(64):
            out[d] = rd(rd(n[d] * cos[d]) + rd(-n[d + 64] * sin[d]))
            out[d + 64] = rd(rd(n[d + 64] * cos[d]) + rd(n[d] * sin[d]))
        return out

    q = [norm_rope(row[h * HD:(h + 1) * HD], c.qw) for h in range(nq)]
    k_new = [norm_rope(row[(nq + g) * HD:(nq + g + 1) * HD], c.kw) for g in range(c.n_kv)]
    v_new = [row[(nq + c.n_kv + g) * HD:(nq + c.n_kv + g + 1) * HD] for g in range(c.n_kv)]
    outs = []
    for h in range(nq):
        g = h // c.rep
        keys = [([float(v) for v in c.Kb[g, j]], [float(v) for v in c.Vb[g, j]]) for j in range(c.n_pad, c.pos)]
        if c.pos >= c.n_pad:
            keys.append((k_new[g], v_new[g]))
        sc = []
        for kj, _ in keys:
            t = 0.0
            for d in range(HD):
                t += q[h][d] * kj[d]
            sc.append(c.scale * t)
        m = max(sc)
        p = [math.exp(s - m) for s in sc]
        l = sum(p)
        outs.append([sum(p[j] * keys[j][1][d] for j in range(len(keys))) / l for d in range(HD)])
    return outs, q, k_new, v_new


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("kind,n_kv,rep,pos,n_pad", [("random", 1, 1, 0, 0), ("random", 2, 2, 3, 0), ("which", 2, 1, 5, 2),
                                                     ("random", 1, 2, 4, 4), ("random", 1, 1, 16, 0)])
def test_reference_equals_naive_scalar_loop(dt, kind, n_kv, rep, pos, n_pad):
    c = A.make_case(dt, kind, n_kv, rep, pos, n_pad, 17, seed=3)
    r = A.reference(c)
    outs, q, k_new, v_new = naive(c)
    assert torch.equal(r.q, torch.tensor(q, dtype=F64)) and torch.equal(r.k_new, torch.tensor(k_new, dtype=F64))
    assert torch.equal(r.v_new, torch.tensor(v_new, dtype=F64))
    o = torch.tensor(outs, dtype=F64)
    assert float((r.out - o).abs().max()) <= 1e-13 * max(1.0, float(o.abs().max()))
    assert bool((r.A + 1e-15 >= r.out.abs()).all())


def test_reference_partials_merge_to_the_output():
    for S in (1, 3, 8):
        for pos, n_pad in ((0, 0), (64, 0), (65, 5), (200, 70), (639, 0)):
            c = A.make_case("f32", "random", 2, 2, pos, n_pad, 640)
            r = A.reference(c, S)
            mo, _ = A.merge(r.p_num, r.p_m, r.p_l, S)
            mA, _ = A.merge(r.p_A, r.p_m, r.p_l, S)
            assert float((mo.reshape(-1, HD) - r.out).abs().max()) <= 1e-13
            assert float((mA.reshape(-1, HD) - r.A).abs().max()) <= 1e-13
            own_worker = (pos // 64) % S
            assert bool((r.p_l[:, own_worker] > 0).all())                              # the own key's worker is never empty
            empty = [w for w in range(S) if all(((t % S) != w) for t in range(n_pad // 64, pos // 64 + 1))]
            for w in empty:
                assert bool((r.p_l[:, w] == 0).all()) and bool((r.p_m[:, w] == A.EMPTY_M).all())


# ---- tie-free inputs -------------------------------------------------------------------------------------------------------------
def test_generator_needs_a_bounded_number_of_redraws():
    gen = torch.Generator().manual_seed(11)
    counts = []
    for _ in range(300):
        x, n = A.draw_head(gen, "bf16", 1e-6)
        assert A.tie_margin(x, 1e-6) > A.TAU
        counts.append(n)
    assert max(counts) <= A.MAX_REDRAWS
    assert sum(counts) / len(counts) <= 4.0, "expected (1 - 2^-7)^-128 - 1 = 1.7 redraws per head"


def all_cases(dt, kind):
    return [A.make_case(d, k, A.N_KV, rep, pos, n_pad, ms, seed=sd) for d, k, rep, pos, n_pad, ms, sd in A.gpu_cases()
            if d == dt and k == kind]


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_float32_model_is_inside_the_bound_at_every_gpu_case(dt, kind):
    """... and every committed case is tie-free under the reference alone, with sum (|a| + |b|) |k| <= RHO sum |q k| (the constant
    C_S of the score bound assumes it)."""
    worst = 0.0
    for c in all_cases(dt, kind):
        what = f"{dt} {kind} rep {c.rep} pos {c.pos} n_pad {c.n_pad} max_seq {c.max_seq}"
        assert c.redraws <= A.MAX_REDRAWS
        if dt == "bf16":
            nh = c.n_kv * c.rep + c.n_kv
            assert all(A.tie_margin(c.qkv[h * HD:(h + 1) * HD], c.eps) > A.TAU for h in range(nh)), what
        r = A.reference(c)
        assert r.rho <= A.RHO, f"{what}: rho {r.rho}"
        if kind == "which" and r.n_keys > 1:      # all scores within one unit of each other
            assert float(A.delta_max(r).max()) < 1e-4
        out, k_new, v_new = A.float32_model(c)
        v = A.check_output(out, r, dt, what=what)
        assert v, v.msg
        vk = A.check_kv_row(k_new, v_new, r, dt, what=what)
        assert vk, vk.msg
        worst = max(worst, v.ratio if dt == "f32" else 0.0, vk.ratio)
    print(f"float32 model, {dt} {kind}: largest err / bound {worst:.3g}")


# ---- the checker rejects each mutant ---------------------------------------------------------------------------------------------
def stored(x, dt):
    return A.rnd(x, dt)


def rejects_output(c, dt, **mut):
    good, bad = A.reference(c), A.reference(c, **mut)
    v = A.check_output(stored(good.out, dt), good, dt)
    assert v, "the correct output must pass: " + v.msg
    return not A.check_output(stored(bad.out, dt), good, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_checker_rejects_wrong_key_sets(dt, kind):
    mk = lambda pos, n_pad: A.make_case(dt, kind, 2, 2, pos, n_pad, 640)
    assert rejects_output(mk(200, 0), dt, drop=(199,)), "the last live key dropped"
    assert rejects_output(mk(639, 0), dt, drop=(638,)), "the last live key dropped (longest context)"
    assert rejects_output(mk(200, 70), dt, drop=(70,)), "key n_pad dropped"
    assert rejects_output(mk(200, 70), dt, extra=(69,)), "key n_pad - 1 included"
    assert rejects_output(mk(64, 0), dt, mutant="no_own"), "the own key dropped"
    assert rejects_output(mk(639, 0), dt, mutant="no_own"), "the own key dropped (longest context)"
    assert rejects_output(mk(65, 0), dt, mutant="own_twice"), "the own key counted twice"
    assert rejects_output(mk(130, 0), dt, drop=(63,)), "key 63 dropped"
    assert rejects_output(mk(130, 0), dt, drop=(64,)), "key 64 dropped"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_checker_rejects_own_key_in_two_workers(dt):
    c = A.make_case(dt, "which", 2, 2, 65, 0, 640)
    good = A.reference(c, 3)
    part = to_slots(good)
    assert A.check_partials(part, good), "the correct slots must pass"
    bad = part.clone()                                # worker 2 (no tile of its own yet) takes the own key as well
    own_s = c.scale * (good.q.view(2, 2, HD) * good.k_new[:, None]).sum(-1)
    bad[:, 2, :, :HD] = good.v_new[:, None, :]
    bad[:, 2, :, HD], bad[:, 2, :, HD + 1] = own_s, 1.0
    assert not A.check_partials(bad, good)


def to_slots(r):
    part = torch.full((r.p_num.shape[0], A.MAX_WORKERS, r.p_num.shape[2], A.PART_STRIDE), float("nan"), dtype=F64)
    part[:, :r.S, :, :HD], part[:, :r.S, :, HD], part[:, :r.S, :, HD + 1] = r.p_num, r.p_m, r.p_l
    return part.to(torch.float32).to(F64)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_checker_rejects_rope_and_norm_defects(dt):
    c = A.make_case(dt, "random", 2, 2, 130, 0, 640)
    good = A.reference(c)
    assert A.check_kv_row(good.k_new, good.v_new, good, dt)
    bad = A.reference(c, mutant="rope_sign")
    assert not A.check_kv_row(bad.k_new, bad.v_new, good, dt), "rotate_half sign flipped (K row)"
    assert not A.check_output(stored(bad.out, dt), good, dt), "rotate_half sign flipped (output)"
    assert not A.check_kv_row(good.k_new, good.v_new + 2.0 ** -20, good, dt), "V row not a copy"
    if dt == "bf16":      # (fp32 has no first rounding: the defect does not exist there)
        bad = A.reference(c, mutant="gain_before_round")
        assert not A.check_kv_row(bad.k_new, bad.v_new, good, dt), "gain applied before the first rounding"


def test_checker_rejects_merge_defects():
    c = A.make_case("f32", "random", 2, 2, 200, 0, 640)
    good = A.reference(c, 3)
    part = to_slots(good)
    assert A.check_partials(part, good)
    mo, _ = A.merge(part[:, :, :, :HD], part[:, :, :, HD], part[:, :, :, HD + 1], 3, swap=(0, 1))
    assert not A.check_output(mo.reshape(-1, HD), good, "f32"), "partial-merge weights of two workers swapped"
    c = A.make_case("f32", "which", 2, 2, 65, 0, 640)
    good = A.reference(c, 8)
    part = to_slots(good)
    assert A.check_partials(part, good)
    bad = part.clone()
    bad[:, 5, :, HD] = 0.0
    assert not A.check_partials(bad, good), "an empty worker's slot given m = 0"
    # the merge alone: NaN slots >= n_part are ignored by the reference, a wrong n_part is not accepted
    num, m, l = part[:, :, :, :HD], part[:, :, :, HD], part[:, :, :, HD + 1]
    out, _ = A.merge(num, m, l, 8)
    assert A.check_merge(out.reshape(-1, HD), num, m, l, 8, "f32")
    out2, _ = A.merge(num, m, l, 1)
    assert not A.check_merge(out2.reshape(-1, HD), num, m, l, 8, "f32")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_token_without_a_valid_key_has_empty_slots_and_zero_output(dt):
    c = A.make_case(dt, "random", 2, 2, 64, 70, 640)             # pos < n_pad: no live key, the own key is not valid
    r = A.reference(c, 3)
    assert r.n_keys == 0 and bool((r.out == 0).all()) and bool((r.p_l == 0).all()) and bool((r.p_m == A.EMPTY_M).all())
    assert A.check_partials(to_slots(r), r)
    assert A.check_output(torch.zeros_like(r.out), r, dt)
    assert not A.check_output(torch.full_like(r.out, float("nan")), r, dt)
    assert not A.check_output(torch.full_like(r.out, 2.0 ** -100), r, dt)
    out, k_new, v_new = A.float32_model(c)
    assert A.check_output(out, r, dt) and A.check_kv_row(k_new, v_new, r, dt)


@pytest.mark.parametrize("kind", A.KINDS)
def test_checker_rejects_truncated_output(kind):
    c = A.make_case("bf16", kind, 2, 4, 200, 0, 640)
    good = A.reference(c)
    assert A.check_output(A.rnd(good.out, "bf16"), good, "bf16")
    v = A.check_output(A.rnd_trunc(good.out, "bf16"), good, "bf16")
    assert not v and v.exact < 0.9


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_checker_rejects_v_row_of_the_neighbouring_head(dt):
    c = A.make_case(dt, "random", 2, 2, 130, 0, 640)
    assert rejects_output(c, dt, mutant="v_other_head")
