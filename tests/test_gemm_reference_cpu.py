"""Self-test of the float64 GEMM reference and its checker (tests/_gemm_ref.py), CPU only.

The reference must agree with a naive scalar triple loop on tiny shapes for every epilogue (bf16, bf16 x 2, fp32), and the checker must
reject each deliberate defect of an output while it accepts correctly rounded values with a few 1-ulp flips."""
import math
import struct

import pytest
import torch

import _gemm_ref as R

F64 = torch.float64


# ---- an independent scalar emulation (bit operations on fp32, math module functions) -----------------------------------------
def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def bf16(x):
    u = struct.unpack("<I", struct.pack("<f", f32(x)))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


def bfs(x):
    v = f32(x)
    hi = bf16(v)
    lo = bf16(f32(v - hi))
    return f32(hi + lo)


RND = {"bf16": bf16, "bfs": bfs, "f32": f32}


def act_scalar(act, v):
    if act == 1:
        return 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))
    if act == 3:
        return v / (1.0 + math.exp(-v))
    if act == 4:
        return max(v, 0.0)
    if act == 5:
        return v if v > 0 else math.expm1(v)
    if act == 6:
        return math.tanh(max(v, 0.0))
    if act == 7:
        return 1.0 / (1.0 + math.exp(-v))
    return math.log(max(v, 1e-5))


def naive(g: R.Gemm):
    rd = RND[g.dt]
    nseg, N, C = g.n_seg, g.N, g.Cin
    Y = [[[None] * (N // 2 if g.act == 2 else N) for _ in range(g.M)] for _ in range(nseg)]
    Y2 = [[[None] * N for _ in range(g.M)] for _ in range(nseg)]
    for s in range(nseg):
        for m in range(g.m_lo, g.M):
            acc = [0.0] * N
            for n in range(N):
                t = 0.0
                for ti, off in enumerate(g.taps):
                    r = m + off
                    if r < 0 or r >= g.a_rows:
                        continue
                    for c in range(C):
                        t += float(g.A[s, r, c]) * float(g.W[n, ti * C + c])
                acc[n] = t
            if g.act == 2:
                for j in range(N // 2):
                    gc = 32 * (j // 16) + j % 16
                    gq, uq = rd(acc[gc]), rd(acc[gc + 16])
                    Y[s][m][j] = rd(rd(gq / (1.0 + math.exp(-gq))) * uq)
                continue
            for n in range(N):
                ch = n % g.bmod
                v = rd(acc[n] + (float(g.bias[ch]) if g.bias is not None else 0.0))
                if g.act:
                    v = rd(act_scalar(g.act, v))
                if g.scale is not None:
                    v = rd(float(g.scale[n]) * v)
                if g.res is not None:
                    v = rd(v + float(g.res[s, m, n]))
                Y[s][m][n] = v
                if g.y2:
                    if g.act2:
                        Y2[s][m][n] = rd(v if v > 0 else math.expm1(v))
                    else:
                        a, ib = float(g.sn_a[ch]), float(g.sn_ib[ch])
                        sn = rd(math.sin(rd(v * a)))
                        Y2[s][m][n] = rd(v + rd(ib * rd(sn * sn)))
    return Y, Y2


def make(dt="bf16", *, M=9, N=64, Cin=32, taps=(0,), nseg=1, a_rows=None, m_lo=0, act=0, bias=True, bias_mod=0, scale=False,
         res=False, y2=False, act2=0, seed=0, rows=None):
    gen = torch.Generator().manual_seed(seed)
    rows = rows or M + 4
    A = R.rnd(torch.randn(nseg, rows, Cin, generator=gen, dtype=F64), dt)
    W = R.rnd(torch.randn(N, len(taps) * Cin, generator=gen, dtype=F64) / math.sqrt(len(taps) * Cin), "bf16")
    bmod = bias_mod or N
    g = R.Gemm(A=A, W=W, M=M, a_rows=M if a_rows is None else a_rows, taps=list(taps), m_lo=m_lo, dt=dt, act=act, bias_mod=bias_mod,
               y2=y2, act2=act2)
    if bias:
        g.bias = R.rnd(torch.randn(bmod, generator=gen, dtype=F64) * 0.5, dt)
    if scale:
        g.scale = R.rnd(torch.rand(N, generator=gen, dtype=F64) + 0.5, dt)
    if res:
        g.res = R.rnd(torch.randn(nseg, M, N, generator=gen, dtype=F64), dt)
    if y2 and act2 == 0:
        g.sn_a = R.rnd(torch.rand(bmod, generator=gen, dtype=F64) + 0.5, dt)
        g.sn_ib = R.rnd(torch.rand(bmod, generator=gen, dtype=F64) + 0.5, dt)
    if act == 8:
        g.A = g.A.abs()
        g.W = g.W.abs()
    return g


EPILOGUES = [dict(), dict(act=1), dict(act=3, scale=True), dict(act=4, res=True), dict(act=5), dict(act=6), dict(act=7), dict(act=8),
             dict(res=True, y2=True), dict(y2=True, act2=1, bias_mod=24), dict(act=2, bias=False), dict(scale=True, res=True, y2=True),
             dict(taps=(-4, -2, 0), a_rows=7, m_lo=2, res=True), dict(taps=(-3, 0), nseg=2, bias_mod=16)]


@pytest.mark.parametrize("dt", ["bf16", "bfs", "f32"])
@pytest.mark.parametrize("ep", range(len(EPILOGUES)))
def test_reference_matches_naive_triple_loop(dt, ep):
    kw = dict(EPILOGUES[ep])
    if kw.get("act") == 2 and dt != "bf16":
        pytest.skip("SwiGLU in the tiles is a bf16 epilogue")
    g = make(dt, **kw)
    ref = R.reference(g)
    Y, Y2 = naive(g)
    for s in range(g.n_seg):
        for i, m in enumerate(range(g.m_lo, g.M)):
            got = torch.tensor(Y[s][m], dtype=F64)
            assert torch.equal(ref.y[s, i], got), (dt, kw, s, m)
            if g.y2:
                assert torch.equal(ref.y2[s, i], torch.tensor(Y2[s][m], dtype=F64)), (dt, kw, s, m)


def test_bfs_rounding_keeps_16_bits():
    x = torch.randn(1000, dtype=F64)
    r = R.rnd(x, "bfs")
    assert torch.equal(r, torch.tensor([bfs(float(v)) for v in x], dtype=F64))
    assert float(((r - x) / x).abs().max()) < 2.0 ** -15
    assert torch.equal(R.from_storage(R.to_storage(r, "bfs"), "bfs"), r)


def test_interleave16_layout():
    W = torch.arange(64, dtype=F64)[:, None].repeat(1, 2)          # row r holds r
    Wi = R.interleave16(W)[:, 0].long().tolist()
    assert Wi[:32] == list(range(16)) + list(range(32, 48))
    assert Wi[32:] == list(range(16, 32)) + list(range(48, 64))


# ---- the checker rejects each defect -----------------------------------------------------------------------------------------
def _check(g, got, ref):
    return R.check(got, ref.y, ref.s_y, g.dt, ref.K, what="self-test", extra=ref.e_y)


def big(dt="bf16", **kw):
    kw.setdefault("M", 40)
    kw.setdefault("N", 64)
    kw.setdefault("Cin", 256)
    return make(dt, **kw)


MUTANTS = {
    "drop_kstep": dict(),
    "trunc": dict(),
    "bias_by_n": dict(bias_mod=48, N=96),
    "prev_seg": dict(taps=(-3, 0), nseg=2),
    "ignore_a_rows": dict(a_rows=30, taps=(-2, 0, 2)),
    "res_after_round": dict(res=True, act=1),
    "res_one_rounding": dict(res=True),
    "swap_gate_up": dict(act=2, bias=False),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_checker_rejects_mutant(mutant):
    g = big(**MUTANTS[mutant])
    ref = R.reference(g)
    assert _check(g, ref.y, ref).ok
    bad = R.reference(g, mutant=mutant)
    v = _check(g, bad.y, ref)
    assert not v.ok, f"{mutant} passed: {v.msg}"


def test_checker_rejects_sentinel_left_in_ragged_row():
    g = big(M=37)
    ref = R.reference(g)
    got = ref.y.clone()
    got[0, 36, :] = float("nan")
    assert not _check(g, got, ref).ok


def test_checker_rejects_norm_without_gain_rounding():
    g = big(M=24, N=64, Cin=1024, bias=False)
    gen = torch.Generator().manual_seed(3)
    g.A = R.rnd(torch.randn(1, 28, 1024, generator=gen, dtype=F64) * 3.0, "bf16")
    g.gain = R.rnd(torch.rand(1024, generator=gen, dtype=F64) + 0.5, "bf16")
    g.ssq = (g.A[0, :24] ** 2).reshape(24, 64, 16).sum(-1).to(torch.float32)
    ref = R.reference(g)
    acc, _ = R.accumulate(g, torch.arange(24))
    assert torch.equal(R.rnd(acc, "bf16"), ref.y)
    Xn = R.norm_input(g, 0, gain_round=False)[:24]
    bad = R.rnd((Xn @ g.W.t())[None], "bf16")
    assert not _check(g, bad, ref).ok


def test_checker_accepts_rare_one_ulp_flips():
    g = big(M=200, N=128, Cin=512)
    ref = R.reference(g)
    got = ref.y.clone()
    gen = torch.Generator().manual_seed(7)
    flip = torch.rand(got.shape, generator=gen) < 0.003
    sign = torch.where(torch.rand(got.shape, generator=gen) < 0.5, -1.0, 1.0).to(F64)
    got = torch.where(flip, got + sign * R.ulp(got, "bf16"), got)
    assert int(flip.sum()) > 0
    v = _check(g, got, ref)
    assert v.ok, v.msg
    assert v.max_ulp <= 1.0


def test_checker_rejects_truncation_in_bfs():
    # bf16 x 2 with both halves truncated instead of rounded to nearest even: within the bound, caught by the exact fraction
    g = big("bfs", res=True, y2=True)
    ref = R.reference(g)
    assert _check(g, ref.y, ref).ok
    bad = R.reference(g, mutant="trunc")
    v = _check(g, bad.y, ref)
    assert not v.ok and v.exact < 0.8, v.msg


def test_checker_reports_the_worst_element():
    g = big("bfs")
    ref = R.reference(g)
    got = ref.y.clone()
    got[0, 5, 7] += 100 * float(R.ulp(got[0, 5, 7], "bfs"))
    v = _check(g, got, ref)
    assert not v.ok and v.worst[:3] == (0, 5, 7), v.msg
