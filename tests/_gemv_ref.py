"""Float64 reference of the decode GEMV contract (csrc/decode_kernels.cuh: gemv_kernel; csrc/batch_kernels.cuh: gemv_batch_kernel,
rmsnorm_batch_kernel, gemv_batch_mfma_norm_kernel, gemv_batch_mfma_plain_kernel), the cases the GPU suite runs, and the checker.

Written from the header comments and the ``DT<T>`` rounding rules, not from the kernel bodies:

* y[t][n] = epilogue(sum_k W[n][k] xn[t][k]); W is [N][K] row-major (SwiGLU: the "up" row of logical row n is row n + up_off).
* Prologue PLAIN: xn = x.  NORM: ``xn = rnd(rnd(x * rs) * gain)``, ``rs = 1 / sqrt(mean(x^2) + eps)`` over the TRUE K (fp32).
  COMBINE: xn = rnd(merge of the first n_part split-KV partial slots) -- the merge of tests/_attn_ref.py, reused.
* Accumulation in fp32 (float64 here, with S = sum_k |w_k xn_k| as the scale of cancellation).
* Epilogues, one rounding to T per op: STORE ``rnd(acc + bias)``; RESIDUAL ``rnd(rnd(acc + bias) + res)``; SWIGLU
  ``rnd(rnd(silu(rnd(g))) * rnd(u))``.  xn_out receives xn (an observable of its own).
* Tails: a row >= N, a chunk beyond K and a token column >= B are clamped duplicates that are never stored and never read beyond
  the described buffers; everything outside [0, B) x [0, N) of the output stays untouched.

Bounds (the constants of ``_gemm_ref.TOL``, calibrated for the same rnd(acc) contract): per element
``|got - ref| <= k ulp_T(ref) + c S_eff + e`` with bf16 k = 2, c = 2^-18; fp32 k = 8, c = 8 sqrt(K) 2^-24.  e is the allowance for
what EARLIER rounding points may move (as in _gemm_ref: one ulp of rnd(acc + bias) under the residual add, the SwiGLU factors), plus
the prologue's share E_x = sum_k |w_k| ex_k:

* NORM.  The kernels' fp32 rs differs from the float64 one by at most EPS_X(K) = (K / 128 + 8) 2^-24 relative, product included: the
  sum of squares is one fma chain of K / 64 terms per lane and a 6-level tree over positive terms ((K / 64 + 6) 2^-24), the division
  by K, the eps add, sqrtf and the reciprocal are correctly rounded (4 x 2^-24; the square root halves what precedes it:
  (K / 128 + 3 + 2) 2^-24), and x * rs rounds once more to fp32 before the rounding to T.  bf16: an element can only flip (by one ulp)
  where x * rs lies within that distance of a rounding tie; rnd(u * gain) is then exact (an 8 x 8 bit product).  So
  ex_k = flippable_k (ulp(u_k) |gain_k| + ulp(xn_k)): one-ulp flips of xn propagated through sum_k |w_k| ulp(xn_k), restricted to the
  elements that can flip.  The cases' inputs are TIE-FREE (no element within 4 EPS_X of a tie: an element that is gets nudged by one
  ulp of x until none is), so ex = 0, xn_out is compared bit for bit and the bf16 exact fraction is not diluted.  fp32:
  ex_k = |xn_k| (EPS_X + 2^-23).
* COMBINE.  The fp32 merge is within gamma(n_part) A_k of the float64 one (_attn_ref.gamma, the bound its suite holds
  combine_batch_kernel to).  bf16: tie-free inputs again (no merged value within gamma A of a tie; the slots of one element are of one
  sign, so A = |out|), ex = 0 and xn_out is compared bit for bit; fp32: ex_k = gamma A_k + ulp_fp32(xn_k).

bf16 exact fraction (share of stored elements equal to the reference): f = 0.99 (TOL), as for the GEMM families.  The operands are
wide-range and every eighth weight row nearly cancels (S ~ 2^8 |acc|): on those rows no fp32 sum can pin the rounding, so they are
held to the bound only and the fraction is scored over the OTHER rows (SwiGLU: the outputs whose gate and up rows both are).  A case
of MIN_SCORED = 512 scored elements or more must reach 0.99 by itself.  The N = 1, 3, 5 cases hold a handful of elements each, where
one flip is 20 %: their elements are pooled per test (ExactPool) and the pool of n elements must reach 0.99 less three standard
deviations of a count at that rate, 0.99 - 3 sqrt(0.99 x 0.01 / n).  test_gemv_reference_cpu.py requires the float32 models of the
kernels' summation orders to clear both at every case, and one-ulp defects (truncation, a rounding moved across the bias or the
residual add) to fail them for every epilogue.  No constant is tuned to what the kernels produce; tests/test_gpu_gemv_reference.py
records what the MI355X gave.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

import _attn_ref as A
import _gemm_ref as G
from _gemm_ref import F64, rnd, rnd_trunc, ulp, silu

PRO_PLAIN, PRO_NORM, PRO_COMBINE = 0, 1, 2
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU = 0, 1, 2
PAIRS = ((PRO_NORM, EPI_STORE), (PRO_NORM, EPI_SWIGLU), (PRO_PLAIN, EPI_STORE), (PRO_PLAIN, EPI_RESIDUAL), (PRO_COMBINE, EPI_RESIDUAL))
PAIR_NAME = {(1, 0): "NORM+STORE", (1, 2): "NORM+SWIGLU", (0, 0): "PLAIN+STORE", (0, 1): "PLAIN+RESIDUAL", (2, 1): "COMBINE+RESIDUAL"}
DTS = ("f32", "bf16")
EPS = 1e-6
HD, MAX_WORKERS, PART_STRIDE = A.HD, A.MAX_WORKERS, A.PART_STRIDE
TOK_TILE, MAX_LANES, COMBINE_MAX_K = 16, 128, 2048
U32 = 2.0 ** -24
MAX_NUDGES = 60
F_EXACT = G.TOL["bf16"]["f"]


def eps_x(K: int) -> float:
    """Relative error of the kernels' fp32 x * rs against float64 (module docstring)."""
    return (K / 128 + 8) * U32


def gemv_chunks(K: int, most: int) -> int:
    need = (K + 511) // 512
    for n in (1, 2, 4, 6, 12):
        if need <= n and n <= most:
            return n
    return 0


def most_nch(pro: int, m: int) -> int:
    return 4 if pro in (PRO_NORM, PRO_COMBINE) else (6 if m == 2 else 12)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    kind: str                 # "gemv" | "batch" | "norm" | "plain" | "rmsnorm"
    dt: str
    pro: int
    epi: int
    N: int
    K: int
    B: int
    bias: bool = False
    up_gap: int = 0           # SWIGLU: up_off = N + up_gap
    n_part: int = 0
    rep: int = 0
    cancel: bool = True
    x_scale: float = 1.0      # every token's x times this (a power of two)
    seed: int = 0
    group: int = 0            # batch: a forced group next to the launcher's choice (0: none)
    # operands (float64 holding T values), filled by build()
    W: Optional[torch.Tensor] = None        # [n_rows][K]; SWIGLU: rows [N, up_off) are never read (NaN)
    x: Optional[torch.Tensor] = None        # [B][K]
    gain: Optional[torch.Tensor] = None
    bias_v: Optional[torch.Tensor] = None
    res: Optional[torch.Tensor] = None      # [B][N]
    slots: Optional[torch.Tensor] = None    # COMBINE: [B][n_groups][8][rep][132] fp32 values, slots >= n_part NaN
    num: Optional[torch.Tensor] = None      # COMBINE, head-major: [B][H][n_part][1][128]
    m: Optional[torch.Tensor] = None        # [B][H][n_part][1]
    l: Optional[torch.Tensor] = None

    @property
    def up_off(self):
        return self.N + self.up_gap if self.epi == EPI_SWIGLU else 0

    @property
    def n_rows(self):
        return self.up_off + self.N if self.epi == EPI_SWIGLU else self.N

    @property
    def name(self):
        s = f"{self.kind} {self.dt} {PAIR_NAME.get((self.pro, self.epi), 'rmsnorm')} N={self.N} K={self.K} B={self.B}"
        if self.pro == PRO_COMBINE:
            s += f" n_part={self.n_part} rep={self.rep}"
        return s + (" bias" if self.bias else "") + (f" up_off=N+{self.up_gap}" if self.epi == EPI_SWIGLU else "")


def _tie_dist(y):
    """Relative distance of |y| (float64, > 0) to the nearest bf16 rounding tie."""
    y = y.abs().clamp_min(2.0 ** -120)
    u = torch.pow(2.0, torch.floor(torch.log2(y)) - 7)
    frac = torch.remainder(y / u, 1.0)
    return (frac - 0.5).abs() * u / y


def norm_flippable(x, K, eps, margin):
    rs = 1.0 / torch.sqrt((x * x).sum(dim=-1, keepdim=True) / K + eps)
    y = x * rs
    return (y != 0) & (_tie_dist(y) <= margin)


@functools.lru_cache(maxsize=64)
def _weights(dt, n_rows, K, seed, cancel):
    gen = torch.Generator().manual_seed(1000 + seed)
    W = torch.randn(n_rows, K, generator=gen, dtype=F64) / math.sqrt(K)
    W = rnd(W, dt)
    if cancel:
        # every eighth row nearly cancels: its second half of K is the negated first half times (1 + 2^-7), against x halves that repeat
        h = K // 2
        W[1::8, h:2 * h] = rnd(-W[1::8, :h] * (1 + 2.0 ** -7), dt)
    return W


def build(c: Case) -> Case:
    """Fill in the operands (seeded; wide-range x over 2^-8 .. 2^7 per channel; partly cancelling rows; tie-free prologue inputs)."""
    if c.W is not None or (c.kind == "rmsnorm" and c.x is not None):
        return c
    dt, K, B, N = c.dt, c.K, c.B, c.N
    gen = torch.Generator().manual_seed(77 + c.seed)
    h = K // 2
    if c.kind != "rmsnorm":
        c.W = _weights(dt, c.n_rows, K, c.seed % 7, c.cancel)
        if c.epi == EPI_SWIGLU and c.up_gap:
            c.W = c.W.clone()
            c.W[N:c.up_off] = float("nan")
    scale = torch.pow(2.0, torch.randint(-8, 8, (K,), generator=gen).to(F64))
    if c.pro == PRO_COMBINE:
        _build_combine(c, gen)
    else:
        x = rnd(torch.randn(B, K, generator=gen, dtype=F64) * scale, dt) * c.x_scale
        if c.pro == PRO_NORM or c.kind == "rmsnorm":
            x[1::4] *= 2.0 ** -17                 # tokens 1, 5, ..: mean(x^2) below eps, so that eps decides their rs
        if c.cancel:
            x[:, h:2 * h] = x[:, :h]
        if c.pro == PRO_NORM or c.kind == "rmsnorm":
            g = rnd(torch.rand(K, generator=gen, dtype=F64) + 0.5, dt)
            if c.cancel:
                g[h:2 * h] = g[:h]
            c.gain = g
            if dt == "bf16":
                for _ in range(MAX_NUDGES):
                    flag = norm_flippable(x, K, EPS, 4.0 * eps_x(K))
                    if not bool(flag.any()):
                        break
                    x = torch.where(flag, rnd(x + torch.sign(x) * ulp(x, "bf16"), "bf16"), x)
                else:
                    raise RuntimeError(f"{c.name}: no tie-free input within MAX_NUDGES")
        c.x = x
    if c.bias:
        c.bias_v = rnd(torch.randn(N, generator=gen, dtype=F64) * 0.3, dt)
    if c.epi == EPI_RESIDUAL:
        c.res = rnd(torch.randn(B, N, generator=gen, dtype=F64), dt)
    return c


def _merge_case(c, num, m, l):
    """float64 merge of head-major slots: returns (out [B][K], A [B][K])."""
    out, Aa = A.merge(num, m, l, c.n_part)
    return out.reshape(c.B, c.K), Aa.reshape(c.B, c.K)


def _build_combine(c: Case, gen):
    B, K, S, rep = c.B, c.K, c.n_part, c.rep
    H = K // HD
    h = K // 2
    sign = torch.where(torch.rand(B, 1, K, generator=gen) < 0.5, -1.0, 1.0).to(F64)

    def draw_num():
        return rnd(sign * (0.05 + torch.randn(B, S, K, generator=gen, dtype=F64).abs() * 3.0), "f32")
    numf = draw_num()                                                                     # [B][S][K], one sign per element
    m = rnd(torch.rand(B, S, H, generator=gen, dtype=F64) * 60.0 - 30.0, "f32")
    l = rnd(1.0 + 49.0 * torch.rand(B, S, H, generator=gen, dtype=F64), "f32")
    empty = torch.rand(B, S, H, generator=gen) < 0.3
    empty[:, c.seed % S] = False                                                          # at least one live slot per head
    m[empty], l[empty] = A.EMPTY_M, 0.0

    def finish(numf):
        numf = numf.clone()
        numf[empty.repeat_interleave(HD, dim=2)] = 0.0
        mm, ll = m.clone(), l.clone()
        if c.cancel:                                                                      # x halves repeat (K = 128: inside the one head)
            numf[..., h:] = numf[..., :h]
            if H >= 2:
                mm[..., H // 2:], ll[..., H // 2:] = mm[..., :H // 2], ll[..., :H // 2]
                numf[..., h:] = numf[..., :h]
        num = numf.view(B, S, H, 1, HD).permute(0, 2, 1, 3, 4)                            # [B][H][S][1][128]
        return numf, num, mm.permute(0, 2, 1)[..., None], ll.permute(0, 2, 1)[..., None]
    if c.cancel and H >= 2:
        empty[..., H // 2:] = empty[..., :H // 2]
    for _ in range(MAX_NUDGES):
        numf, num, mm, ll = finish(numf)
        out, Aa = _merge_case(c, num, mm, ll)
        if c.dt != "bf16":
            break
        u = ulp(out, "bf16")
        frac = torch.remainder(out.abs() / u, 1.0)
        flag = ((frac - 0.5).abs() * u <= A.gamma(S) * Aa) & (out != 0)
        if not bool(flag.any()):
            break
        numf = torch.where(flag[:, None, :], draw_num(), numf)
    else:
        raise RuntimeError(f"{c.name}: no tie-free merge input within MAX_NUDGES")
    c.num, c.m, c.l = num, mm, ll
    slots = torch.full((B, H // rep, MAX_WORKERS, rep, PART_STRIDE), float("nan"), dtype=F64)
    nh = num.view(B, H // rep, rep, S, HD).permute(0, 1, 3, 2, 4)                         # [B][g][S][hh][128]
    slots[:, :, :S, :, :HD] = nh
    slots[:, :, :S, :, HD] = mm.view(B, H // rep, rep, S).permute(0, 1, 3, 2)
    slots[:, :, :S, :, HD + 1] = ll.view(B, H // rep, rep, S).permute(0, 1, 3, 2)
    slots[:, :, :S, :, HD + 2:] = 0.0
    c.slots = slots


# ---- the reference -------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_last_chunk", "drop_wave_share", "norm_pad512", "gain_before_round", "no_eps", "trunc", "bias_after_round",
           "res_before_round", "up_off_by_one", "swap_gate_up", "token_shift", "tile_copy")
MIN_SCORED = 512            # scored elements from which a case answers for its exact fraction alone


@dataclass
class Ref:
    y: torch.Tensor            # [B][N]
    s: torch.Tensor            # S propagated through the epilogue
    e: torch.Tensor            # extra absolute allowance
    xn: torch.Tensor           # [B][K] prologue result
    ex: torch.Tensor           # [B][K] allowance of xn (0 where it is exact)
    scored: torch.Tensor       # [N] bool: rows whose elements count for the bf16 exact fraction (not nearly cancelling)
    K: int


def prologue(c: Case, mutant: str = ""):
    dt, K = c.dt, c.K
    R = (lambda v: rnd_trunc(v, dt)) if (mutant == "trunc" and dt == "bf16") else (lambda v: rnd(v, dt))
    if c.pro == PRO_COMBINE:
        out, Aa = _merge_case(c, c.num, c.m, c.l)
        xn = R(out)
        ex = torch.zeros_like(xn) if dt == "bf16" else A.gamma(c.n_part) * Aa + ulp(xn, "f32")
        return xn, ex
    if c.pro == PRO_PLAIN and c.kind != "rmsnorm":
        return c.x, torch.zeros_like(c.x)
    Kd = ((K + 511) // 512) * 512 if mutant == "norm_pad512" else K
    eps = 0.0 if mutant == "no_eps" else EPS
    rs = 1.0 / torch.sqrt((c.x * c.x).sum(dim=-1, keepdim=True) / Kd + eps)
    if mutant == "gain_before_round":
        xn = R(c.x * rs * c.gain)
    else:
        u = R(c.x * rs)
        xn = R(u * c.gain)
    if dt == "bf16":
        flag = norm_flippable(c.x, K, EPS, eps_x(K)).to(F64)
        ex = flag * (ulp(u if mutant != "gain_before_round" else xn, dt) * c.gain.abs() + ulp(xn, dt))
    else:
        ex = xn.abs() * (eps_x(K) + 2.0 * U32)
    return xn, ex


def scored_rows(c: Case) -> torch.Tensor:
    """Output rows none of whose weight rows was built nearly cancelling (build: rows 1, 9, 17, ..)."""
    n = torch.arange(c.N)
    ok = torch.ones(c.N, dtype=torch.bool) if not c.cancel else (n % 8 != 1)
    if c.cancel and c.epi == EPI_SWIGLU:
        ok &= (n + c.up_off) % 8 != 1
    return ok


def reference(c: Case, mutant: str = "") -> Ref:
    if mutant and mutant not in MUTANTS:
        raise ValueError(f"unknown mutant {mutant!r}")
    build(c)
    dt, K, N, B = c.dt, c.K, c.N, c.B
    R = (lambda v: rnd_trunc(v, dt)) if (mutant == "trunc" and dt == "bf16") else (lambda v: rnd(v, dt))
    xn, ex = prologue(c, mutant)
    if c.kind == "rmsnorm":
        return Ref(xn, xn.abs(), ex, xn, ex, torch.ones(K, dtype=torch.bool), K)
    xa = xn
    if mutant == "token_shift" and B > 1:
        xa = torch.roll(xn, -1, dims=0)
    if mutant == "tile_copy" and B > TOK_TILE:
        xa = xn.clone()
        xa[TOK_TILE:2 * TOK_TILE] = xn[:TOK_TILE][: xa[TOK_TILE:2 * TOK_TILE].shape[0]]
    W = torch.nan_to_num(c.W, nan=0.0)
    if mutant == "drop_last_chunk":
        W = W.clone()
        W[:, 512 * ((K + 511) // 512 - 1):] = 0.0
    if mutant == "drop_wave_share":
        W = W.clone()
        W[:, K // 4: K // 2] = 0.0
    acc = xa @ W.t()
    S = xa.abs() @ W.abs().t()
    E = ex @ W.abs().t()
    if c.epi == EPI_SWIGLU:
        n = torch.arange(N)
        uo = c.up_off + (1 if mutant == "up_off_by_one" else 0)
        gi, ui = n, torch.clamp(n + uo, max=c.n_rows - 1)
        if mutant == "swap_gate_up":
            gi, ui = ui, gi
        r = G.swiglu_ref(acc[:, gi], acc[:, ui], S[:, gi], S[:, ui], dt, R, K)
        gq, uq = R(acc[:, gi]), R(acc[:, ui])
        sq = R(silu(gq))
        e = r.e_y + 1.2 * E[:, gi] * uq.abs() + E[:, ui] * sq.abs()
        return Ref(r.y, r.s_y, e, xn, ex, scored_rows(c), K)
    acc, S, E = acc[:, :N], S[:, :N], E[:, :N]
    b = c.bias_v if c.bias_v is not None else torch.zeros(N, dtype=F64)
    if mutant == "bias_after_round":
        v = R(R(acc) + b)
    elif mutant == "res_before_round" and c.res is not None:
        v = acc + b + c.res
    else:
        v = R(acc + b)
    e = E.clone()
    if c.epi == EPI_RESIDUAL:
        e = e + ulp(v, dt)
        v = R(v) if mutant == "res_before_round" else R(v + c.res)
    return Ref(v, S, e, xn, ex, scored_rows(c), K)


# ---- checker ---------------------------------------------------------------------------------------------------------------------
def check_y(got: torch.Tensor, ref: Ref, c: Case, what: str = "", rows=None) -> G.Verdict:
    """got [B][N] float64 as stored in T (rows: the tokens of ref that got holds).  The bound everywhere; bf16: the exact fraction over
    the scored rows (v.n_exact of v.n_scored, v.exact), which a case of MIN_SCORED scored elements must hold at F_EXACT by itself --
    smaller cases go to an ExactPool."""
    y, s, e = (ref.y, ref.s, ref.e) if rows is None else (ref.y[rows], ref.s[rows], ref.e[rows])
    v = G.check(got[None], y[None], s[None], c.dt, c.K, what=what or c.name, extra=e[None], f=0.0)
    t = G.TOL[c.dt]
    bound = t["k"] * ulp(y, c.dt) + (t["c"] if t["c"] is not None else 8.0 * math.sqrt(c.K) * U32) * s + e
    err = torch.nan_to_num((got - y).abs(), nan=float("inf"))
    v.ratio = float((err / bound).max()) if got.numel() else 0.0           # largest err / bound (a record: check() has judged)
    v.n_scored = v.n_exact = 0
    if c.dt == "bf16":
        eq = (got == y)[:, ref.scored]
        v.n_scored, v.n_exact = eq.numel(), int(eq.sum())
        v.exact = v.n_exact / max(1, v.n_scored)
        if v.n_scored >= MIN_SCORED and v.exact < F_EXACT:
            v.ok = False
            v.msg += f"; exact fraction over the scored rows {v.exact:.5f} ({v.n_exact} of {v.n_scored}) below {F_EXACT}"
    return v


class ExactPool:
    """The scored elements of the cases too small to answer for their exact fraction alone (module docstring)."""

    def __init__(self):
        self.n = self.k = 0

    def add(self, v):
        if v.n_scored < MIN_SCORED:
            self.n, self.k = self.n + v.n_scored, self.k + v.n_exact

    @property
    def exact(self):
        return self.k / self.n if self.n else 1.0

    @property
    def floor(self):
        return F_EXACT - 3.0 * math.sqrt(F_EXACT * (1.0 - F_EXACT) / self.n) if self.n else 0.0

    def check(self, what=""):
        assert self.exact >= self.floor, f"{what}: pooled bf16 exact fraction {self.exact:.5f} ({self.k} of {self.n}) below {self.floor:.5f}"


def check_xn(got: torch.Tensor, ref: Ref, c: Case, what: str = "", rows=None) -> G.Verdict:
    """The prologue result got [B][K]: bf16 with ex = 0 bit-exact; otherwise |got - xn| <= ex (+ one rounding)."""
    xn, ex = (ref.xn, ref.ex) if rows is None else (ref.xn[rows], ref.ex[rows])
    bound = ex + (0.0 if c.dt == "bf16" else 0.5 * ulp(xn, "f32"))
    err = (got - xn).abs()
    err = torch.where(torch.isnan(got), torch.full_like(err, float("inf")), err)
    bad = err > bound
    exact = float((got == xn).double().mean())
    ratio = float((err / bound.clamp_min(2.0 ** -140)).max()) if bool((bound > 0).any()) else (0.0 if not bool(bad.any()) else float("inf"))
    msg = f"{what or c.name} xn: {int(bad.sum())} / {got.numel()} elements out of bound, exact fraction {exact:.5f}"
    if bool(bad.any()):
        i = torch.nonzero(bad)[0]
        msg += f", first at {tuple(int(v) for v in i)}: got {float(got[tuple(i)])!r}, ref {float(xn[tuple(i)])!r}"
    v = G.Verdict(not bool(bad.any()), float((err / ulp(xn, c.dt)).max()) if got.numel() else 0.0, exact, (), msg)
    v.ratio = ratio
    return v


def check_image(img: torch.Tensor, B: int, N: int, what: str = "") -> str:
    """img [rows][ld] float64 with NaN standing for an untouched sentinel: NaN-free inside [0, B) x [0, N), all NaN outside."""
    inside = img[:B, :N]
    if bool(torch.isnan(inside).any()):
        i = torch.nonzero(torch.isnan(inside))[0]
        return f"{what}: element (token {int(i[0])}, row {int(i[1])}) was not written or is NaN"
    mask = torch.ones_like(img, dtype=torch.bool)
    mask[:B, :N] = False
    touched = mask & ~torch.isnan(img)
    if bool(touched.any()):
        i = torch.nonzero(touched)[0]
        return f"{what}: written outside [0, B) x [0, N) at (token {int(i[0])}, row {int(i[1])})"
    return ""


# ---- float32 models of the kernels' summation orders (the bounds must admit them) ----------------------------------------------
def _epilogue32(c: Case, acc: torch.Tensor) -> torch.Tensor:
    """acc [B][n_rows] float32 accumulators -> stored values (float64), every op in fp32 then rounded to T."""
    f32, dt, N = torch.float32, c.dt, c.N
    R = lambda v: rnd(v.to(F64), dt).to(f32)
    if c.epi == EPI_SWIGLU:
        g, u = R(acc[:, :N]), R(acc[:, c.up_off:c.up_off + N])
        sg = R(g / (1.0 + torch.exp(-g)))
        return R(sg * u).to(F64)
    b = c.bias_v.to(f32) if c.bias_v is not None else torch.zeros(N, dtype=f32)
    v = R(acc[:, :N] + b)
    if c.epi == EPI_RESIDUAL:
        v = R(v + c.res.to(f32))
    return v.to(F64)


def prologue32(c: Case) -> torch.Tensor:
    """The prologue with an fp32 rs (sum of squares as a float32 sum)."""
    if c.pro != PRO_NORM and c.kind != "rmsnorm":
        return prologue(c)[0]
    f32 = torch.float32
    x = c.x.to(f32)
    ss = (x * x).sum(dim=-1, keepdim=True, dtype=f32)
    rs = 1.0 / torch.sqrt(ss / float(c.K) + f32_scalar(EPS))
    u = rnd((x * rs).to(F64), c.dt).to(f32)
    return rnd((u * c.gain.to(f32)).to(F64), c.dt)


def f32_scalar(v):
    return torch.tensor(v, dtype=torch.float32)


def model_valu(c: Case) -> torch.Tensor:
    """gemv_kernel / gemv_batch_kernel: lane l owns elements 512 j + 8 l + i, one fma chain over (j, i), then the wave tree."""
    build(c)
    f32, K = torch.float32, c.K
    xn = prologue32(c)
    nch = (K + 511) // 512
    W = torch.zeros(c.n_rows, nch * 512, dtype=F64)
    W[:, :K] = torch.nan_to_num(c.W, nan=0.0)
    X = torch.zeros(c.B, nch * 512, dtype=F64)
    X[:, :K] = xn
    Wl, Xl = W.view(c.n_rows, nch, 64, 8), X.view(c.B, nch, 64, 8)
    acc = torch.zeros(c.B, c.n_rows, 64, dtype=f32)
    for j in range(nch):
        for i in range(8):
            acc = (acc.to(F64) + Xl[:, None, j, :, i] * Wl[None, :, j, :, i]).to(f32)          # fma: one rounding
    lane = torch.arange(64)
    for sh in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[..., lane ^ sh]
    return _epilogue32(c, acc[..., 0])


def model_mfma(c: Case, NW: Optional[int] = None) -> torch.Tensor:
    """The matrix-core kernels: NW waves split K, each adds its 16x16x32 blocks in order (one fp32 rounding per block here), the NW
    shares are added in fixed order by wave 0."""
    build(c)
    f32, K = torch.float32, c.K
    NW = NW or (4 if (c.pro == PRO_NORM or K <= 1024) else 8)
    ks = K // (32 * NW)
    xn = prologue32(c)
    W = torch.nan_to_num(c.W, nan=0.0)
    blocks = torch.einsum("bwsk,nwsk->bnws", xn.view(c.B, NW, ks, 32), W.view(c.n_rows, NW, ks, 32))
    part = torch.zeros(c.B, c.n_rows, NW, dtype=f32)
    for s in range(ks):
        part = (part.to(F64) + blocks[..., s]).to(f32)
    tot = part[..., 0]
    for w in range(1, NW):
        tot = tot + part[..., w]
    return _epilogue32(c, tot)


# ---- the cases of the GPU suite ----------------------------------------------------------------------------------------------------
GEMV_K = (8, 264, 512, 520, 1024, 1032, 2048, 2056, 3072, 3080, 6144)
GEMV_K_BIG_N = (8, 520, 1032, 2056, 3080)          # one K per chunk count (1, 2, 4, 6, 12), each with a short last chunk
GEMV_N_SMALL, GEMV_N_BIG = (1, 3, 5), (1024, 1029, 2052)
COMBINE_K, COMBINE_PARTS, COMBINE_REPS = (128, 1024, 2048), (1, 3, 8), (1, 2, 4)
BATCH_B = (1, 3, 4, 5, 8, 9, 16, 17)
BATCH_GROUPS = (1, 3, 4, 8)
BATCH_SHAPES = ((5, 520), (1, 8), (3, 1032), (6, 2056), (5, 3080), (5, 6144), (1029, 264))
MFMA_B = (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80, 128)
NORM_KSTEPS, NORM_N = (2, 4, 8, 16), (16, 24, 48)
PLAIN_K, PLAIN_N = (256, 512, 768, 1024, 2048, 3072, 4096, 6144), (16, 24)
RMSNORM_SHAPES = ((8, 1), (520, 5), (1024, 17), (1032, 3), (2048, 6))


def gemv_cases(dt, pro, epi):
    out, i = [], 0
    if pro == PRO_COMBINE:
        for K in COMBINE_K:
            for n_part in COMBINE_PARTS:
                for rep in COMBINE_REPS:
                    if (K // HD) % rep:
                        continue
                    for N in (5, 1029):
                        i += 1
                        out.append(Case("gemv", dt, pro, epi, N, K, 2, bias=bool(i % 2), n_part=n_part, rep=rep, seed=i))
        return out
    kmax = 2048 if pro == PRO_NORM else 6144
    for K in GEMV_K:
        if K > kmax:
            continue
        for N in GEMV_N_SMALL + (GEMV_N_BIG if K in GEMV_K_BIG_N else ()):
            i += 1
            out.append(Case("gemv", dt, pro, epi, N, K, 2, bias=bool(i % 2), up_gap=(0 if i % 3 else 3), seed=i))
    return out


def batch_group_max(dt, K):
    return 4 if (dt == "f32" and (K + 511) // 512 > 6) else 8


def batch_cases(dt, pro, epi):
    out, esz = [], 2 if dt == "bf16" else 4
    for i, B in enumerate(BATCH_B):
        for j, (N, K) in enumerate(BATCH_SHAPES):
            if (i + j) % 2 or (pro == PRO_NORM and K > 2048):
                continue
            g = BATCH_GROUPS[(i + j // 2) % 4]
            ok = g <= min(B, batch_group_max(dt, K)) and g * K * esz <= 150 * 1024
            out.append(Case("batch", dt, pro, epi, N, K, B, bias=bool((i + j) % 4 == 0), up_gap=(0 if j % 2 else 5), seed=10 * i + j,
                            group=g if ok else 0))
    return out


def norm_cases(ks, epi):
    return [Case("norm", "bf16", PRO_NORM, epi, NORM_N[(i + ks) % 3], 128 * ks, B, bias=bool(i % 2 and epi == EPI_STORE),
                 up_gap=(0 if i % 2 else 16), seed=100 + i) for i, B in enumerate(MFMA_B)]


def plain_cases(K, epi):
    return [Case("plain", "bf16", PRO_PLAIN, epi, PLAIN_N[(i + K // 256) % 2], K, B, bias=bool(i % 2), seed=200 + i)
            for i, B in enumerate(MFMA_B)]


def rmsnorm_cases():
    return [Case("rmsnorm", "bf16", PRO_NORM, EPI_STORE, 1, K, B, seed=300 + K) for K, B in RMSNORM_SHAPES]


def all_cases():
    out = []
    for dt in DTS:
        for pro, epi in PAIRS:
            out += gemv_cases(dt, pro, epi)
            if pro != PRO_COMBINE:
                out += batch_cases(dt, pro, epi)
    for ks in NORM_KSTEPS:
        for epi in (EPI_STORE, EPI_SWIGLU):
            out += norm_cases(ks, epi)
    for K in PLAIN_K:
        for epi in (EPI_STORE, EPI_RESIDUAL):
            out += plain_cases(K, epi)
    return out + rmsnorm_cases()
