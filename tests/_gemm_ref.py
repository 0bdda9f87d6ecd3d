"""Float64 reference of the implicit-GEMM contract (csrc/codec_kernels.cuh, csrc/skinny_gemm.cuh) and an element-wise checker.

Written from the documented contract, not from the kernels:

* ``GemmArgs`` field comments: the A row of (m, tap) is ``m + tap_off[tap]``; rows outside ``[0, a_rows)`` read as zero; only rows
  ``[m_lo, M)`` are computed (the reads below ``m_lo`` are real); segment g of a batched launch reads / writes its own rows only;
  ``bias[n % bias_mod]``; act 0 none, 1 exact GELU, 2 SwiGLU over 16-column [gate | up] groups, 3 SiLU, 4 ReLU, 5 ELU, 6 tanh(ReLU),
  7 sigmoid, 8 log(max(v, 1e-5)); ``scale`` after the activation; the residual; the second output Y2 = SnakeBeta (act2 0) or ELU
  (act2 1) of the stored value, channel ``n % bias_mod``.
* ``epilogue_elem``: one rounding to the storage type T per op: v = rnd(acc + b), v = rnd(act(v)), v = rnd(scale * v),
  y = rnd(v + res); SnakeBeta y2 = rnd(y + rnd(ib * rnd(s * s))), s = rnd(sin(rnd(y * a))); ELU y2 = rnd(elu(y)).
* SwiGLU (act 2 of the tiles, ``silu_mul_kernel``, SK_SWIGLU): y = rnd(rnd(silu(g)) * u) with g, u the T-rounded accumulators.
* The SK_* table of skinny_gemm.cuh: SK_STORE y = rnd(acc), SK_RESIDUAL y = rnd(rnd(acc) + res); NORM: x_n = rnd(rnd(x * rs) * gain),
  rs = 1 / sqrt(sum(ssq) / K + eps); ``ssq_out`` = per token and 16-column block the sum of squares of the stored values.
* ``DT<T>`` / ``f_to_bfs``: rounding to bf16 is round-to-nearest-even of the fp32 value; bf16 x 2 (``bfs_t``) keeps hi = bf16(v) and
  lo = bf16(v - hi) (16 significant bits); fp32 needs no rounding.  Every rounding point goes through fp32 first, as in the kernels.

Accumulators are float64 (bf16 / fp32 operand products are exact there).  ``S = sum_k |a_k w_k|`` rides along as the scale of
cancellation for the checker.

Checker, per element: ``|got - ref| <= k * ulp_T(|ref|) + c * S_eff`` (S_eff = S propagated through the epilogue's factors), and the
fraction of elements exactly equal to the emulated value must be at least f (catches truncation instead of round-to-nearest-even,
which a 1-ulp bound cannot).  Constants:

* bf16: an fp32 accumulator of K products carries ~sqrt(K) 2^-24 S of error; against a bf16 half-ulp (2^-9 relative) that flips the
  rounding of roughly one element in 10^3 at K = 10^4, and one element of a SwiGLU or SnakeBeta chain one ulp further.  k = 2 ulp,
  c = 2^-18 (a floor for rows whose exact sum nearly cancels), f = 0.99.
* bf16 x 2: 16 significant bits (ulp 2^-15 relative): the fp32 accumulation error is within an order of magnitude of it at long K, so
  k = 4, c = 2^-18, f = 0.9 - 0.004 sqrt(K) (at least 0.5).  Observed on the MI355X: exact fraction 0.937 at K = 128 (SnakeBeta Y2
  included), 0.773 at K = 7168.
* Every output also gets the flips of its EARLIER rounding points (a one-ulp flip of rnd(acc + b) moves rnd(v + res) by that ulp, however
  small the result) propagated through the epilogue as an extra absolute allowance.
* fp32: no rounding to compare with (the order of the fp32 sum is the kernel's own): bound only, k = 8 (the fp32 transcendentals of
  the epilogue), c = 8 sqrt(K) 2^-24, f = 0.
See tests/test_gpu_gemm_reference.py for the values observed on the MI355X.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

torch.set_num_threads(min(16, max(1, torch.get_num_threads())))

F64 = torch.float64

TOL = {
    "bf16": dict(k=2.0, c=2.0 ** -18, f=0.99),
    "bfs": dict(k=4.0, c=2.0 ** -18, f=None),     # f = 0.9 - 0.004 sqrt(K), at least 0.5
    "f32": dict(k=8.0, c=None, f=0.0),
}


# ---- rounding emulation --------------------------------------------------------------------------------------------------
def rnd(x: torch.Tensor, dt: str) -> torch.Tensor:
    """Round a float64 tensor to storage type dt through fp32 (the kernels' rounding points); returns float64."""
    x32 = x.to(torch.float32)
    if dt == "f32":
        return x32.to(F64)
    hi = x32.to(torch.bfloat16).to(torch.float32)
    if dt == "bf16":
        return hi.to(F64)
    lo = (x32 - hi).to(torch.bfloat16).to(torch.float32)        # x32 - hi is exact in fp32
    return (hi + lo).to(F64)


def rnd_trunc(x: torch.Tensor, dt: str) -> torch.Tensor:
    """Truncating (round-toward-zero) rounding to bf16, or to bf16 x 2 (both halves truncated): the defect the exact-fraction test
    exists for."""
    assert dt in ("bf16", "bfs")
    x32 = x.to(torch.float32)
    hi = (x32.view(torch.int32) & ~0xFFFF).view(torch.float32)
    if dt == "bf16":
        return hi.to(F64)
    lo = ((x32 - hi).view(torch.int32) & ~0xFFFF).view(torch.float32)
    return (hi + lo).to(F64)


def ulp(x: torch.Tensor, dt: str) -> torch.Tensor:
    """ulp of |x| in storage type dt (bf16: 8 significant bits, bf16 x 2: 16, fp32: 24)."""
    bits = {"bf16": 8, "bfs": 16, "f32": 24}[dt]
    ax = x.abs().clamp_min(2.0 ** -120)
    e = torch.floor(torch.log2(ax))
    return torch.pow(2.0, e - (bits - 1))


# ---- element-wise functions of the epilogue (float64) -----------------------------------------------------------------------
def silu(v):
    return v / (1.0 + torch.exp(-v))


def elu(v):
    return torch.where(v > 0, v, torch.expm1(v))


def act_fn(act: int, v: torch.Tensor) -> torch.Tensor:
    if act == 1:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == 3:
        return silu(v)
    if act == 4:
        return v.clamp_min(0.0)
    if act == 5:
        return elu(v)
    if act == 6:
        return torch.tanh(v.clamp_min(0.0))
    if act == 7:
        return 1.0 / (1.0 + torch.exp(-v))
    if act == 8:
        return torch.log(v.clamp_min(1e-5))
    raise ValueError(act)


def act_slope(act: int, v: torch.Tensor) -> torch.Tensor:
    """|d act / dv| bound near v (propagates the cancellation floor through the activation)."""
    if act in (1, 3):
        return torch.full_like(v, 1.2)
    if act in (4, 5, 6):
        return torch.ones_like(v)
    if act == 7:
        return torch.full_like(v, 0.25)
    if act == 8:
        return 1.0 / v.abs().clamp_min(1e-5)
    raise ValueError(act)


# ---- the GEMM description --------------------------------------------------------------------------------------------------
@dataclass
class Gemm:
    """One GEMM of the contract.  Tensors hold T-representable values as float64.

    A: [n_seg][rows][Cin] (rows >= a_rows: what lies beyond a_rows must not be read); W: [N][taps * Cin]."""
    A: torch.Tensor
    W: torch.Tensor
    M: int
    a_rows: int
    taps: list = field(default_factory=lambda: [0])
    m_lo: int = 0
    dt: str = "bf16"
    bias: Optional[torch.Tensor] = None
    bias_mod: int = 0                 # 0 = N
    scale: Optional[torch.Tensor] = None
    res: Optional[torch.Tensor] = None   # [n_seg][M][N]
    act: int = 0
    y: bool = True
    y2: bool = False
    act2: int = 0
    sn_a: Optional[torch.Tensor] = None
    sn_ib: Optional[torch.Tensor] = None
    # skinny NORM consumer: A is the raw residual stream, ssq [M][K / 16] fp32 partials, gain [K]
    ssq: Optional[torch.Tensor] = None
    gain: Optional[torch.Tensor] = None
    eps: float = 1e-6

    @property
    def n_seg(self):
        return self.A.shape[0]

    @property
    def N(self):
        return self.W.shape[0]

    @property
    def Cin(self):
        return self.A.shape[2]

    @property
    def bmod(self):
        return self.bias_mod or self.N


def gather(g: Gemm, seg: int, rows: torch.Tensor, a_rows: Optional[int] = None, prev_seg: bool = False) -> torch.Tensor:
    """X[r] = concat over taps of A[seg][rows[r] + off] (zero outside [0, a_rows)): [len(rows)][taps * Cin].
    prev_seg (a mutant): rows below 0 read the previous segment's rows instead of zeros."""
    a_rows = g.a_rows if a_rows is None else a_rows
    A = g.A[seg]
    if g.ssq is not None:
        A = norm_input(g, seg)
    parts = []
    for off in g.taps:
        src = rows + off
        ok = (src >= 0) & (src < a_rows)
        X = torch.zeros(len(rows), g.Cin, dtype=F64)
        X[ok] = A[src[ok]]
        if prev_seg and seg > 0:
            neg = src < 0
            back = g.A[seg - 1].shape[0] + src[neg]
            okb = back >= 0
            idx = torch.nonzero(neg).flatten()[okb]
            X[idx] = g.A[seg - 1][back[okb]]
        parts.append(X)
    return torch.cat(parts, dim=1)


def norm_input(g: Gemm, seg: int, gain_round: bool = True) -> torch.Tensor:
    """NORM: x_n = rnd(rnd(x * rs) * gain), rs = 1 / sqrt(sum(ssq) / K + eps) in fp32."""
    K = g.Cin
    s = g.ssq.to(F64).sum(dim=1)
    rs = (1.0 / torch.sqrt(s / K + g.eps)).to(torch.float32).to(F64)
    xs = rnd(g.A[seg][: len(rs)] * rs[:, None], "bf16")
    prod = xs * g.gain[None, :]
    out = torch.zeros_like(g.A[seg])
    out[: len(rs)] = rnd(prod, "bf16") if gain_round else prod
    return out


@dataclass
class Ref:
    y: Optional[torch.Tensor]      # [n_seg][len(rows)][N_out] emulated values
    y2: Optional[torch.Tensor]
    s_y: torch.Tensor              # cancellation scale per element of y (S propagated)
    s_y2: Optional[torch.Tensor]
    K: int
    pre_res: Optional[torch.Tensor] = None   # y before the residual (for the mutants)
    e_y: Optional[torch.Tensor] = None       # extra absolute allowance of y: flips of the earlier rounding points, propagated
    e_y2: Optional[torch.Tensor] = None      # extra absolute allowance of y2 (SnakeBeta: one ulp of the sine moves its term by ~2 ulp)


def accumulate(g: Gemm, rows: torch.Tensor, drop_kstep: int = -1, **kw):
    """float64 accumulators and S for rows (absolute row numbers) of every segment: [n_seg][len(rows)][N]."""
    accs, ss = [], []
    Wt = g.W.t()
    if drop_kstep >= 0:
        Wt = Wt.clone()
        Wt[32 * drop_kstep: 32 * drop_kstep + 32] = 0.0
    for seg in range(g.n_seg):
        X = gather(g, seg, rows, **kw)
        accs.append(X @ Wt)
        ss.append(X.abs() @ Wt.abs())
    return torch.stack(accs), torch.stack(ss)


def reference(g: Gemm, rows: Optional[torch.Tensor] = None, *, mutant: str = "") -> Ref:
    """Emulated outputs of rows (default: every row of [m_lo, M)).  mutant names a deliberate defect (the checker's self-test)."""
    if rows is None:
        rows = torch.arange(g.m_lo, g.M)
    dt = g.dt
    R = (lambda x: rnd_trunc(x, dt)) if mutant == "trunc" else (lambda x: rnd(x, dt))
    kw = {}
    if mutant == "prev_seg":
        kw["prev_seg"] = True
    if mutant == "ignore_a_rows":
        kw["a_rows"] = g.A.shape[1]
    acc, S = accumulate(g, rows, drop_kstep=(1 if mutant == "drop_kstep" else -1), **kw)
    K = g.W.shape[1]
    N = g.N
    if g.act == 2:
        # SwiGLU over 16-column [gate | up] groups: logical column j <- gate column 32 (j // 16) + j % 16, up + 16
        j = torch.arange(N // 2)
        gc = 32 * (j // 16) + j % 16
        uc = gc + 16
        if mutant == "swap_gate_up":
            gc, uc = uc, gc
        return swiglu_ref(acc[..., gc], acc[..., uc], S[..., gc], S[..., uc], dt, R, K)
    n = torch.arange(N)
    ch = n % g.bmod
    b = g.bias[ch] if g.bias is not None else torch.zeros(N, dtype=F64)
    if mutant == "bias_by_n":                 # bias[n]: past bias_mod it reads whatever follows the vector
        b = torch.cat([g.bias, -g.bias.flip(0).repeat(N // g.bmod + 1)])[:N]
    v = R(acc + b)
    s = S.clone()
    e = torch.zeros_like(v)       # what a one-ulp flip of an EARLIER rounding point (fp32 accumulation order) moves the value by
    if g.act:
        sl = act_slope(g.act, v)
        s, e = s * sl, ulp(v, dt) * sl
        v = R(act_fn(g.act, v))
    if g.scale is not None:
        e = (e + ulp(v, dt)) * g.scale.abs() if g.act else ulp(v, dt) * g.scale.abs()
        v = R(g.scale * v)
        s = s * g.scale.abs()
    pre = v
    if g.res is not None:
        e = e + ulp(v, dt)
        r = g.res[:, rows]
        if mutant == "res_after_round":
            v = R(v) + r
        elif mutant == "res_one_rounding":
            v = R(acc + b + r) if not g.act and g.scale is None else R(v + r)
        else:
            v = R(v + r)
    y2 = s2 = e2 = None
    if g.y2:
        if g.act2 == 1:
            y2 = R(elu(v))
            s2 = s
            e2 = e + ulp(v, dt)
        else:
            a, ib = g.sn_a[n % g.bmod], g.sn_ib[n % g.bmod]
            sn = R(torch.sin(R(v * a)))
            term = R(ib * R(sn * sn))
            y2 = R(v + term)
            s2 = s * (1.0 + (ib * a).abs())
            e2 = 2.0 * ulp(term, dt) + (1.0 + (ib * a).abs()) * (e + ulp(v, dt))
    return Ref(v if g.y else None, y2, s, s2, K, pre_res=pre, e_y=e, e_y2=e2)


def swiglu_ref(ga, ua, sg, su, dt, R=None, K=0, swap=False):
    """y = rnd(rnd(silu(rnd(g))) * rnd(u)) from the float64 gate / up accumulators."""
    R = R or (lambda x: rnd(x, dt))
    gq, uq = R(ga), R(ua)
    if swap:
        gq, uq = uq, gq
    sq = R(silu(gq))
    y = R(sq * uq)
    s = sg * 1.2 * uq.abs() + su * silu(gq).abs()
    e = (1.2 * ulp(gq, dt) + ulp(sq, dt)) * uq.abs() + ulp(uq, dt) * sq.abs()
    return Ref(y, None, s, None, K, e_y=e)


def swiglu_halves_ref(g: Gemm, rows=None, mutant: str = "") -> Ref:
    """gemm_swiglu_halves: W = [gate (I rows) | up (I rows)], y[m][j] = rnd(rnd(silu(g_j)) * u_j)."""
    rows = torch.arange(g.m_lo, g.M) if rows is None else rows
    acc, S = accumulate(g, rows)
    I = g.N // 2
    gi, ui = slice(0, I), slice(I, 2 * I)
    if mutant == "swap_gate_up":
        gi, ui = ui, gi
    R = (lambda x: rnd_trunc(x, g.dt)) if mutant == "trunc" else None
    return swiglu_ref(acc[..., gi], acc[..., ui], S[..., gi], S[..., ui], g.dt, R, g.W.shape[1])


def interleave16(W: torch.Tensor) -> torch.Tensor:
    """The row-major [gate | up] copy with the halves interleaved in 16-row blocks (fq3_api.hip, packed kind 2):
    out row 32 b + w = gate row 16 b + w (w < 16), up row I + 16 b + (w - 16) otherwise."""
    N = W.shape[0]
    I = N // 2
    o = torch.arange(N)
    blk, w = o // 32, o % 32
    src = torch.where(w < 16, blk * 16 + w, I + blk * 16 + (w - 16))
    return W[src]


# ---- checker -----------------------------------------------------------------------------------------------------------------
@dataclass
class Verdict:
    ok: bool
    max_ulp: float
    exact: float
    worst: tuple
    msg: str


def check(got: torch.Tensor, ref: torch.Tensor, S: torch.Tensor, dt: str, K: int, *, what: str = "",
          rows: Optional[torch.Tensor] = None, k=None, c=None, f=None, extra=None) -> Verdict:
    """got / ref / S: [n_seg][rows][N] float64.  Per element |got - ref| <= k ulp_T(ref) + c S, no NaN, exact fraction >= f."""
    t = TOL[dt]
    k = t["k"] if k is None else k
    f = t["f"] if f is None else f
    if f is None:
        f = max(0.5, 0.9 - 0.004 * math.sqrt(K))
    if c is None:
        c = t["c"] if t["c"] is not None else 8.0 * math.sqrt(max(K, 1)) * 2.0 ** -24
    u = ulp(ref, dt)
    err = (got - ref).abs()
    nan = torch.isnan(got)
    err = torch.where(nan, torch.full_like(err, float("inf")), err)
    bound = k * u + c * S + (extra if extra is not None else 0.0)
    bad = err > bound
    e_ulp = err / u
    max_ulp = float(e_ulp.max()) if e_ulp.numel() else 0.0
    exact = float((got == ref).double().mean()) if got.numel() else 1.0
    worst = ()
    if e_ulp.numel():
        idx = int(torch.argmax(torch.where(bad, e_ulp + 1e30, e_ulp)))
        seg, r, n = np.unravel_index(idx, tuple(got.shape))
        m = int(rows[r]) if rows is not None else int(r)
        worst = (int(seg), m, int(n), float(got.flatten()[idx]), float(ref.flatten()[idx]))
    ok = not bool(bad.any()) and exact >= f
    msg = (f"{what}: {int(bad.sum())} / {got.numel()} elements out of bound (k={k}, c={c:.3g}), max error {max_ulp:.3g} ulp, "
           f"exact fraction {exact:.5f} (need {f}), worst (segment, m, n, got, ref) = {worst}")
    return Verdict(ok, max_ulp, exact, worst, msg)


# ---- device storage <-> float64 ----------------------------------------------------------------------------------------------
SENTINEL = {"bf16": 0xFFC1, "f32": 0xFFC1FFC1, "bfs": 0xFFC1FFC1}   # a quiet-NaN bit pattern no kernel produces


def to_storage(x: torch.Tensor, dt: str) -> torch.Tensor:
    """float64 values (T-representable) -> the storage tensor (bf16 / fp32 / int32 words of bfs_t)."""
    if dt == "bf16":
        return x.to(torch.bfloat16)
    if dt == "f32":
        return x.to(torch.float32)
    x32 = x.to(torch.float32)
    hi = x32.to(torch.bfloat16)
    lo = (x32 - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.stack([hi, lo], dim=-1).view(torch.int32).squeeze(-1)


def from_storage(t: torch.Tensor, dt: str) -> torch.Tensor:
    if dt == "bf16":
        return t.to(F64)
    if dt == "f32":
        return t.to(F64)
    hl = t.unsqueeze(-1).view(torch.bfloat16).to(torch.float32)
    return (hl[..., 0] + hl[..., 1]).to(F64)


def raw_bits(t: torch.Tensor) -> torch.Tensor:
    """the raw bit pattern of a storage tensor as int64 (bf16 -> 16 bits, fp32 / bfs_t -> 32 bits)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).to(torch.int64) & 0xFFFF
    if t.dtype == torch.float32:
        return t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return t.to(torch.int64) & 0xFFFFFFFF
