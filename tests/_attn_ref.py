"""Float64 reference of the decode-time attention contract (csrc/decode_kernels.cuh, csrc/batch_kernels.cuh) and an element-wise checker.

Written from the documented contract (the comments above ``AttnArgs``, ``attn_decode_body``, ``attn_pred_body``,
``attn_decode_batch_kernel`` and ``attn_decode_lane_kernel``), not from the kernel bodies:

* one token's row is ``[q (n_kv * rep heads) | k (n_kv heads) | v (n_kv heads)]``, head dim 128; q heads ``g * rep .. g * rep + rep - 1``
  attend to kv head g.
* per head RMSNorm then rotate_half RoPE of every q head and of the new k, one rounding to the storage type T per op (fp32 first, then
  T, as every rounding point of the kernels): ``n = rnd(w * rnd(x * rs))``, ``rs = 1 / sqrt(mean(x^2) + eps)``; dims d < 64:
  ``rnd(rnd(n_d * cos_d) + rnd(-n_{d+64} * sin_d))``, dims d >= 64: ``rnd(rnd(n_d * cos_{d-64}) + rnd(n_{d-64} * sin_{d-64}))``.
  v is copied unchanged.  The new k / v row is appended at cache row ``pos`` of its kv head (paged: slot ``pos % 64`` of block
  ``table[pos / 64]``) -- unless the loop is done (``done_ptr`` / ``DecodeState::done`` nonzero), which writes nothing at all.
* softmax in fp32 over the live keys ``n_pad <= j < pos`` plus the token's own key (valid when ``pos >= n_pad``), scores
  ``scale * q . k_j``; dead slots may hold NaN bit patterns and rows below n_pad anything.
* split-KV: worker s of S walks the 64-key tiles s, s + S, ...; the worker of tile ``pos / 64`` also takes the own key; every worker
  writes its slot ``{num[128], m, l}`` (empty: ``{0, m = -1e30, l = 0}``); the merge is ``sum_s e^(m_s - M) num_s / sum_s e^(m_s - M) l_s``
  rounded once to T and ignores slots >= n_part.  A done lane of the batch form leaves ``{0, m = 0, l = 1}`` (merged: zeros), a done
  lane of the lane kernel writes zeros.  A token without any valid key (pos < n_pad: no live key, and the own key is not valid) has
  empty slots only and the output zero.

Everything is float64 here (products of bf16 / fp32 operands are exact there).  Alongside the output ride the scales of the bound:
``A_d = sum_j p_j |v_jd|`` (the output's cancellation scale) and ``B_j = scale * sum_d |q_d k_jd|`` (the score's).

Tie-free inputs.  The only rounding point whose pre-rounding value the kernel does not know exactly is ``rnd(x * rs)``: w * (.) is a
product of two bf16 values (exact in fp32), n * cos is one correctly rounded fp32 product, the RoPE sum one correctly rounded fp32 sum.
The kernel's fp32 rs differs from the exact one: the sum of 128 squares is at most 12 roundings deep in the arrangements a wave
uses (an 8-term fma chain per lane + a 4-level tree, or 2 per lane + a 6-level tree; u = 2^-24 each, all terms positive: 12 u),
``/ 128`` is exact, ``+ eps`` 1 u  => 13 u on the radicand, 6.5 u after the square root, + 1 u each for the (correctly rounded) sqrt and
division  => 8.5 u, + 1 u for the product x * rs and 1 u slack for a 1-ulp (not 0.5-ulp) sqrt / division  => about 10.5 u = 2^-20.6,
i.e. of the order of 2^-20.  TAU = 16 * 2^-20 = 2^-16: the generator redraws, per head, any vector whose float64
x * rs has an element within the RELATIVE margin TAU of a bf16 rounding tie, so the kernel's value rounds to the same bf16 as the
reference's and bf16 q, k_new and v_new are determined exactly.  A tie lies every 2^-7 .. 2^-8 (relative), so an element is rejected
with probability about 2 TAU / 2^-8 = 2^-7 and a 128-vector accepted with probability (1 - 2^-7)^128 = 0.37: 1.7 redraws per head
on average, and more than MAX_REDRAWS = 40 with probability 0.63^40 = 1e-8.

Checker.
* appended K / V row, bf16: bit-exact.  fp32: ``|got - ref| <= C_K * 2^-24 * (|a| + |b|)``, a, b the two RoPE products: kernel 10.5 u on
  x * rs (above), + 1 u gain product, + 1 u RoPE product, + 1 u RoPE sum = 13.5 u; the reference rounds each of its four stages to
  fp32 (4 u): 17.5 u, C_K = 20.  v: bit-exact in both types.
* outputs and partial numerators: ``|got - ref| <= E * A_d`` (+ half a T-ulp of ref where the kernel stores T), ``E = 2 max_j(delta_j) +
  gamma``.
  - ``delta_j = C_S * 2^-24 * B_j``: gamma_128 of a 128-term fp32 dot product however it is ordered (128 u) + 1 u for ``* scale`` = 129 u,
    + the input error of q: 16 u of |a| + |b| per element (the K-row bound less the reference's share), and sum_d (|a_d| + |b_d|) |k_d| <=
    RHO * sum_d |q_d k_d| with RHO = 2 (asserted for every case by the CPU self-test: tests/test_attn_reference_cpu.py) = 32 u, + the
    same for the own key's k = 32 u: 193 u, C_S = 200.  The factor 2: out = sum_j w_j v_j, w_j = p_j / sum p; a common error of the
    running maximum cancels between numerator and denominator, the rest moves the numerator by delta A and the denominator by delta.
  - ``gamma = 2 * (ceil(n / 16) + 16) * (EXP_REL + 2 * 2^-24)`` for n keys: the documented layout walks the keys in 16 lane groups (4 rows
    x 4 waves; fewer keys per group with more workers), so a term passes at most ceil(n / 16) online-softmax steps -- each one __expf
    (rescale or probability) and two roundings (fma + product) -- plus at most 4 + 8 + 1 <= 16 for the merges across rows, waves,
    worker slots and the normalisation; times 2 for numerator and denominator.
  - EXP_REL = 2 * the measured maximum relative error of ``__expf`` against float64 exp on a grid of 2^16 + 1 arguments in [-90, 0]
    (attn_probe_expf; results below 2^-126 are flushed and excluded: such a weight is below 1e-38 of the largest).  Measured on the
    MI355X: 3.835e-6 (at x = -87.3331: the error is the rounding of x * log2(e), it grows with |x|), so EXP_REL = 7.7e-6; below
    2^-126 the largest absolute error was 1.17e-38.
    tests/test_gpu_attn_reference.py::test_expf_grid asserts measured <= EXP_REL / 2.
  - bf16: the fraction of stored elements exactly equal to rnd(ref) must be at least F_EXACT = 0.99, as in _gemm_ref.check (an fp32
    error of ~1e-6 against the 2^-9 half-ulp flips about one element in 10^3; truncation instead of round-to-nearest-even halves it).
* partial slots: the kernel's running maximum may differ from the reference's by delta, so a slot is compared after rescaling by
  ``e^(m_got - m_ref)`` in float64: ``|m_got - m_ref| <= max delta``, numerators within ``E * sum_j p_j |v_jd|``, l within ``E * l``; an empty
  slot must be exactly ``{0, -1e30, 0}``; and the float64 merge of the kernel's slots must meet the output bound.
See tests/test_gpu_attn_reference.py for the values observed on the MI355X.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from _gemm_ref import F64, rnd, rnd_trunc, ulp

HD, KS, MAX_WORKERS, PART_STRIDE = 128, 64, 8, 132
U32 = 2.0 ** -24
C_K = 20.0
C_S = 200.0
RHO = 2.0
EXP_REL = 7.7e-6
TAU = 2.0 ** -16
MAX_REDRAWS = 40
F_EXACT = 0.99
EMPTY_M = float(torch.tensor(-1e30, dtype=torch.float32))
BIG = 2.0 ** 60


# ---- head RMSNorm + RoPE ------------------------------------------------------------------------------------------------------
def head_norm_rope(x, w, cos, sin, eps, dt, *, mutant=""):
    """x [..., 128], w [128], cos / sin [64] (float64 holding T / fp32 values).  Returns (rotated [..., 128], |a| + |b| [..., 128])."""
    R = lambda v: rnd(v, dt)
    rs = 1.0 / torch.sqrt((x * x).mean(dim=-1, keepdim=True) + eps)
    n = R(w * x * rs) if mutant == "gain_before_round" else R(w * R(x * rs))
    n0, n1 = n[..., :64], n[..., 64:]
    sg = -1.0 if mutant == "rope_sign" else 1.0
    a0, b0 = R(n0 * cos), R(-sg * n1 * sin)
    a1, b1 = R(n1 * cos), R(sg * n0 * sin)
    out = torch.cat([R(a0 + b0), R(a1 + b1)], dim=-1)
    ab = torch.cat([a0.abs() + b0.abs(), a1.abs() + b1.abs()], dim=-1)
    return out, ab


def tie_margin(x, eps):
    """Smallest relative distance of an element of the float64 x * rs to a bf16 rounding tie (x [128])."""
    y = (x / torch.sqrt((x * x).mean() + eps)).abs()
    y = y[y > 0]
    u = torch.pow(2.0, torch.floor(torch.log2(y)) - 7)          # bf16 ulp in y's binade
    frac = torch.remainder(y / u, 1.0)
    return float(((frac - 0.5).abs() * u / y).min()) if y.numel() else float("inf")


def draw_head(gen, dt, eps, sigma=1.0):
    """One 128-vector of T values, tie-free for bf16; returns (x, redraws)."""
    for n in range(MAX_REDRAWS + 1):
        x = rnd(torch.randn(HD, generator=gen, dtype=F64) * sigma, dt)
        if dt != "bf16" or tie_margin(x, eps) > TAU:
            return x, n
    raise RuntimeError("no tie-free vector within MAX_REDRAWS draws")


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_cache(dt, kind, n_kv, max_seq, seed):
    """The cache rows every case of (dt, kind) shares: K, V [n_kv][max_seq][128] (callers never modify them)."""
    gen = torch.Generator().manual_seed(77_000 + seed)
    if kind == "which":
        # V row j = (1 + j // 128) * unit(j % 128); scores within a unit of each other: output dim d is the probability of key d (+ aliases)
        K = rnd(torch.randn(n_kv, max_seq, HD, generator=gen, dtype=F64) * 0.05, dt)
        V = torch.zeros(n_kv, max_seq, HD, dtype=F64)
        j = torch.arange(max_seq)
        V[:, j, j % HD] = (1 + j // HD).to(F64)
    else:
        K = rnd(torch.randn(n_kv, max_seq, HD, generator=gen, dtype=F64), dt)
        V = rnd(torch.randn(n_kv, max_seq, HD, generator=gen, dtype=F64), dt)
    return K, V


@functools.lru_cache(maxsize=None)
def base_gains(dt, kind):
    """Per-head RMSNorm gains around 1 (the lanes of a batch launch share them); "which": a small k gain keeps the own key's score
    within a unit of the others."""
    gen = torch.Generator().manual_seed(4242)
    qw = rnd(1.0 + 0.1 * torch.randn(HD, generator=gen, dtype=F64), dt)
    kw = rnd((0.1 if kind == "which" else 1.0) * (1.0 + 0.1 * torch.randn(HD, generator=gen, dtype=F64)), dt)
    return qw, kw


@functools.lru_cache(maxsize=None)
def base_rope(pos):
    """The RoPE row of a position (fp32 cos / sin of 64 seeded random angles: every sign combination occurs).  It depends on the
    position alone: the lanes of a predictor launch share one row."""
    gen = torch.Generator().manual_seed(31_000 + pos)
    th = torch.rand(64, generator=gen, dtype=F64) * (2.0 * math.pi)
    return rnd(torch.cos(th), "f32"), rnd(torch.sin(th), "f32")


@dataclass
class Case:
    dt: str
    kind: str
    n_kv: int
    rep: int
    pos: int
    n_pad: int
    max_seq: int
    eps: float
    scale: float
    qkv: torch.Tensor        # [(rep + 2) * n_kv * 128]
    qw: torch.Tensor
    kw: torch.Tensor
    cos: torch.Tensor
    sin: torch.Tensor
    Kb: torch.Tensor         # shared base rows [n_kv][max_seq][128]
    Vb: torch.Tensor
    redraws: int = 0         # the largest redraw count of one head

    @property
    def q_dim(self):
        return self.n_kv * self.rep * HD

    def cache_image(self):
        """The logical cache before the launch: live rows the base, rows >= pos NaN (the caller writes the sentinel bits there), rows
        < n_pad large finite values: V +/- 2^60 in every such row, K +/- 2^60 in every second one counted from the edge -- row
        n_pad - 1, n_pad - 3, ... keep an ordinary K, so that a kernel that takes such a row cannot miss its V by the sign of a score."""
        out = []
        for X, is_k in ((self.Kb, True), (self.Vb, False)):
            X = X.clone()
            X[:, self.pos:] = float("nan")
            n = min(self.n_pad, self.pos)
            if n:
                r = torch.arange(n)
                sign = 1.0 - 2.0 * ((r[:, None] + torch.arange(HD)[None, :]) % 2).to(F64)
                big = ((self.n_pad - 1 - r) % 2 == 1) if is_k else torch.ones(n, dtype=torch.bool)
                X[:, r[big]] = (BIG * sign)[big]
            out.append(X)
        return out


@functools.lru_cache(maxsize=None)
def make_case(dt, kind, n_kv, rep, pos, n_pad, max_seq, seed=0) -> Case:
    gen = torch.Generator().manual_seed(((seed * 1009 + pos) * 1009 + n_pad) * 1009 + rep * 16 + n_kv * 4 + (kind == "which") * 2 + (dt == "bf16"))
    eps, scale = 1e-6, 1.0 / math.sqrt(HD)
    Kb, Vb = base_cache(dt, kind, n_kv, max_seq, seed)
    heads, worst = [], 0
    for h in range(n_kv * rep + n_kv):            # q heads and the new k: through the norm, tie-free
        x, n = draw_head(gen, dt, eps, sigma=1.0 + 0.5 * (h % 3))
        heads.append(x)
        worst = max(worst, n)
    if kind == "which":
        v = torch.zeros(n_kv, HD, dtype=F64)
        v[:, pos % HD] = float(1 + pos // HD)
    else:
        v = rnd(torch.randn(n_kv, HD, generator=gen, dtype=F64), dt)
    qkv = torch.cat(heads + [v.flatten()])
    qw, kw = base_gains(dt, kind)
    cos, sin = base_rope(pos)
    return Case(dt, kind, n_kv, rep, pos, n_pad, max_seq, eps, scale, qkv, qw, kw, cos, sin, Kb, Vb, worst)


# ---- the cases of the GPU module (shared with the CPU self-test, which runs the float32 model on every one) -------------------
MAX_SEQ = 640
POS_NOPAD = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129, 200, 255, 256, 511, 512, 513, 575, 576, 639]
POS_PAD = [(p, n) for n in (5, 64, 70) for p in (64, 65, 130, 200)] + [(5, 5), (70, 70)]
POSITIONS = [(p, 0) for p in POS_NOPAD] + POS_PAD                   # (pos, n_pad), max_seq = 640
LANE_NI2_EXTRA = [(64 * t + r, 0) for t, r in ((0, 7), (1, 8), (2, 9), (0, 23), (3, 24), (5, 25))]     # pos % 64 around NI = 2 steps
CLAMP_CASE = dict(max_seq=200, S=4, positions=[(0, 0), (63, 0), (64, 5), (130, 70), (191, 0), (192, 0), (199, 0)])
PRED_POSITIONS = list(range(17))
N_KV = 2
REPS = (1, 2, 4)
WORKERS = (1, 3, 8)
KINDS = ("random", "which")


BATCH3 = [(0, 0), (200, 70), (130, 5)]                               # three different lanes of one launch (lane l: seed l)


def gpu_cases():
    """Every (dt, kind, rep, pos, n_pad, max_seq, seed) the GPU module launches."""
    out = []
    for dt in ("f32", "bf16"):
        for kind in KINDS:
            for rep in REPS:
                for pos, n_pad in POSITIONS + LANE_NI2_EXTRA:
                    out.append((dt, kind, rep, pos, n_pad, MAX_SEQ, 0))
                for seed, (pos, n_pad) in enumerate(BATCH3):
                    out.append((dt, kind, rep, pos, n_pad, MAX_SEQ, seed))
                for pos, n_pad in CLAMP_CASE["positions"]:
                    out.append((dt, kind, rep, pos, n_pad, CLAMP_CASE["max_seq"], 0))
            for pos in PRED_POSITIONS:
                for seed in range(3):
                    out.append((dt, kind, 2, pos, 0, 17, seed))
    return out


# ---- reference -------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    out: torch.Tensor            # [n_kv * rep][128] float64, not rounded
    A: torch.Tensor              # [n_kv * rep][128]
    Bmax: torch.Tensor           # [n_kv * rep]
    n_keys: int
    q: torch.Tensor              # [n_kv * rep][128] rotated q (T values)
    k_new: torch.Tensor          # [n_kv][128]
    v_new: torch.Tensor
    k_ab: torch.Tensor           # |a| + |b| of the new k
    rho: float                   # max over heads / keys of sum (|a| + |b|) |k| / sum |q k| (q and the own k)
    S: int = 0
    p_num: Optional[torch.Tensor] = None      # [n_kv][S][rep][128]
    p_A: Optional[torch.Tensor] = None
    p_m: Optional[torch.Tensor] = None        # [n_kv][S][rep]
    p_l: Optional[torch.Tensor] = None


def reference(c: Case, S: int = 0, *, mutant: str = "", drop=(), extra=()) -> Ref:
    """The token's attention over its cache.  S > 0 also returns the per-worker partials.  Deliberate defects (the checker's
    self-test): mutant in {rope_sign, gain_before_round, no_own, own_twice, v_other_head}; drop / extra: cache keys left out / taken
    although dead."""
    n_kv, rep, pos, n_pad = c.n_kv, c.rep, c.pos, c.n_pad
    nq = n_kv * rep
    xq = c.qkv[:nq * HD].view(nq, HD)
    xk = c.qkv[nq * HD:(nq + n_kv) * HD].view(n_kv, HD)
    v_new = c.qkv[(nq + n_kv) * HD:].view(n_kv, HD)
    nm = mutant if mutant in ("rope_sign", "gain_before_round") else ""
    q, q_ab = head_norm_rope(xq, c.qw, c.cos, c.sin, c.eps, c.dt, mutant=nm)
    k_new, k_ab = head_norm_rope(xk, c.kw, c.cos, c.sin, c.eps, c.dt, mutant=nm)
    K, V = c.cache_image()
    idx = [j for j in range(n_pad, pos) if j not in drop] + [j for j in extra]
    idx = torch.tensor(idx, dtype=torch.long)
    own = 0 if (pos < n_pad or mutant == "no_own") else (2 if mutant == "own_twice" else 1)
    tiles = torch.cat([idx // KS, torch.full((own,), pos // KS, dtype=torch.long)])
    n = len(tiles)
    out = torch.zeros(nq, HD, dtype=F64)
    A = torch.zeros(nq, HD, dtype=F64)
    Bmax = torch.zeros(nq, dtype=F64)
    rho = 0.0
    if S:
        p_num = torch.zeros(n_kv, S, rep, HD, dtype=F64)
        p_A = torch.zeros(n_kv, S, rep, HD, dtype=F64)
        p_m = torch.full((n_kv, S, rep), EMPTY_M, dtype=F64)
        p_l = torch.zeros(n_kv, S, rep, dtype=F64)
    for g in range(n_kv):
        Kall = torch.cat([K[g][idx]] + [k_new[g][None]] * own)
        Vall = torch.cat([V[g][idx]] + [v_new[g][None]] * own)
        if mutant == "v_other_head" and len(idx):                  # one V row (the middle live key) from the neighbouring kv head
            Vall[len(idx) // 2] = V[(g + 1) % n_kv][idx[len(idx) // 2]]
        qg = q[g * rep:(g + 1) * rep]
        s = c.scale * qg @ Kall.t()                                  # [rep][n]
        B = c.scale * qg.abs() @ Kall.abs().t()
        Bq = c.scale * q_ab[g * rep:(g + 1) * rep] @ Kall.abs().t()
        if own:
            Bq[:, -1] = torch.maximum(Bq[:, -1], c.scale * qg.abs() @ k_ab[g])
        if n:
            rho = max(rho, float((Bq / B.clamp_min(1e-300)).max()))
            m = s.max(dim=1, keepdim=True).values
            p = torch.exp(s - m)
            l = p.sum(dim=1, keepdim=True)
            out[g * rep:(g + 1) * rep] = (p @ Vall) / l
            A[g * rep:(g + 1) * rep] = (p @ Vall.abs()) / l
            Bmax[g * rep:(g + 1) * rep] = B.max(dim=1).values
        for w in range(S):
            sel = (tiles % S) == w
            if not bool(sel.any()):
                continue
            sw = s[:, sel]
            mw = sw.max(dim=1, keepdim=True).values
            pw = torch.exp(sw - mw)
            p_num[g, w] = pw @ Vall[sel]
            p_A[g, w] = pw @ Vall[sel].abs()
            p_m[g, w] = mw[:, 0]
            p_l[g, w] = pw.sum(dim=1)
    r = Ref(out, A, Bmax, n, q, k_new, v_new, k_ab, rho)
    if S:
        r.S, r.p_num, r.p_A, r.p_m, r.p_l = S, p_num, p_A, p_m, p_l
    return r


def merge(num, m, l, n_part, *, swap=None):
    """float64 merge of partial slots num [..., S, rep, 128], m / l [..., S, rep] over the first n_part slots; returns (out, A).
    swap = (s, t): the weights of slots s and t exchanged (a mutant)."""
    num, m, l = num[..., :n_part, :, :], m[..., :n_part, :], l[..., :n_part, :]
    M = m.max(dim=-2, keepdim=True).values
    w = torch.exp(m - M)
    if swap:
        w = w.clone()
        s, t = swap
        w[..., [s, t], :] = w[..., [t, s], :]
    den = (w * l).sum(dim=-2)
    inv = torch.where(den > 0, 1.0 / den.clamp_min(1e-300), torch.zeros_like(den))[..., None]      # every slot empty: zeros
    return (w[..., None] * num).sum(dim=-3) * inv, (w[..., None] * num.abs()).sum(dim=-3) * inv


# ---- checker ---------------------------------------------------------------------------------------------------------------------
def gamma(n_keys: int) -> float:
    return 2.0 * (math.ceil(n_keys / 16) + 16) * (EXP_REL + 2.0 * U32)


def delta_max(ref: Ref) -> torch.Tensor:
    return C_S * U32 * ref.Bmax                       # per head


def e_bound(ref: Ref) -> torch.Tensor:
    """E per head: 2 max_j delta_j + gamma."""
    return 2.0 * delta_max(ref) + gamma(ref.n_keys)


@dataclass
class Verdict:
    ok: bool
    ratio: float            # largest err / bound
    exact: float
    msg: str

    def __bool__(self):
        return self.ok


def _bounded(got, ref, bound, what, names, exact_ref=None, f=0.0):
    err = (got - ref).abs()
    err = torch.where(torch.isnan(got), torch.full_like(err, float("inf")), err)
    ratio_t = err / bound.clamp_min(1e-300)
    ratio_t = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), ratio_t)
    ratio = float(ratio_t.max()) if ratio_t.numel() else 0.0
    bad = err > bound
    exact = float((got == exact_ref).double().mean()) if exact_ref is not None and got.numel() else 1.0
    ok = not bool(bad.any()) and exact >= f
    msg = ""
    if not ok:
        i = int(torch.argmax(ratio_t))
        at = [int(v) for v in np.unravel_index(i, tuple(got.shape))]
        msg = (f"{what}: {int(bad.sum())} / {got.numel()} elements out of bound, worst err / bound {ratio:.3g} at {dict(zip(names, at))}: "
               f"got {float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}; exact fraction {exact:.4f} (need {f})")
    return Verdict(ok, ratio, exact, msg)


def check_output(got, ref: Ref, dt: str, *, stored=True, what="", out=None, A=None, E=None) -> Verdict:
    """got [heads][128] float64 (a final, normalised output).  |got - ref| <= E A (+ half a T-ulp of ref where stored in T); bf16
    stored: exact-rounding fraction >= F_EXACT."""
    out = ref.out if out is None else out
    A = ref.A if A is None else A
    E = e_bound(ref)[:, None] if E is None else E
    bound = E * A
    if stored:
        bound = bound + 0.5 * ulp(out.abs() + bound, dt)
    is_bf = stored and dt == "bf16"
    return _bounded(got, out, bound, what, ("head", "dim"), rnd(out, dt) if is_bf else None, F_EXACT if is_bf else 0.0)


def check_kv_row(got_k, got_v, ref: Ref, dt: str, what="") -> Verdict:
    """The appended row of every kv head: got_k / got_v [n_kv][128] float64."""
    if not bool((got_v == ref.v_new).all()):
        return Verdict(False, float("inf"), 0.0, f"{what}: appended V row differs from the token's v")
    bound = torch.zeros_like(ref.k_ab) if dt == "bf16" else C_K * U32 * ref.k_ab
    return _bounded(got_k, ref.k_new, bound, what + " appended K row", ("kv head", "dim"))


def check_partials(part, ref: Ref, what="") -> Verdict:
    """part [n_kv][8][rep][132] float64: the kernel's slots for the S workers of ref (slots >= S are not looked at)."""
    S = ref.S
    n_kv, rep = part.shape[0], part.shape[2]
    num, m, l = part[:, :S, :, :HD], part[:, :S, :, HD], part[:, :S, :, HD + 1]
    if bool(torch.isnan(part[:, :S, :, :HD + 2]).any()):
        return Verdict(False, float("inf"), 0.0, f"{what}: NaN in a partial slot")
    empty = ref.p_l == 0
    if not (bool((m[empty] == EMPTY_M).all()) and bool((l[empty] == 0).all()) and bool((num[empty] == 0).all())):
        return Verdict(False, float("inf"), 0.0, f"{what}: an empty worker's slot is not {{0, m = -1e30, l = 0}}")
    if bool(((l == 0) & ~empty).any()):
        return Verdict(False, float("inf"), 0.0, f"{what}: a worker with keys left an empty slot")
    E = e_bound(ref).view(n_kv, 1, rep)
    dm = delta_max(ref).view(n_kv, 1, rep).expand(n_kv, S, rep)
    live = ~empty
    v = _bounded(torch.where(live, m, ref.p_m), ref.p_m, dm + 0.5 * ulp(ref.p_m, "f32"), what + " slot maximum", ("kv head", "worker", "q head"))
    if not v:
        return v
    resc = torch.where(live, torch.exp(m - ref.p_m), torch.ones_like(m))
    v2 = _bounded(l * resc, ref.p_l, E * ref.p_l, what + " slot sum", ("kv head", "worker", "q head"))
    if not v2:
        return v2
    v3 = _bounded(num * resc[..., None], ref.p_num, E[..., None] * ref.p_A, what + " slot numerator", ("kv head", "worker", "q head", "dim"))
    if not v3:
        return v3
    mo, _ = merge(num, m, l, S)
    v4 = check_output(mo.reshape(n_kv * rep, HD), ref, "f32", stored=False, what=what + " float64 merge of the slots")
    if not v4:
        return v4
    return Verdict(True, max(v.ratio, v2.ratio, v3.ratio, v4.ratio), 1.0, "")


def check_merge(got, num, m, l, n_part, dt, what="") -> Verdict:
    """The merge alone on given slots: got [n_kv * rep][128] against the float64 merge; E = gamma(n_part) (the slots are exact inputs)."""
    out, A = merge(num, m, l, n_part)
    shape = (-1, HD)
    return check_output(got, None, dt, what=what, out=out.reshape(shape), A=A.reshape(shape), E=torch.tensor(gamma(n_part), dtype=F64))


# ---- a plain float32 model of the same operation (straight softmax, no tiling): the bound must admit it ------------------------
def float32_model(c: Case):
    """Everything in torch.float32 (rounding to T where the contract rounds); returns (out [heads][128] stored in T, k_new, v_new) as
    float64."""
    f32 = torch.float32
    T = (lambda v: v.to(torch.bfloat16).to(f32)) if c.dt == "bf16" else (lambda v: v)
    nq, n_kv, rep = c.n_kv * c.rep, c.n_kv, c.rep

    def nr(x, w):
        x, w = x.to(f32), w.to(f32)
        rs = 1.0 / torch.sqrt((x * x).sum(dim=-1, keepdim=True) / HD + f32_scalar(c.eps))
        n = T(w * T(x * rs))
        n0, n1 = n[..., :64], n[..., 64:]
        cs, sn = c.cos.to(f32), c.sin.to(f32)
        return torch.cat([T(T(n0 * cs) + T(-n1 * sn)), T(T(n1 * cs) + T(n0 * sn))], dim=-1)

    q = nr(c.qkv[:nq * HD].view(nq, HD), c.qw)
    k_new = nr(c.qkv[nq * HD:(nq + n_kv) * HD].view(n_kv, HD), c.kw)
    v_new = c.qkv[(nq + n_kv) * HD:].view(n_kv, HD).to(f32)
    out = torch.zeros(nq, HD, dtype=f32)
    for g in range(n_kv):
        Kall, Vall = c.Kb[g, c.n_pad:c.pos].to(f32), c.Vb[g, c.n_pad:c.pos].to(f32)
        if c.pos >= c.n_pad:
            Kall, Vall = torch.cat([Kall, k_new[g][None]]), torch.cat([Vall, v_new[g][None]])
        if not len(Kall):              # pos < n_pad: no valid key at all, the output is zero
            continue
        s = (q[g * rep:(g + 1) * rep] @ Kall.t()) * f32_scalar(c.scale)
        p = torch.exp(s - s.max(dim=1, keepdim=True).values)
        out[g * rep:(g + 1) * rep] = (p @ Vall) / p.sum(dim=1, keepdim=True)
    return T(out).to(F64), k_new.to(F64), v_new.to(F64)


def f32_scalar(v):
    return torch.tensor(v, dtype=torch.float32)
