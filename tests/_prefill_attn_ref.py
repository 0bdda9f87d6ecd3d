"""Float64 reference of the prefill and windowed attention contracts (csrc/prefill_kernels.cuh, csrc/codec_kernels.cuh,
csrc/refenc_kernels.cuh) and element-wise checkers, in the form of tests/_attn_ref.py (whose helpers it reuses).

Written from the documented contract (the header comment of csrc/fq3_prefill.hip, the comments above each kernel, the paged layout
comment above ``PagedKV``), not from the kernel bodies:

* paged layout: the pool is ``[n_blocks][n_kv][64][128]``; row ``key`` of kv head g lives in slot ``key % 64`` of block
  ``table[key / 64]``.  One prompt row of qkv is ``[q (NH heads) | k (NKV heads) | v (NKV heads)]``, head dim 128; q head h attends to
  kv head ``h / (NH / NKV)``.
* norm + RoPE + K/V write (``qk_norm_rope_kv_kernel``, ``qk_norm_rope_kv_pack_kernel``): for every row ``t >= n_pad``: per head RMSNorm
  then rotate_half RoPE of every q head (in place) and every k head (to the cache), one rounding to T per op exactly as
  ``_attn_ref.head_norm_rope``; the RoPE row is ``clamp(t + rope_delta, 0, rope_len - 1)``; v is copied.  Rows ``t < n_pad`` are untouched
  everywhere (qkv and cache).  The packed form does this for every sequence of the pack with that sequence's own rows, n_pad,
  rope_delta and block table; positions restart at 0 in every sequence.
* causal attention (``prefill_attn_kernel``, ``flash_prefill_kernel``, ``flash_prefill_small_kernel``): query row t attends to the keys
  ``n_pad <= j <= t`` of its kv head, scores ``scale * q . k_j``, softmax in fp32, one rounding to T.  Output rows ``t < n_pad`` are exact
  zeros, rows ``>= L`` are untouched.  The flash kernels multiply P = 0 by what the dead rows of owned blocks hold (finite by contract),
  the wave kernel never reads them.
* windowed attention (``swa_attn_kernel``, ``win_attn_kernel``) over qkv ``[batch][Tn][q | k | v of NH * HD]``: query q attends to the keys
  ``max(0, q - window + 1) .. q``; rows below ``row_lo`` and beyond Tn are untouched; every batch index restarts positions at 0.
* ``rope_rows_kernel``: the q and k thirds of rows ``[row_lo, Tn)``, rotate_half convention, position = row: dims j < HD/2:
  ``rnd(x_j cos_j) + rnd(-x_{j+HD/2} sin_j)``, dims j + HD/2: ``rnd(x_{j+HD/2} cos_j) + rnd(x_j sin_j)``; the products are rounded to T, the sum
  is rounded on store.

Everything is float64 (products of bf16 / fp32 operands are exact there).  Alongside an attention output ride the scales of its bound,
as in _attn_ref: ``A_d = sum_j p_j |v_jd|`` and ``B = max_j scale * sum_d |q_d k_jd|``.

Checker: ``|got - ref| <= E * A_d`` plus half a T-ulp where the kernel stores T, ``E = 2 max_j delta_j + gamma``.  u = 2^-24.
* K / V rows and the rotated q of the norm kernels: the rule of _attn_ref (its tie-free generator, TAU and C_K are reused: the
  kernels' sum of squares is "2 per lane + a 6-level tree", one of the two arrangements TAU was derived for): bf16 bit-exact on tie-free
  inputs, fp32 within ``C_K u (|a| + |b|)``, v bit-exact.
* ``delta_j = C * u * B_j``.  The attention kinds take q and the cache as EXACT inputs (no norm in front), so only the dot product
  counts: an HD-term fp32 sum however it is ordered (HD u; the MFMA's products of bf16 operands are exact, its fp32 accumulation is
  such a sum), + 1 u for ``* scale``, + for the flash kernels 1.5 u for ``scale * log2(e)`` (the constant and the product) and, for every
  kernel, 2 u for the rounding of ``s - max`` (|s - max| <= 2 B): C = HD + 4.5, rounded up to C_SP = 134 for HD = 128 and HD + 6 for the
  windowed kernels.
* online-softmax steps, from each kernel's documented layout; every step is one exponential (rescale or probability) and two roundings
  (fma + product), times 2 for numerator and denominator:
  - wave kernel: "16 lanes per key, 16 keys in flight per trip": four 16-lane groups, each takes 4 keys of every trip of 16 one after
    the other, so a term passes at most ``4 ceil(n / 16)`` steps in its group, + 2 merges across the groups + 2 (normalisation, store):
    ``gamma_wave(n) = 2 (4 ceil(n / 16) + 4) (EXP_REL + 2 u)``, EXP_REL the __expf constant of _attn_ref.
  - flash: one step per 64-key tile the row has live keys in (``tiles = t / 64 - n_pad / 64 + 1``; a tile that is wholly masked for the row
    rescales by exp2(0) = 1 and adds zeros: exact), + 1 for the normalisation: ``2 (tiles + 1) (EXP2_REL + 2 u)``; inside the tiles the
    numerator is a sum of 2 n fp32 terms (bf16 hi + residual of every probability) and the denominator of n, however ordered: 3 n u;
    and the two bf16 parts leave a relative 2^-16 on each probability, as the kernel comment says: ``gamma_flash(n, tiles) =
    2 (tiles + 1) (EXP2_REL + 2 u) + 3 n u + 2^-16``.
  - windowed: one single-pass softmax (one exponential, the rounding of its argument and of the sum's terms) plus an nk-term fma chain
    for the numerator and a wave sum (at most 8 roundings) for the denominator, the division and the store:
    ``gamma_win(nk) = 2 (EXP + 2 u) + 2 (nk + 8) u``, EXP = EXP_REL (__expf) for swa_attn_kernel and EXPF_REL for win_attn_kernel.
* exponentials, measured on the MI355X against float64 on the grid of attn_probe_expf (2^16 + 1 arguments in [-90, 0]; results below
  2^-126 are flushed and excluded), the constant twice the measured maximum
  (tests/test_gpu_prefill_attn_reference.py::test_exp_grids asserts measured <= constant / 2):
  - exp2f: measured 8.14e-8 (at x = -61.94; the argument is already in base 2, so the error does not grow with |x| as __expf's does),
    EXP2_REL = 1.63e-7; no result of the grid is below 2^-126.
  - expf: measured 7.805e-8 (at x = -46.40), EXPF_REL = 1.57e-7; below 2^-126 the largest absolute error was 1.22e-45.
* bf16 exact fraction (the share of stored elements equal to rnd(ref), over the rows the kernel computes): the wave and the windowed
  kernels keep F_EXACT = 0.99 of _attn_ref.  For the flash kernels the floor is derived from the bound, per case, before anything runs:
  an element flips when a rounding tie lies within its error of the reference; ties are one bf16 ulp apart, so an error e flips an
  element with probability e over the half-ulp h_d = ulp(ref_d) / 2, at most ``r = mean_d min(1, E A_d / h_d)`` of the elements on
  average, and the count of N elements fluctuates by sqrt(r / N): ``floor = min(F_EXACT, 1 - r - 3 sqrt(r / N))``.  With E >= 2^-16 against
  h_d ~ 2^-8.5 |ref_d| that is r >= 0.0055 A_d / |ref_d|: about 0.98 on the "which key" operands (A_d = |ref_d|, scores within a
  unit) and 0.33 .. 0.94 on the random ones, whose E is dominated by 2 delta (B ~ 10) and whose sums cancel (A_d ~ 3 |ref_d|).  The
  observed fractions are recorded in tests/test_gpu_prefill_attn_reference.py beside these floors; no floor is set from them.
* rope_rows: bf16 bit-exact (every op is one correctly rounded fp32 operation followed by the rounding to bf16, which the reference
  reproduces; no tie condition is needed as no inexact intermediate is rounded twice differently); fp32: T = float has no rounding
  between the products and their sum, so the compiler may fuse one product into the sum: both forms stay within one rounding per
  op of the exact value: ``|got - ref| <= C_ROPE u (|a| + |b|)``, C_ROPE = 4 (3 roundings of at most u (|a| + |b|) in the reference,
  at most as many in the kernel, |a + b| <= |a| + |b|: 2 + 2).
See tests/test_gpu_prefill_attn_reference.py for the values observed on the MI355X.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

import _attn_ref as A
from _attn_ref import BIG, C_K, EXP_REL, F_EXACT, HD, KS, MAX_REDRAWS, U32, Verdict, _bounded
from _gemm_ref import F64, rnd, ulp

C_SP = 134.0
EXP2_REL = 1.63e-7
EXPF_REL = 1.57e-7
SPLIT_REL = 2.0 ** -16
C_ROPE = 4.0
KINDS = A.KINDS
N_KV = A.N_KV
REPS = A.REPS                     # rep 2 and 4: the shipped talker configs; 1: no GQA
NH_MAX = N_KV * max(REPS)
L_MAX = 448                       # 64 ceil(400 / 64): the longest prompt's whole tiles
N_NORM_ROWS = 400                 # rows of the shared pre-norm pool (the longest pack holds 394)
EPS = 1e-6
SCALE = 1.0 / math.sqrt(HD)

# ---- the cases of the GPU module (shared with the CPU self-test) -------------------------------------------------------------------
L_LIST = [1, 16, 17, 63, 64, 65, 128, 129, 200, 256, 257, 321]


def pads(L):
    return sorted({p for p in (0, 1, 63, 64, 65, L - 1) if 0 <= p < L})


WAVE_CASES = sorted({(L, p) for L in L_LIST for p in pads(L)} | {(200, 130), (65, 64)})       # also flash <4,false>
PAIRED4_CASES = [(L, p) for L in (64, 65, 129, 200, 321) for p in (0, 70) if p < L]         # block counts 1, 2, 3 (middle block), 4, 6
PAIRED8_CASES = [(L, p) for L in (100, 129, 257, 400) for p in (0, 70)]                      # block counts 1, 2, 3, 4
SMALL_CASES = [(L, p) for L, p in WAVE_CASES if L <= 256]
# packs: (L, n_pad, rope_delta) per sequence
PACK3 = [(200, 70, -7), (65, 0, 40), (129, 64, 0)]
PACK_MIXED = [(17, 0, 0), (256, 65, 3)]                                                       # grid.x is sized by Lmax
PACK64 = [(1 + q % 5, 1 if (q % 3 == 0 and q % 5 > 0) else 0, q - 30) for q in range(64)]
PACKS = {"pack3": PACK3, "mixed": PACK_MIXED, "pack64": PACK64}
ROPE_LEN = 300
ROPE_DELTAS = (0, -7, 40)                                                                      # t + delta below 0, beyond rope_len - 1

SWA_TN = (1, 3, 4, 5, 65, 130)
SWA_WINDOWS = (1, 2, 64, 65, 72, 127, 128)
WIN_TN = (1, 5, 64, 65, 250, 251, 300)
WIN_WINDOWS = (1, 64, 65, 129, 250)
WIN_INST = [(hd, np_) for hd in (32, 64, 128) for np_ in (1, 2, 3, 4)]                         # what fq3_refenc.hip instantiates
W_NH = 2


def swa_row_los(Tn):
    return sorted({r for r in (0, 3, Tn - 1) if 0 <= r < Tn})


def win_cases(np_):
    """(Tn, window) a win_attn_kernel<HD, NP> launch admits: min(window, Tn) <= 64 NP; and the largest window NP admits."""
    out = {(Tn, w) for Tn in WIN_TN for w in WIN_WINDOWS + (64 * np_,) if min(w, Tn) <= 64 * np_}
    return sorted(out)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_q(dt, seed):
    """q rows [L_MAX][NH_MAX][128] every paged attention case of dt shares (already normed and rotated as far as the kernel knows)."""
    gen = torch.Generator().manual_seed(55_000 + seed)
    return rnd(torch.randn(L_MAX, NH_MAX, HD, generator=gen, dtype=F64), dt)


@dataclass(frozen=True)
class Seq:
    """One prompt for the causal attention kinds: q [L][NH][128], K / V [n_kv][L][128] (T values as float64; never modified)."""
    dt: str
    kind: str
    n_kv: int
    rep: int
    L: int
    n_pad: int
    seed: int = 0

    @property
    def NH(self):
        return self.n_kv * self.rep

    @property
    def q(self):
        return base_q(self.dt, self.seed)[:self.L, :self.NH]

    @property
    def KV(self):
        K, V = A.base_cache(self.dt, self.kind, self.n_kv, L_MAX, self.seed)
        return K[:, :self.L], V[:, :self.L]

    def dead_rows(self, finite):
        """The rows of the owned blocks no key may come from: rows < n_pad and the rows L .. 64 ceil(L / 64) - 1 of the last tile,
        as (K, V) images [n_kv][rows][128] for the whole tiles: NaN (finite False) or, finite, V +/- 2^60 everywhere and K +/- 2^60 in every
        second row counted from the live edge (the others an ordinary K, so that a kernel that takes such a row cannot miss its V by the
        sign of a score)."""
        n_rows = KS * ((self.L + KS - 1) // KS)
        K = torch.full((self.n_kv, n_rows, HD), float("nan"), dtype=F64)
        V = K.clone()
        Kl, Vl = self.KV
        K[:, self.n_pad:self.L], V[:, self.n_pad:self.L] = Kl[:, self.n_pad:], Vl[:, self.n_pad:]
        if finite:
            r = torch.arange(n_rows)
            dead = (r < self.n_pad) | (r >= self.L)
            sign = 1.0 - 2.0 * ((r[:, None] + torch.arange(HD)[None, :]) % 2).to(F64)
            dist = torch.where(r < self.n_pad, self.n_pad - 1 - r, r - self.L)
            V[:, dead] = (BIG * sign)[dead]
            big_k = dead & (dist % 2 == 1)
            K[:, big_k] = (BIG * sign)[big_k]
            small_k = dead & ~big_k
            K[:, small_k] = base_q(self.dt, 7)[:n_rows, 0][small_k]
        return K, V


def to_pool(X, table, n_blocks):
    """[n_kv][64 * tiles][128] -> the pool image [n_blocks][n_kv][64][128] through the block table; unowned blocks NaN."""
    n_kv, rows, _ = X.shape
    pool = torch.full((n_blocks, n_kv, KS, HD), float("nan"), dtype=F64)
    for t in range(rows // KS):
        pool[table[t]] = X[:, t * KS:(t + 1) * KS]
    return pool


def from_pool(pool, table, rows):
    """The logical rows [n_kv][rows][128] a reader of `table` sees."""
    tiles = (rows + KS - 1) // KS
    return torch.cat([pool[table[t]] for t in range(tiles)], dim=1)[:, :rows]


def shuffled_table(n_tiles, n_blocks, seed):
    g = torch.Generator().manual_seed(9000 + seed)
    t = torch.randperm(n_blocks, generator=g)[:n_tiles].tolist()
    if t == sorted(t) and n_tiles > 1:
        t = t[::-1]                                  # (shuffled AND non-monotonic)
    if n_tiles == 1 and t[0] == 0:
        t = [n_blocks - 1]                           # never the identity
    return t


# ---- causal attention ----------------------------------------------------------------------------------------------------------------
@dataclass
class AttnRef:
    out: torch.Tensor            # [L][NH][128] float64, not rounded; rows < n_pad zero
    A: torch.Tensor
    Bmax: torch.Tensor           # [L][NH]
    n_keys: torch.Tensor         # [L]
    tiles: torch.Tensor          # [L] 64-key tiles with a live key of the row
    n_pad: int


def attn_reference(q, K, V, n_pad, scale=SCALE, *, mutant="") -> AttnRef:
    """q [L][NH][HD], K / V [n_kv][L][HD].  Deliberate defects (the checker's self-test): mutant in {causal_minus (key t dropped),
    causal_plus (key t + 1 taken), pad_gt (j > n_pad), kv_head (h % n_kv), v_pair_swap (V rows 2i and 2i + 1 exchanged)}."""
    L, NH, _ = q.shape
    n_kv = K.shape[0]
    rep = NH // n_kv
    t = torch.arange(L)
    hi = t - 1 if mutant == "causal_minus" else (t + 1 if mutant == "causal_plus" else t)
    lo = n_pad + 1 if mutant == "pad_gt" else n_pad
    mask = (t[None, :] <= hi[:, None]) & (t[None, :] >= lo)                      # [query][key]
    if mutant == "v_pair_swap":
        idx = t ^ 1
        idx[idx >= L] = L - 1
        V = V[:, idx]
    out = torch.zeros(L, NH, HD, dtype=F64)
    Aa = torch.zeros(L, NH, HD, dtype=F64)
    Bmax = torch.zeros(L, NH, dtype=F64)
    live = mask.any(dim=1)
    for h in range(NH):
        g = h % n_kv if mutant == "kv_head" else h // rep
        s = scale * q[:, h] @ K[g].t()
        B = scale * q[:, h].abs() @ K[g].abs().t()
        s = torch.where(mask, s, torch.full_like(s, -float("inf")))
        m = s.max(dim=1, keepdim=True).values
        p = torch.where(mask, torch.exp(s - torch.where(live[:, None], m, torch.zeros_like(m))), torch.zeros_like(s))
        l = p.sum(dim=1, keepdim=True).clamp_min(1e-300)
        Vg = V[g]
        out[:, h] = (p @ Vg) / l
        Aa[:, h] = (p @ Vg.abs()) / l
        Bmax[:, h] = torch.where(mask, B, torch.zeros_like(B)).max(dim=1).values
    dead_q = t < n_pad
    out[dead_q], Aa[dead_q], Bmax[dead_q] = 0.0, 0.0, 0.0
    n_keys = (t - n_pad + 1).clamp_min(0)
    tiles = (t // KS - n_pad // KS + 1).clamp_min(0)
    return AttnRef(out, Aa, Bmax, n_keys, tiles, n_pad)


@functools.lru_cache(maxsize=None)
def seq_reference(seq: Seq) -> AttnRef:
    K, V = seq.KV
    return attn_reference(seq.q, K, V, seq.n_pad)


def gamma_wave(n):
    return 2.0 * (4.0 * torch.ceil(n.to(F64) / 16.0) + 4.0) * (EXP_REL + 2.0 * U32)


def gamma_flash(n, tiles):
    return 2.0 * (tiles.to(F64) + 1.0) * (EXP2_REL + 2.0 * U32) + 3.0 * n.to(F64) * U32 + SPLIT_REL


def gamma_win(nk, exp_rel):
    return 2.0 * (exp_rel + 2.0 * U32) + 2.0 * (nk.to(F64) + 8.0) * U32


def attn_e(ref: AttnRef, kernel: str) -> torch.Tensor:
    """E per (row, head): 2 max_j delta_j + gamma of the kernel ("wave" or "flash")."""
    g = gamma_wave(ref.n_keys) if kernel == "wave" else gamma_flash(ref.n_keys, ref.tiles)
    return 2.0 * C_SP * U32 * ref.Bmax + g[:, None]


def flash_floor(ref: AttnRef, rows=None) -> float:
    """The derived floor of the bf16 exact fraction of a flash kernel over the live rows (see the module docstring)."""
    rows = slice(ref.n_pad, None) if rows is None else rows
    E = attn_e(ref, "flash")[rows, :, None]
    out, Aa = ref.out[rows], ref.A[rows]
    h = 0.5 * ulp(rnd(out, "bf16"), "bf16")
    r = float((E * Aa / h).clamp_max(1.0).mean()) if out.numel() else 0.0
    return min(F_EXACT, 1.0 - r - 3.0 * math.sqrt(r / max(1, out.numel())))


def check_attn(got, ref: AttnRef, dt, kernel, what="") -> Verdict:
    """got [L][NH][128] float64 as stored in T.  Rows < n_pad: exact zeros.  Live rows: the bound, and for bf16 the exact fraction."""
    if bool(torch.isnan(got).any()):
        return Verdict(False, float("inf"), 0.0, f"{what}: NaN in the output")
    if not bool((got[:ref.n_pad] == 0).all()):
        return Verdict(False, float("inf"), 0.0, f"{what}: an output row below n_pad is not exact zeros")
    rows = slice(ref.n_pad, None)
    out = ref.out[rows]
    bound = attn_e(ref, kernel)[rows, :, None] * ref.A[rows]
    bound = bound + 0.5 * ulp(out.abs() + bound, dt)
    f = 0.0 if dt != "bf16" else (F_EXACT if kernel == "wave" else flash_floor(ref))
    return _bounded(got[rows], out, bound, what, ("row", "head", "dim"), rnd(out, dt) if dt == "bf16" else None, f)


def attn_float32_model(q, K, V, n_pad, dt, scale=SCALE):
    """Plain torch.float32 causal attention (straight softmax), stored in T; returns float64."""
    f32 = torch.float32
    L, NH, _ = q.shape
    n_kv = K.shape[0]
    rep = NH // n_kv
    t = torch.arange(L)
    mask = (t[None, :] <= t[:, None]) & (t[None, :] >= n_pad)
    out = torch.zeros(L, NH, HD, dtype=f32)
    for h in range(NH):
        g = h // rep
        s = (q[:, h].to(f32) @ K[g].to(f32).t()) * torch.tensor(scale, dtype=f32)
        s = torch.where(mask, s, torch.full_like(s, -1e30))
        p = torch.where(mask, torch.exp(s - s.max(dim=1, keepdim=True).values), torch.zeros_like(s))
        out[:, h] = (p @ V[g].to(f32)) / p.sum(dim=1, keepdim=True).clamp_min(1e-30)
    out[t < n_pad] = 0.0
    return (out.to(torch.bfloat16).to(f32) if dt == "bf16" else out).to(F64)


# ---- norm + RoPE + K/V write -----------------------------------------------------------------------------------------------------------
def rope_row(p):
    return A.base_rope(p)


@functools.lru_cache(maxsize=None)
def rope_table(rope_len=ROPE_LEN):
    """cos / sin [rope_len][64] (fp32 values as float64)."""
    rows = [rope_row(p) for p in range(rope_len)]
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


@functools.lru_cache(maxsize=None)
def norm_rows(dt, n_rows, seed=0):
    """Prompt rows [n_rows][NH_MAX q | N_KV k | N_KV v heads][128] before the norm, every q and k head tie-free (the generator of
    _attn_ref); returns (rows, the largest redraw count)."""
    gen = torch.Generator().manual_seed(66_000 + seed)
    x = torch.empty(n_rows, NH_MAX + 2 * N_KV, HD, dtype=F64)
    worst = 0
    for t in range(n_rows):
        for h in range(NH_MAX + N_KV):
            x[t, h], n = A.draw_head(gen, dt, EPS, sigma=1.0 + 0.5 * (h % 3))
            worst = max(worst, n)
    x[:, NH_MAX + N_KV:] = rnd(torch.randn(n_rows, N_KV, HD, generator=gen, dtype=F64), dt)
    return x, worst


def norm_input(dt, rep, L, start=0):
    """[L][NH + 2 N_KV][128]: rows start .. start + L - 1 of the shared pool: their first NH q heads, k, v."""
    x, _ = norm_rows(dt, N_NORM_ROWS)
    NH = N_KV * rep
    return torch.cat([x[start:start + L, :NH], x[start:start + L, NH_MAX:]], dim=1)


@dataclass
class NormRef:
    q: torch.Tensor              # [L][NH][128]; rows < n_pad NaN (untouched)
    q_ab: torch.Tensor
    k: torch.Tensor              # [n_kv][L][128] the logical cache rows; rows < n_pad NaN
    k_ab: torch.Tensor
    v: torch.Tensor
    n_pad: int


def norm_reference(x, qw, kw, n_kv, n_pad, rope_delta, dt, rope_len=ROPE_LEN, eps=EPS, *, mutant="") -> NormRef:
    """x [L][NH + 2 n_kv][128].  mutant "rope_unclamped": the RoPE row of position t + rope_delta itself."""
    L, per, _ = x.shape
    NH = per - 2 * n_kv
    pos = torch.arange(L) + rope_delta
    if mutant == "rope_unclamped":
        rows = [rope_row(abs(int(p))) for p in pos]
        cos, sin = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
    else:
        ct, st = rope_table(rope_len)
        pos = pos.clamp(0, rope_len - 1)
        cos, sin = ct[pos], st[pos]
    q, q_ab = A.head_norm_rope(x[:, :NH], qw, cos[:, None], sin[:, None], eps, dt)
    k, k_ab = A.head_norm_rope(x[:, NH:NH + n_kv], kw, cos[:, None], sin[:, None], eps, dt)
    v = x[:, NH + n_kv:].clone()
    for X in (q, k, v):
        X[:n_pad] = float("nan")
    return NormRef(q, q_ab, k.transpose(0, 1).contiguous(), k_ab.transpose(0, 1).contiguous(), v.transpose(0, 1).contiguous(), n_pad)


def check_norm(got_q, got_k, got_v, ref: NormRef, dt, what="") -> Verdict:
    """got_q [L][NH][128], got_k / got_v [n_kv][L][128], the rows >= n_pad only are looked at (the caller checks the others bit for bit)."""
    r = slice(ref.n_pad, None)
    if not bool((got_v[:, r] == ref.v[:, r]).all()):
        return Verdict(False, float("inf"), 0.0, f"{what}: a written V row differs from the row's v")
    worst = 0.0
    for got, want, ab, name, names in ((got_q[r], ref.q[r], ref.q_ab[r], "q", ("row", "head", "dim")),
                                       (got_k[:, r], ref.k[:, r], ref.k_ab[:, r], "K row", ("kv head", "row", "dim"))):
        bound = torch.zeros_like(ab) if dt == "bf16" else C_K * U32 * ab
        v = _bounded(got, want, bound, f"{what} {name}", names)
        if not v:
            return v
        worst = max(worst, v.ratio)
    return Verdict(True, worst, 1.0, "")


def norm_float32_model(x, qw, kw, n_kv, n_pad, rope_delta, dt, rope_len=ROPE_LEN, eps=EPS):
    f32 = torch.float32
    T = (lambda v: v.to(torch.bfloat16).to(f32)) if dt == "bf16" else (lambda v: v)
    L, per, _ = x.shape
    NH = per - 2 * n_kv
    ct, st = rope_table(rope_len)
    pos = (torch.arange(L) + rope_delta).clamp(0, rope_len - 1)
    cs, sn = ct[pos][:, None].to(f32), st[pos][:, None].to(f32)

    def nr(xx, w):
        xx, w = xx.to(f32), w.to(f32)
        rs = 1.0 / torch.sqrt((xx * xx).sum(dim=-1, keepdim=True) / HD + torch.tensor(eps, dtype=f32))
        n = T(w * T(xx * rs))
        n0, n1 = n[..., :64], n[..., 64:]
        return torch.cat([T(T(n0 * cs) + T(-n1 * sn)), T(T(n1 * cs) + T(n0 * sn))], dim=-1).to(F64)

    return nr(x[:, :NH], qw), nr(x[:, NH:NH + n_kv], kw).transpose(0, 1), x[:, NH + n_kv:].transpose(0, 1)


# ---- windowed attention and rope_rows --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def win_input(dt, kind, hd, n_batch, Tn, seed=0):
    """qkv [n_batch][Tn][3][W_NH][hd]; "which": V row j = (1 + j // hd) * unit(j % hd), K small (scores within a unit)."""
    gen = torch.Generator().manual_seed(((88_000 + seed) * 131 + hd) * 131 + Tn * 7 + n_batch + (kind == "which") * 3 + (dt == "bf16"))
    x = rnd(torch.randn(n_batch, Tn, 3, W_NH, hd, generator=gen, dtype=F64), dt)
    if kind == "which":
        x[:, :, 1] = rnd(x[:, :, 1] * 0.05, dt)
        j = torch.arange(Tn)
        V = torch.zeros(Tn, hd, dtype=F64)
        V[j, j % hd] = (1 + j // hd).to(F64)
        x[:, :, 2] = V[None, :, None, :]
    return x


@dataclass
class WinRef:
    out: torch.Tensor            # [n_batch][Tn][NH][hd]
    A: torch.Tensor
    Bmax: torch.Tensor           # [n_batch][Tn][NH]
    nk: torch.Tensor             # [Tn]


def win_reference(x, window, scale, *, mutant="") -> WinRef:
    """mutant "window_plus": one key more (q - window); "window_minus": one key fewer."""
    nb, Tn, _, NH, hd = x.shape
    t = torch.arange(Tn)
    w = window + (1 if mutant == "window_plus" else (-1 if mutant == "window_minus" else 0))
    lo = (t - w + 1).clamp_min(0)
    mask = (t[None, :] <= t[:, None]) & (t[None, :] >= lo[:, None])
    out = torch.zeros(nb, Tn, NH, hd, dtype=F64)
    Aa = torch.zeros_like(out)
    Bmax = torch.zeros(nb, Tn, NH, dtype=F64)
    for b in range(nb):
        for h in range(NH):
            q, k, v = x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h]
            s = torch.where(mask, scale * q @ k.t(), torch.full((Tn, Tn), -float("inf"), dtype=F64))
            B = scale * q.abs() @ k.abs().t()
            p = torch.exp(s - s.max(dim=1, keepdim=True).values)
            l = p.sum(dim=1, keepdim=True)
            out[b, :, h], Aa[b, :, h] = (p @ v) / l, (p @ v.abs()) / l
            Bmax[b, :, h] = torch.where(mask, B, torch.zeros_like(B)).max(dim=1).values
    return WinRef(out, Aa, Bmax, (t - (t - window + 1).clamp_min(0) + 1))


def check_win(got, ref: WinRef, dt, row_lo, exp_rel, what="") -> Verdict:
    """got [n_batch][Tn][NH][hd] as stored; rows >= row_lo are looked at."""
    hd = got.shape[-1]
    r = slice(row_lo, None)
    if bool(torch.isnan(got[:, r]).any()):
        return Verdict(False, float("inf"), 0.0, f"{what}: NaN in the output")
    E = 2.0 * (hd + 6.0) * U32 * ref.Bmax[:, r] + gamma_win(ref.nk[r], exp_rel)[None, :, None]
    out = ref.out[:, r]
    bound = E[..., None] * ref.A[:, r]
    bound = bound + 0.5 * ulp(out.abs() + bound, dt)
    bf = dt == "bf16"
    return _bounded(got[:, r], out, bound, what, ("batch", "row", "head", "dim"), rnd(out, dt) if bf else None, F_EXACT if bf else 0.0)


def win_float32_model(x, window, scale, dt):
    f32 = torch.float32
    nb, Tn, _, NH, hd = x.shape
    t = torch.arange(Tn)
    mask = (t[None, :] <= t[:, None]) & (t[None, :] >= (t - window + 1).clamp_min(0)[:, None])
    out = torch.zeros(nb, Tn, NH, hd, dtype=f32)
    xf = x.to(f32)
    for b in range(nb):
        for h in range(NH):
            s = (xf[b, :, 0, h] @ xf[b, :, 1, h].t()) * torch.tensor(scale, dtype=f32)
            s = torch.where(mask, s, torch.full_like(s, -1e30))
            p = torch.where(mask, torch.exp(s - s.max(dim=1, keepdim=True).values), torch.zeros_like(s))
            out[b, :, h] = (p @ xf[b, :, 2, h]) / p.sum(dim=1, keepdim=True)
    return (out.to(torch.bfloat16).to(f32) if dt == "bf16" else out).to(F64)


@functools.lru_cache(maxsize=None)
def win_rope_table(Tn, hd):
    """cos / sin [Tn][hd / 2] fp32 values of seeded random angles (every sign combination occurs)."""
    gen = torch.Generator().manual_seed(12_000 + Tn * 3 + hd)
    th = torch.rand(Tn, hd // 2, generator=gen, dtype=F64) * (2.0 * math.pi)
    return rnd(torch.cos(th), "f32"), rnd(torch.sin(th), "f32")


def rope_rows_reference(x, cos, sin, dt, *, mutant=""):
    """x [n_batch][Tn][3][NH][hd] -> (the q and k thirds rotated [n_batch][Tn][2][NH][hd], |a| + |b|).  mutant "interleaved": pairs
    (2j, 2j + 1) instead of rotate_half's (j, j + hd / 2)."""
    R = lambda v: rnd(v, dt)
    half = x.shape[-1] // 2
    qk = x[:, :, :2]
    cs, sn = cos[None, :, None, None, :], sin[None, :, None, None, :]
    if mutant == "interleaved":
        x0, x1 = qk[..., 0::2], qk[..., 1::2]
    else:
        x0, x1 = qk[..., :half], qk[..., half:]
    a0, b0, a1, b1 = R(x0 * cs), R(-x1 * sn), R(x1 * cs), R(x0 * sn)
    o0, o1 = R(a0 + b0), R(a1 + b1)
    ab0, ab1 = a0.abs() + b0.abs(), a1.abs() + b1.abs()
    if mutant == "interleaved":
        return torch.stack([o0, o1], dim=-1).flatten(-2), torch.stack([ab0, ab1], dim=-1).flatten(-2)
    return torch.cat([o0, o1], dim=-1), torch.cat([ab0, ab1], dim=-1)


def check_rope_rows(got, want, ab, dt, row_lo, what="") -> Verdict:
    r = slice(row_lo, None)
    bound = torch.zeros_like(ab[:, r]) if dt == "bf16" else C_ROPE * U32 * ab[:, r]
    return _bounded(got[:, r], want[:, r], bound, what, ("batch", "row", "q|k", "head", "dim"))


def rope_rows_float32_model(x, cos, sin, dt):
    f32 = torch.float32
    T = (lambda v: v.to(torch.bfloat16).to(f32)) if dt == "bf16" else (lambda v: v)
    half = x.shape[-1] // 2
    qk = x[:, :, :2].to(f32)
    cs, sn = cos.to(f32)[None, :, None, None, :], sin.to(f32)[None, :, None, None, :]
    x0, x1 = qk[..., :half], qk[..., half:]
    return torch.cat([T(T(x0 * cs) + T(-x1 * sn)), T(T(x1 * cs) + T(x0 * sn))], dim=-1).to(F64)
