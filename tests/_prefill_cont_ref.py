"""Float64 reference of the continuation prefill kernels (csrc/prefill_kernels.cuh: qk_norm_rope_kv_cont_kernel,
prefill_attn_cont_kernel, flash_prefill_cont_kernel + flash_cont_merge_kernel) and their checkers.

The reference of a continuation is the rows >= start of the WHOLE-sequence reference of tests/_prefill_attn_ref.py (``attn_reference``,
``norm_reference``; imported, not restated): new row t of a continuation at ``start`` is row start + t of the prompt of start + n rows,
without left padding.  Written from the documented contract (the header comment of fq3_prefill_continue, the comments above the kernels):

* norm + RoPE + K/V write: local row t is normalised and rotated at RoPE row clamp(start + t + rope_delta, 0, rope_len - 1); q in place at
  local row t; K / V to cache row start + t; every other cache row (below start, beyond start + n) is untouched.  The checks of
  ``_prefill_attn_ref.check_norm`` apply to the n rows (bf16 bit-exact on the tie-free rows, fp32 within C_K u (|a| + |b|), v bit-exact).
* wave kernel with a query base: per row "the same loop over keys 0 .. start + t" -- the bound of prefill_attn_kernel, ``gamma_wave`` of the
  row's start + t + 1 keys.
* flash kernel with key splits: the key tiles [0, nt) of a query block are cut into S contiguous ranges; inside a range the arithmetic is
  flash_tile's, so over all ranges a row passes one online-softmax step per tile it has live keys in, as in the whole prefill
  (``gamma_flash``: the tiles, the normalisation, the 3 n u of the sums, the 2^-16 of the two bf16 parts of P).  The merge adds one
  online-softmax step per split -- one exponential 2^(m_s - M) and two roundings (product + fma), for numerator and denominator:
  ``gamma_cont = gamma_flash + 2 S (EXP2_REL + 2 u)`` for S > 1, gamma_flash itself for S == 1 (no merge launch).  The bf16 exact-fraction
  floor is ``flash_floor(ref, rows=slice(start, None))``, derived from the whole-prefill E as that function documents.
* the split count is the launcher's rule (``flash_cont_splits``), mirrored by :func:`splits`: S = min(n_cu // (blocks * heads),
  key tiles // 4, 16), at least 1 (and the records must fit the workspace).

The case list of the GPU module lives here so that the CPU self-test (tests/test_prefill_cont_reference_cpu.py) runs the checkers on
exactly those cases.  No constant is tuned to an observed value."""
from __future__ import annotations

import functools

import torch

import _attn_ref as A
import _prefill_attn_ref as P
from _attn_ref import F_EXACT, U32, Verdict, _bounded
from _gemm_ref import F64, rnd, ulp
from _prefill_attn_ref import EPS, EXP2_REL, HD, KS, N_KV, SCALE

REP = 2                               # head ratio 2: the shipped talker configs
NH = N_KV * REP
N_CU = 256                            # the MI355X; the GPU module passes the device's own count to the probe and to splits()
MIN_TILES, MAX_SPLIT, REC = 4, 16, 2 + HD
WS_FLOATS = 1 << 20
ROPE_LEN = 560
ROPE_DELTAS = (0, -7, 40)             # case i takes ROPE_DELTAS[i % 3]: start + t + delta below 0 (start 0) and beyond rope_len - 1 (start 448)
KINDS = P.KINDS

STARTS = [0, 1, 63, 64, 65, 130, 200, 448]
NS = [1, 16, 17, 63, 64, 65, 130]
BASE_CASES = [(s, n) for s in STARTS for n in NS]
# longer starts, up to about 1100 keys, for the split counts: with NH = 4 the rule gives S = key tiles // 4 here --
# (448, 130) above: 10 tiles, S = 2; (704, 64): 12 tiles, S = 3, whole ranges of 4; (760, 17): 13 tiles, S = 3, ranges of 5, the last one
# ragged (3 tiles); (1000, 100): 18 tiles, S = 4, two query blocks (17 and 18 tiles), ragged; (1090, 130): 20 tiles, S = 5, three blocks
LONG_CASES = [(704, 64), (760, 17), (1000, 100), (1090, 130)]
CASES = BASE_CASES + LONG_CASES
# split counts the launcher would not choose for the size, given to the kernel by hand: a split without a tile ((200, 17): 4 tiles cut
# in 5), one tile per split ((64, 65): 3 tiles in 3), and S = 1 at a size where the launcher splits
FORCED = [(200, 17, 5), (64, 65, 3), (760, 17, 1)]
L_BIG = 1280


def splits(start, n, nh=NH, n_cu=N_CU, ws_floats=WS_FLOATS):
    nqb, nt = (n + KS - 1) // KS, (start + n + KS - 1) // KS
    S = min(n_cu // (nqb * nh), nt // MIN_TILES, MAX_SPLIT)
    while S > 1 and S * n * nh * REC > ws_floats:
        S -= 1
    return max(S, 1)


def split_ranges(start, n, S):
    """Per query block: the tile ranges [lo, hi) of its S splits (hi <= lo: a split without a tile)."""
    out = []
    for q0 in range(0, n, KS):
        nt = (start + min(q0 + KS, n) - 1) // KS + 1
        tps = (nt + S - 1) // S
        out.append([(z * tps, min(nt, z * tps + tps)) for z in range(S)])
    return out


# ---- operands ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_q(dt):
    gen = torch.Generator().manual_seed(77_000)
    return rnd(torch.randn(L_BIG, NH, HD, generator=gen, dtype=F64), dt)


def operands(dt, kind, start, n):
    """q [L][NH][128], K / V [n_kv][L][128] of the whole prompt of L = start + n rows (T values as float64)."""
    L = start + n
    K, V = A.base_cache(dt, kind, N_KV, L_BIG, 0)
    return base_q(dt)[:L], K[:, :L], V[:, :L]


def case_reference(dt, kind, start, n, *, mutant=""):
    """The whole-sequence reference (rows >= start are the continuation's).  Deliberate defects: causal_minus / causal_plus (the bound
    off by one), drop_past (keys below start dropped), tile_local (the key tile looked up by its index counted from the first new
    tile), v_tile_swap (the V rows of the first past tile in reverse order)."""
    q, K, V = operands(dt, kind, start, n)
    L = start + n
    if mutant in ("causal_minus", "causal_plus"):
        return P.attn_reference(q, K, V, 0, mutant=mutant)
    if mutant == "drop_past":
        return P.attn_reference(q, K, V, start)
    if mutant == "tile_local":
        j = torch.arange(L)
        idx = ((j // KS - start // KS) % ((L + KS - 1) // KS)) * KS + j % KS
        idx = idx.clamp_max(L - 1)
        return P.attn_reference(q, K[:, idx], V[:, idx], 0)
    if mutant == "v_tile_swap":
        V = V.clone()
        m = min(KS, start)
        V[:, :m] = V[:, :m].flip(1)
        return P.attn_reference(q, K, V, 0)
    assert mutant == ""
    return P.attn_reference(q, K, V, 0)


def mutant_applies(mutant, start, n, delta=0):
    """False where the defect cannot change a new row's output (rope_local: where the clamp gives both positions the same RoPE row)."""
    clamp = lambda p: min(max(p, 0), ROPE_LEN - 1)
    return {"causal_minus": True, "causal_plus": n >= 2, "drop_past": start >= 1, "tile_local": start >= KS, "v_tile_swap": start >= 2,
            "rope_local": any(clamp(start + t + delta) != clamp(t + delta) for t in range(n)), "kv_local_row": start >= 1}[mutant]


# ---- attention checkers --------------------------------------------------------------------------------------------------------------
def attn_e_cont(ref, kernel, S):
    e = P.attn_e(ref, "wave" if kernel == "wave" else "flash")
    if kernel == "flash" and S > 1:
        e = e + 2.0 * S * (EXP2_REL + 2.0 * U32)
    return e


def check_attn_cont(got, ref, start, dt, kernel, S=1, what="") -> Verdict:
    """got [n][NH][128] float64 as stored in T: the output rows of the new rows."""
    rows = slice(start, None)
    if bool(torch.isnan(got).any()):
        return Verdict(False, float("inf"), 0.0, f"{what}: NaN in the output")
    out = ref.out[rows]
    bound = attn_e_cont(ref, kernel, S)[rows, :, None] * ref.A[rows]
    bound = bound + 0.5 * ulp(out.abs() + bound, dt)
    f = 0.0 if dt != "bf16" else (F_EXACT if kernel == "wave" else P.flash_floor(ref, rows=rows))
    return _bounded(got, out, bound, what, ("row", "head", "dim"), rnd(out, dt) if dt == "bf16" else None, f)


def attn_model(dt, kind, start, n, *, mutant=""):
    """What a kernel would store: plain float32 arithmetic for the unmutated model; a defect is the float64 reference WITH the defect,
    rounded to T (its error is the defect alone)."""
    if mutant == "":
        q, K, V = operands(dt, kind, start, n)
        return P.attn_float32_model(q, K, V, 0, dt)[start:]
    return rnd(case_reference(dt, kind, start, n, mutant=mutant).out[start:], dt)


# ---- norm + RoPE + K/V write -----------------------------------------------------------------------------------------------------------
def norm_input(dt, L):
    """[L][NH + 2 N_KV][128]: the rows of the whole prompt before the norm (the shared tie-free pool of _prefill_attn_ref, cyclic)."""
    x, _ = P.norm_rows(dt, P.N_NORM_ROWS)
    idx = torch.arange(L) % P.N_NORM_ROWS
    return torch.cat([x[idx, :NH], x[idx, P.NH_MAX:]], dim=1)


def norm_reference(dt, start, n, delta):
    qw, kw = A.base_gains(dt, "random")
    return P.norm_reference(norm_input(dt, start + n), qw, kw, N_KV, 0, delta, dt, rope_len=ROPE_LEN)


def _same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def check_norm_cont(got_q, k_after, v_after, k_before, v_before, ref, start, n, dt, what="") -> Verdict:
    """got_q [n][NH][128] (the q third of the new rows after the launch); k / v: the LOGICAL cache rows [n_kv][rows][128] before and after
    (NaN = a sentinel).  Rows outside [start, start + n) must be what they were; the n rows are held to check_norm."""
    keep = torch.ones(k_after.shape[1], dtype=torch.bool)
    keep[start:start + n] = False
    if not (_same(k_after[:, keep], k_before[:, keep]) and _same(v_after[:, keep], v_before[:, keep])):
        return Verdict(False, float("inf"), 0.0, f"{what}: a cache row outside [start, start + n) changed")
    r = slice(start, start + n)
    if bool(torch.isnan(k_after[:, r]).any() or torch.isnan(v_after[:, r]).any() or torch.isnan(got_q).any()):
        return Verdict(False, float("inf"), 0.0, f"{what}: a row of the new rows was not written")
    new = P.NormRef(ref.q[r], ref.q_ab[r], ref.k[:, r], ref.k_ab[:, r], ref.v[:, r], 0)
    return P.check_norm(got_q, k_after[:, r], v_after[:, r], new, dt, what=what)


def norm_model(dt, start, n, delta, rows, *, mutant=""):
    """(q of the new rows, K, V logical cache rows [n_kv][rows][128] after the launch, K, V before) of a float32 model of the kernel on a
    cache of `rows` rows that held NaN sentinels.  Defects: rope_local (the RoPE position without start), kv_local_row (K / V written at
    the local row)."""
    qw, kw = A.base_gains(dt, "random")
    x = norm_input(dt, start + n)
    if mutant == "rope_local":
        q, k, v = P.norm_float32_model(x[start:], qw, kw, N_KV, 0, delta, dt, rope_len=ROPE_LEN)
    else:
        q, k, v = P.norm_float32_model(x, qw, kw, N_KV, 0, delta, dt, rope_len=ROPE_LEN)
        q, k, v = q[start:], k[:, start:], v[:, start:]
    before = torch.full((N_KV, rows, HD), float("nan"), dtype=F64)
    ka, va = before.clone(), before.clone()
    at = 0 if mutant == "kv_local_row" else start
    ka[:, at:at + n], va[:, at:at + n] = k, v
    return q, ka, va, before, before.clone()
