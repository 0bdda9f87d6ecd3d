"""The packs of the packed continuation prefill kernels (csrc/prefill_kernels.cuh: qk_norm_rope_kv_cont_pack_kernel,
flash_prefill_cont_pack_kernel + flash_cont_pack_merge_kernel), a mirror of the launcher's split rule, and the pack builders.

A pack is n sequences, sequence q with cnt[q] NEW rows behind start[q] cached rows; per sequence the contract is that of the
single-sequence kernels, so the float64 references and the checkers are those of tests/_prefill_cont_ref.py (``case_reference``,
``check_attn_cont``, ``check_norm_cont``, ``splits``; imported, not restated) applied to each sequence's own (start, n).  The attention
bound stays ``gamma_flash`` plus one online-softmax step per merged split of THAT sequence.

* split rule (``flash_cont_pack_splits``), mirrored by :func:`pack_splits`: budget = n_cu // (total query blocks of the pack * heads);
  S[q] = min(budget, key tiles of q // 4, 16), at least 1; while the records of the pack (S[q] * cnt[q] * heads * REC floats for every
  S[q] > 1) exceed the workspace, the largest S -- the first of equals -- loses one.  For a pack of one that is ``splits(start, n)``.
* one pool, shuffled and INTERLEAVED block ids (:func:`pack_tables`): tile t of sequence q takes the next id of a shuffled permutation
  in (t, q) order, so neighbouring ids belong to different sequences and a table mix-up lands on another sequence's rows.
* so that another sequence's rows are WRONG rows even where two sequences hold the same positions of the shared operand pool, sequence
  q's V rows are multiplied by :func:`v_scale` (a signed power of two: exact in both storage types, and the kernel's products and sums
  scale with it exactly); the test divides the output by it before the unchanged checker sees it.  Operand kinds alternate too.

The pack list lives here so that the CPU self-test (tests/test_prefill_pack_cont_cpu.py) checks the rule on exactly those packs.  No
constant is tuned to an observed value."""
from __future__ import annotations

import torch

from _prefill_cont_ref import (CASES, KINDS, MAX_SPLIT, MIN_TILES, N_CU, N_KV, NH, REC, REP, ROPE_DELTAS, WS_FLOATS, case_reference,  # noqa: F401
                               check_attn_cont, check_norm_cont, splits)
from _prefill_attn_ref import KS

MAX_PACK = 64

PACK_A = [(0, 1), (63, 17), (64, 64), (130, 65), (1, 16)]
PACK_B = [(200, 17)]
PACK_C = [((0, 1, 63, 64, 65)[i % 5], (1, 16, 17)[i % 3]) for i in range(MAX_PACK)]      # 5 and 3 are coprime: all 15 pairs occur
PACK_D = [(704, 64), (1000, 100), (0, 130)]
PACKS = {"A": PACK_A, "B": PACK_B, "C": PACK_C, "D": PACK_D}
FORCED_D = (1, 3, 5)                     # the same S for every sequence of pack D ((0, 130): 3 tiles cut in 5, splits without a tile)


def tiles_of(start, n):
    return (start + n + KS - 1) // KS


def pack_ws_floats(cnts, S, nh=NH):
    return sum(s * c * nh * REC for s, c in zip(S, cnts) if s > 1)


def pack_splits(starts, cnts, nh=NH, n_cu=N_CU, ws_floats=WS_FLOATS):
    nqb = sum((c + KS - 1) // KS for c in cnts)
    budget = n_cu // (nqb * nh)
    S = [max(1, min(budget, tiles_of(s, c) // MIN_TILES, MAX_SPLIT)) for s, c in zip(starts, cnts)]
    while pack_ws_floats(cnts, S, nh) > ws_floats:
        S[S.index(max(S))] -= 1
    return S


def pack_offsets(cnts):
    off = [0]
    for c in cnts:
        off.append(off[-1] + c)
    return off


def pack_tables(pack, spare=3, seed=0):
    """(n_blocks, [table of sequence q]): one pool of all the pack's tiles + ``spare`` unowned blocks; ids shuffled and interleaved."""
    tiles = [tiles_of(s, n) for s, n in pack]
    n_blocks = sum(tiles) + spare
    perm = torch.randperm(n_blocks, generator=torch.Generator().manual_seed(9100 + seed)).tolist()
    tables = [[0] * t for t in tiles]
    k = 0
    for t in range(max(tiles)):
        for q in range(len(pack)):
            if t < tiles[q]:
                tables[q][t] = perm[k]
                k += 1
    return n_blocks, tables


def v_scale(q):
    """The factor of sequence q's V rows: a signed power of two, 14 different ones."""
    return (-1.0 if (q // 7) % 2 else 1.0) * 2.0 ** (q % 7 - 3)


def kind_of(q):
    return KINDS[q % len(KINDS)]
