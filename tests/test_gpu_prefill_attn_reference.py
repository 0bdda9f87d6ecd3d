"""Conformance of every prefill and windowed attention kernel with the float64 reference of tests/_prefill_attn_ref.py.

Each case is launched alone through tools/microbench/libprefill_attn_probe.so.  Paged kinds: the pool is larger than needed, every
sequence reads a shuffled block table (the tables of a pack are disjoint), every unowned block, every qkv / output row the kernel must
not touch and the k | v thirds of the attention kinds' qkv hold a NaN sentinel bit pattern, and there are guard rows behind every
buffer; all of it is compared bit for bit afterwards.  The dead rows of OWNED blocks (rows below n_pad, rows beyond L in the last
tile) hold +/- 2^60 for the flash kinds -- finite, per the contract stated in csrc/prefill_kernels.cuh -- and the NaN sentinel for
prefill_attn_kernel, which must tolerate them.  Two operand sets per case: random, and the "which key" set of the decode suite (V row
j = (1 + j // 128) * unit vector j % 128 under nearly equal scores: output dim d is the probability of key d, so a dropped, doubled
or misplaced key moves one element by its whole value).  flash_prefill_small_kernel is compared bit for bit with
flash_prefill_kernel<4,false> on the same sequence, as its comment promises; the paired and the 128-query shapes are held to the
bound, and whether they came out bit-identical to <4,false> is reported only (no comment promises it).

The last test prints, per kernel and type, the cases run, the largest err / bound and the smallest bf16 exact fraction, and asserts that
every listed instantiation was reached.  Observed on the MI355X (a record: no bound or floor is tuned to it; a value stored in bf16 sits
up to half an ulp from the float64 reference, so the bf16 err / bound figures approach 1 by construction -- the fp32 figures and the
bf16 exact fraction carry the information):
  kernel                          fp32: cases, largest err / bound    bf16: cases, largest err / bound, smallest exact fraction
  qk_norm_rope_kv_kernel          186, 0.30 of C_K                    186, bit-exact (q, K rows and V rows)
  qk_norm_rope_kv_pack_kernel     369, 0.30 of C_K                    369, bit-exact
  prefill_attn_kernel             324, 0.0017                         324, 0.97, 0.99974
  flash_prefill_kernel<4,false>   -                                   324, 0.994, 0.99744
  flash_prefill_kernel<4,true>    -                                   48, 0.993, 0.99757 (bit-identical to <4,false> in 48 of 48 cases)
  flash_prefill_kernel<8,true>    -                                   48, 0.993, 0.99772 (bit-identical to <4,false> in 48 of 48 cases)
  flash_prefill_small_kernel      -                                   666 sequences, 0.994, 0.99744 (bit-identical to <4,false>: asserted)
  swa_attn_kernel                 1176, 0.022                         1176, 0.995, 0.99609 (one element of 256)
  win_attn_kernel                 840, 0.042                          -
  rope_rows_kernel                24, 0.5 of C_ROPE (a fused product) 24, bit-exact
  The flash kernels' derived exact-fraction floors are 0.33 .. 0.94 on the random operands and 0.98 .. 0.99 on the "which key" ones
  (tests/_prefill_attn_ref.py); every flash case came out at 0.997 or above, the level of the wave kernel's F_EXACT = 0.99.
  exp2f on [-90, 0]: largest relative error 8.14e-8 at x = -61.94; expf: 7.805e-8 at x = -46.40 (1.22e-45 absolute below 2^-126).
No case found a defect: no NaN, no touched sentinel, no element outside its bound.  The finite-dead-rows contract of the flash kernels
is now written above the flash kernels (csrc/prefill_kernels.cuh) and exercised by the +/- 2^60 rows of every flash case.
"""
import ctypes as C
import math
import os
from collections import defaultdict

import pytest
import torch

import _attn_ref as A
import _prefill_attn_ref as P
from _prefill_attn_ref import HD, KS, N_KV
from test_gpu_attn_reference import ibits, is_sentinel, sentinel, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libprefill_attn_probe.so")
F64 = torch.float64
K_NORM_KV, K_NORM_KV_PACK, K_WAVE, K_FLASH, K_FLASH_SMALL, K_SWA, K_WIN, K_ROPE_ROWS = range(8)
TE = {"bf16": 0, "f32": 2}
ESZ = {"bf16": 2, "f32": 4}
vp, i32, f32c = C.c_void_p, C.c_int32, C.c_float
pint = C.POINTER(C.c_int)
DTS = ("f32", "bf16")
GUARD_ROWS = 2


class PrefillProbeArgs(C.Structure):
    _fields_ = [("NH", i32), ("NKV", i32), ("n_seq", i32), ("qkv_rows", i32), ("rope_len", i32), ("n_blocks", i32), ("n_table", i32),
                ("nw", i32), ("paired", i32), ("hd", i32), ("np", i32), ("Tn", i32), ("window", i32), ("row_lo", i32), ("n_batch", i32),
                ("eps", f32c), ("scale", f32c), ("qkv", vp), ("q_norm_w", vp), ("k_norm_w", vp), ("cos_tab", vp), ("sin_tab", vp),
                ("kpool", vp), ("vpool", vp), ("out", vp), ("table", pint), ("seq_len", pint), ("seq_n_pad", pint), ("seq_rope_delta", pint)]


STATS = defaultdict(lambda: {"cases": 0, "ratio": 0.0, "min_exact": 1.0, "min_margin": 1.0})       # per kernel and storage type
REACHED = set()                                                                                  # instantiations launched
IDENTICAL = defaultdict(lambda: [0, 0])                                                          # shape -> [bit-identical to <4,false>, cases]


def record(kernel, dt, v, inst=(), floor=None):
    st = STATS[(kernel, dt)]
    st["cases"] += 1
    st["ratio"] = max(st["ratio"], v.ratio)
    st["min_exact"] = min(st["min_exact"], v.exact)
    if floor is not None:
        st["min_margin"] = min(st["min_margin"], v.exact - floor)
    REACHED.add((kernel, dt) + tuple(inst))


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libprefill_attn_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.prefill_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(PrefillProbeArgs), vp]
    lib.prefill_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(PrefillProbeArgs)]
    lib.prefill_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.prefill_probe_exp.argtypes = [C.c_int, vp, vp, C.c_int, vp]
    assert lib.prefill_probe_version() == 1 and lib.prefill_probe_kinds() == 8
    buf = (C.c_long * 64)()
    n = lib.prefill_probe_layout(buf, 64)
    want = [C.sizeof(PrefillProbeArgs)] + [getattr(PrefillProbeArgs, f[0]).offset for f in PrefillProbeArgs._fields_]
    assert list(buf[:n - 4]) == want, "ctypes mirror of PrefillProbeArgs is out of date"
    assert list(buf[n - 3:n - 1]) == [64, 256]
    return lib


def launch(probe, kind, dt, p, what):
    assert probe.prefill_probe_admits(kind, TE[dt], C.byref(p)) == 1, f"{what}: the probe refuses kind {kind}"
    rc = probe.prefill_probe_run(kind, TE[dt], C.byref(p), None)
    assert rc == 0, f"{what}: kind {kind} returned {rc}"


def unchanged(t, t0, what):
    diff = ibits(t) != t0
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} elements changed, first at {tuple(int(v) for v in torch.nonzero(diff)[0])}"


# ---- device image of the paged kinds ---------------------------------------------------------------------------------------------
class Paged:
    """One or several sequences in one pool.  mode "finite" / "nan": attention (q rows given, the caches filled, dead rows of owned
    blocks +/- 2^60 or NaN); mode "norm": rows before the norm (rows below each n_pad NaN), the pool all NaN."""

    def __init__(self, dt, rep, seqs, mode, *, deltas=None, table_seed=0, kind="random"):
        self.dt, self.rep, self.mode, self.NH = dt, rep, mode, N_KV * rep
        self.per = self.NH + 2 * N_KV
        self.L = [s[0] for s in seqs]
        self.n_pad = [s[1] for s in seqs]
        self.deltas = list(deltas) if deltas is not None else [0] * len(seqs)
        self.off = [0]
        for L in self.L:
            self.off.append(self.off[-1] + L)
        self.rows = self.off[-1]
        tiles = [(L + KS - 1) // KS for L in self.L]
        self.n_table = max(tiles)
        self.n_blocks = sum(tiles) + 3
        g = torch.Generator().manual_seed(4000 + 31 * table_seed + self.rows)
        perm = torch.randperm(self.n_blocks, generator=g).tolist()
        while any(perm[i] == i for i in range(sum(tiles))):     # no owned tile in the block the identity table would name
            perm = torch.randperm(self.n_blocks, generator=g).tolist()
        spare = perm[sum(tiles)]                                 # an unowned block (NaN): what a table entry past a sequence's tiles names
        self.tables, at = [], 0
        for n in tiles:
            self.tables.append(perm[at:at + n] + [spare] * (self.n_table - n))
            at += n
        pools = [torch.full((self.n_blocks, N_KV, KS, HD), float("nan"), dtype=F64) for _ in range(2)]
        qkv = torch.full((self.rows + GUARD_ROWS, self.per, HD), float("nan"), dtype=F64)
        self.seqs = []
        if mode == "norm":
            for q, (L, n_pad) in enumerate(zip(self.L, self.n_pad)):
                x = P.norm_input(dt, rep, L, start=self.off[q]).clone()
                self.seqs.append(x.clone())
                x[:n_pad] = float("nan")
                qkv[self.off[q]:self.off[q + 1]] = x
        else:
            for q, (L, n_pad) in enumerate(zip(self.L, self.n_pad)):
                s = P.Seq(dt, kind, N_KV, rep, L, n_pad, q % 4 if len(seqs) > 1 else 0)
                self.seqs.append(s)
                qkv[self.off[q]:self.off[q + 1], :self.NH] = s.q
                for pool, X in zip(pools, s.dead_rows(finite=(mode == "finite"))):
                    for t in range(tiles[q]):
                        pool[self.tables[q][t]] = X[:, t * KS:(t + 1) * KS]
        self.K, self.V, self.qkv = to_dev(pools[0], dt), to_dev(pools[1], dt), to_dev(qkv, dt)
        self.K0, self.V0, self.qkv0 = ibits(self.K).clone(), ibits(self.V).clone(), ibits(self.qkv).clone()
        self.fresh_out()
        flat = [e for t in self.tables for e in t]
        self.c_table = (C.c_int * len(flat))(*flat)
        self.c_len, self.c_pad, self.c_delta = ((C.c_int * len(seqs))(*v) for v in (self.L, self.n_pad, self.deltas))
        if mode == "norm":
            qw, kw = A.base_gains(dt, "random")
            self.qw64, self.kw64 = qw, kw
            self.qw, self.kw = to_dev(qw, dt), to_dev(kw, dt)
            ct, st = P.rope_table()
            self.cos, self.sin = ct.to(torch.float32).cuda(), st.to(torch.float32).cuda()

    def fresh_out(self):
        self.out = sentinel((self.rows + GUARD_ROWS, self.NH, HD), self.dt)

    def args(self, *, first=0, n_seq=None, nw=0, paired=0):
        """The launch of sequences first .. first + n_seq - 1 (all by default); a single-sequence kind starts at packed row off[first]."""
        n_seq = len(self.L) - first if n_seq is None else n_seq
        p = PrefillProbeArgs()
        p.NH, p.NKV, p.n_seq, p.qkv_rows = self.NH, N_KV, n_seq, self.off[first + n_seq] - self.off[first]
        p.rope_len, p.n_blocks, p.n_table, p.nw, p.paired = P.ROPE_LEN, self.n_blocks, self.n_table, nw, paired
        p.eps, p.scale = P.EPS, P.SCALE
        p.qkv = self.qkv.data_ptr() + self.off[first] * self.per * HD * ESZ[self.dt]
        p.out = self.out.data_ptr() + self.off[first] * self.NH * HD * ESZ[self.dt]
        p.kpool, p.vpool = self.K.data_ptr(), self.V.data_ptr()
        if self.mode == "norm":
            p.q_norm_w, p.k_norm_w, p.cos_tab, p.sin_tab = self.qw.data_ptr(), self.kw.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr()
        off = lambda arr, n: C.cast(C.byref(arr, 4 * n), pint)
        p.table, p.seq_len, p.seq_n_pad, p.seq_rope_delta = (off(self.c_table, first * self.n_table), off(self.c_len, first),
                                                             off(self.c_pad, first), off(self.c_delta, first))
        return p

    def read_attn(self, what, only=None):
        """The attention output [rows][NH][128] float64 after a launch that must have left the inputs alone; rows the launch did not own
        (guard rows; with only = q: every other sequence's) keep the sentinel."""
        unchanged(self.K, self.K0, what + " K pool")
        unchanged(self.V, self.V0, what + " V pool")
        unchanged(self.qkv, self.qkv0, what + " qkv")
        o = self.out.cpu()
        lo, hi = (0, self.rows) if only is None else (self.off[only], self.off[only + 1])
        assert is_sentinel(o[:lo], self.dt) and is_sentinel(o[hi:], self.dt), f"{what}: written outside the launch's output rows"
        return o[lo:hi].to(F64)


def check_seq(img, q, got, kernel, name, what, inst=()):
    s = img.seqs[q]
    ref = P.seq_reference(s)
    v = P.check_attn(got, ref, img.dt, kernel, what=what)
    assert v, v.msg
    floor = P.flash_floor(ref) if (kernel == "flash" and s.L > s.n_pad) else None
    record(name, img.dt, v, inst, floor)


# ---- the probe refuses what would leave the buffers (nothing is launched) ---------------------------------------------------------
def test_probe_refuses_out_of_bounds_arguments(probe):
    refused = probe.prefill_probe_refused_code()
    img = Paged("bf16", 2, [(200, 70), (65, 0)], "finite")
    ints = lambda *v: (C.c_int * len(v))(*v)

    def variants():
        base = lambda: img.args(nw=4)
        yield "baseline small", K_FLASH_SMALL, 0, base(), True
        yield "baseline flash", K_FLASH, 0, img.args(n_seq=1, nw=4), True
        yield "flash in fp32", K_FLASH, 2, img.args(n_seq=1, nw=4), False
        yield "flash <8,false>", K_FLASH, 0, img.args(n_seq=1, nw=8, paired=0), False
        yield "flash NW 2", K_FLASH, 0, img.args(n_seq=1, nw=2), False
        yield "two sequences for a single-sequence kind", K_WAVE, 0, base(), False
        for bad in (-1, img.n_blocks):
            tab = ints(*[e for t in img.tables for e in t])
            tab[img.n_table + 1] = bad
            p = base(); p.table = tab
            yield f"table entry {bad} outside the pool", K_FLASH_SMALL, 0, p, False
        p = base(); p.n_table = 3
        yield "fewer table entries than ceil(L / 64)", K_FLASH_SMALL, 0, p, False
        p = base(); p.qkv_rows = 264
        yield "more rows than the buffers hold", K_FLASH_SMALL, 0, p, False
        p = base(); p.seq_len = ints(257, 8)
        yield "a packed sequence of 257 rows", K_FLASH_SMALL, 0, p, False
        p = base(); p.seq_n_pad = ints(200, 0)
        yield "n_pad = L", K_FLASH_SMALL, 0, p, False
        p = base(); p.n_seq = 65
        yield "65 sequences", K_FLASH_SMALL, 0, p, False
        p = base(); p.NH = 5
        yield "NH no multiple of NKV", K_FLASH_SMALL, 0, p, False
        p = base()
        yield "norm kernel without gains and tables", K_NORM_KV_PACK, 0, p, False
        w = PrefillProbeArgs()
        w.NH, w.hd, w.np, w.Tn, w.window, w.row_lo, w.n_batch, w.qkv, w.out = 2, 64, 2, 300, 128, 0, 1, img.qkv.data_ptr(), img.out.data_ptr()
        yield "win baseline", K_WIN, 2, w, True
        yield "win in bf16", K_WIN, 0, w, False
        for name, val, kind in (("window", 129, K_WIN), ("window", 129, K_SWA), ("window", 0, K_SWA), ("row_lo", 300, K_SWA), ("hd", 48, K_SWA),
                                ("np", 5, K_WIN), ("n_batch", 2, K_WIN), ("Tn", 0, K_SWA)):
            w2 = PrefillProbeArgs.from_buffer_copy(w)
            setattr(w2, name, val)
            yield f"windowed {name} {val}", kind, 2, w2, False

    for name, kind, te, p, ok in variants():
        assert probe.prefill_probe_admits(kind, te, C.byref(p)) == int(ok), name
        if not ok:
            assert probe.prefill_probe_run(kind, te, C.byref(p), None) == refused, name
    assert is_sentinel(img.out, "bf16") and torch.equal(ibits(img.K), img.K0) and torch.equal(ibits(img.qkv), img.qkv0)


# ---- the exponentials ----------------------------------------------------------------------------------------------------------------
def test_exp_grids(probe):
    """exp2f and expf on 2^16 + 1 arguments in [-90, 0] (the grid and the exclusion rule of attn_probe_expf) against float64: the measured
    maximum relative errors (over normal results) are what P.EXP2_REL and P.EXPF_REL double."""
    x = torch.linspace(-90.0, 0.0, 65537, dtype=F64).to(torch.float32).cuda()
    for which, name, const, fn in ((0, "exp2f", P.EXP2_REL, torch.exp2), (1, "expf", P.EXPF_REL, torch.exp)):
        y = torch.empty_like(x)
        assert probe.prefill_probe_exp(which, x.data_ptr(), y.data_ptr(), x.numel(), None) == 0
        xe, ye = x.cpu().to(F64), y.cpu().to(F64)
        ref = fn(xe)
        normal = ref >= 2.0 ** -126
        rel = ((ye - ref).abs() / ref)[normal]
        worst = int(torch.argmax(rel))
        flushed = (ye - ref).abs()[~normal]
        fl = float(flushed.max()) if flushed.numel() else 0.0
        print(f"\n{name}: max relative error {float(rel.max()):.4g} at x = {float(xe[normal][worst]):.4f}; below 2^-126: max absolute error {fl:.3g}")
        assert float(ye[-1]) == 1.0, f"{name}(0) must be exactly 1 (a rescale by an unchanged maximum is exact)"
        assert fl <= 2.0 ** -126
        assert 2.0 * float(rel.max()) <= const, f"update the {name} constant in tests/_prefill_attn_ref.py: it must be twice the measured error"


# ---- wave kernel, flash <4,false>, flash small as a pack of one --------------------------------------------------------------------------
@pytest.mark.parametrize("rep", P.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_wave_flash_and_small_every_length_and_pad(probe, dt, rep):
    for kind in P.KINDS:
        for i, (L, n_pad) in enumerate(P.WAVE_CASES):
            what = f"{dt} {kind} rep {rep} L {L} n_pad {n_pad}"
            img = Paged(dt, rep, [(L, n_pad)], "nan", table_seed=i, kind=kind)
            launch(probe, K_WAVE, dt, img.args(), what)
            check_seq(img, 0, img.read_attn(what + " prefill_attn_kernel"), "wave", "prefill_attn_kernel", what + " prefill_attn_kernel")
            if dt != "bf16":
                continue
            img = Paged(dt, rep, [(L, n_pad)], "finite", table_seed=i, kind=kind)
            launch(probe, K_FLASH, dt, img.args(nw=4, paired=0), what)
            check_seq(img, 0, img.read_attn(what + " flash<4,false>"), "flash", "flash_prefill_kernel<4,false>", what + " flash<4,false>")
            if (L, n_pad) in P.SMALL_CASES:
                bits = ibits(img.out).clone()
                img.fresh_out()
                launch(probe, K_FLASH_SMALL, dt, img.args(), what)
                check_seq(img, 0, img.read_attn(what + " flash small"), "flash", "flash_prefill_small_kernel", what + " flash small", ("one",))
                assert torch.equal(ibits(img.out), bits), f"{what}: flash_prefill_small_kernel differs from flash_prefill_kernel<4,false>"


# ---- the paired and the 128-query shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,cases", [(4, P.PAIRED4_CASES), (8, P.PAIRED8_CASES)], ids=["4-paired", "8-paired"])
@pytest.mark.parametrize("rep", P.REPS)
def test_flash_paired_shapes(probe, rep, nw, cases):
    dt = "bf16"
    for kind in P.KINDS:
        for i, (L, n_pad) in enumerate(cases):
            what = f"flash<{nw},true> {kind} rep {rep} L {L} n_pad {n_pad}"
            img = Paged(dt, rep, [(L, n_pad)], "finite", table_seed=i, kind=kind)
            launch(probe, K_FLASH, dt, img.args(nw=nw, paired=1), what)
            check_seq(img, 0, img.read_attn(what), "flash", f"flash_prefill_kernel<{nw},true>", what)
            bits = ibits(img.out).clone()
            img.fresh_out()
            launch(probe, K_FLASH, dt, img.args(nw=4, paired=0), what)
            same = IDENTICAL[f"<{nw},true>"]
            same[0] += int(torch.equal(ibits(img.out), bits))
            same[1] += 1


# ---- packs -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", sorted(P.PACKS))
@pytest.mark.parametrize("rep", P.REPS)
def test_flash_small_packs(probe, rep, pack):
    """One launch for the whole pack; every sequence against its own reference and bit for bit against flash_prefill_kernel<4,false> run on
    that sequence alone (same pool, the sequence's own table)."""
    dt = "bf16"
    seqs = [(L, p) for L, p, _ in P.PACKS[pack]]
    for kind in P.KINDS:
        what = f"flash small {pack} {kind} rep {rep}"
        img = Paged(dt, rep, seqs, "finite", kind=kind)
        launch(probe, K_FLASH_SMALL, dt, img.args(), what)
        got = img.read_attn(what)
        bits = ibits(img.out).clone()
        for q in range(len(seqs)):
            check_seq(img, q, got[img.off[q]:img.off[q + 1]], "flash", "flash_prefill_small_kernel", f"{what} sequence {q} {seqs[q]}", (pack,))
        for q in range(len(seqs)):
            img.fresh_out()
            launch(probe, K_FLASH, dt, img.args(first=q, n_seq=1, nw=4, paired=0), what)
            img.read_attn(f"{what} sequence {q} alone", only=q)
            rows = slice(img.off[q], img.off[q + 1])
            assert torch.equal(ibits(img.out)[rows], bits[rows]), f"{what}: sequence {q} differs from flash_prefill_kernel<4,false> on it alone"


# ---- norm + RoPE + K/V write ---------------------------------------------------------------------------------------------------------------
def check_norm_image(img, what, name, inst=()):
    dt, NH = img.dt, img.NH
    qkv, qkv0 = ibits(img.qkv).clone(), img.qkv0
    written = torch.zeros(img.rows + GUARD_ROWS, dtype=torch.bool)
    for q in range(len(img.L)):
        written[img.off[q] + img.n_pad[q]:img.off[q + 1]] = True
    written = written.cuda()
    assert torch.equal(qkv[~written], qkv0[~written]), f"{what}: a qkv row below n_pad (or a guard row) was touched"
    assert torch.equal(qkv[:, NH:], qkv0[:, NH:]), f"{what}: the k | v part of qkv was written"
    assert is_sentinel(img.out, dt), f"{what}: the attention output was written"
    pools = [img.K.cpu(), img.V.cpu()]
    owned = torch.zeros(img.n_blocks, KS, dtype=torch.bool)
    qd = img.qkv.cpu().to(F64)
    for q, (L, n_pad) in enumerate(zip(img.L, img.n_pad)):
        ref = P.norm_reference(img.seqs[q], img.qw64, img.kw64, N_KV, n_pad, img.deltas[q], dt)
        gk, gv = (P.from_pool(X.to(F64), img.tables[q], L) for X in pools)
        v = P.check_norm(qd[img.off[q]:img.off[q + 1], :NH], gk, gv, ref, dt, what=f"{what} sequence {q}")
        assert v, v.msg
        record(name, dt, v, inst)
        for t in range(n_pad, L):
            owned[img.tables[q][t // KS], t % KS] = True
    for X, nm in zip(pools, "KV"):
        rest = X.permute(0, 2, 1, 3)[~owned]
        assert is_sentinel(rest, dt), f"{what}: the {nm} pool was written outside the rows n_pad .. L - 1 of the sequences' blocks"


@pytest.mark.parametrize("rep", P.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_norm_rope_kv_every_length_pad_and_delta(probe, dt, rep):
    for i, (L, n_pad) in enumerate(P.WAVE_CASES):
        for delta in (P.ROPE_DELTAS if (L, n_pad) in ((1, 0), (17, 1), (321, 65), (321, 0)) else (P.ROPE_DELTAS[i % 3],)):
            what = f"qk_norm_rope_kv_kernel {dt} rep {rep} L {L} n_pad {n_pad} rope_delta {delta}"
            img = Paged(dt, rep, [(L, n_pad)], "norm", deltas=[delta], table_seed=i)
            launch(probe, K_NORM_KV, dt, img.args(), what)
            check_norm_image(img, what, "qk_norm_rope_kv_kernel")
            if delta == P.ROPE_DELTAS[i % 3]:                             # the packed kernel as a pack of one at the same edges
                img = Paged(dt, rep, [(L, n_pad)], "norm", deltas=[delta], table_seed=i)
                launch(probe, K_NORM_KV_PACK, dt, img.args(), what + " (pack of one)")
                check_norm_image(img, what + " (pack of one)", "qk_norm_rope_kv_pack_kernel", ("one",))


@pytest.mark.parametrize("pack", sorted(P.PACKS))
@pytest.mark.parametrize("rep", P.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_norm_rope_kv_packs(probe, dt, rep, pack):
    seqs = [(L, p) for L, p, _ in P.PACKS[pack]]
    what = f"qk_norm_rope_kv_pack_kernel {dt} rep {rep} {pack}"
    img = Paged(dt, rep, seqs, "norm", deltas=[d for _, _, d in P.PACKS[pack]])
    launch(probe, K_NORM_KV_PACK, dt, img.args(), what)
    check_norm_image(img, what, "qk_norm_rope_kv_pack_kernel", (pack,))


# ---- windowed kinds -------------------------------------------------------------------------------------------------------------------------
class Windowed:
    def __init__(self, dt, x):
        self.dt, self.x = dt, x
        nb, Tn, _, NH, hd = x.shape
        self.nb, self.Tn, self.NH, self.hd = nb, Tn, NH, hd
        img = torch.full((nb * Tn + GUARD_ROWS, 3 * NH * hd), float("nan"), dtype=F64)
        img[:nb * Tn] = x.reshape(nb * Tn, -1)
        self.qkv = to_dev(img, dt)
        self.qkv0 = ibits(self.qkv).clone()
        self.out = sentinel((nb * Tn + GUARD_ROWS, NH * hd), dt)

    def args(self, *, window=0, row_lo=0, np_=0, tabs=None):
        p = PrefillProbeArgs()
        p.NH, p.hd, p.np, p.Tn, p.window, p.row_lo, p.n_batch = self.NH, self.hd, np_, self.Tn, window, row_lo, self.nb
        p.scale = 1.0 / math.sqrt(self.hd)
        p.qkv, p.out = self.qkv.data_ptr(), self.out.data_ptr()
        if tabs:
            p.cos_tab, p.sin_tab = tabs[0].data_ptr(), tabs[1].data_ptr()
        return p

    def read_out(self, row_lo, what):
        unchanged(self.qkv, self.qkv0, what + " qkv")
        o = self.out.cpu()
        body = o[:self.nb * self.Tn].view(self.nb, self.Tn, self.NH, self.hd)
        assert is_sentinel(o[self.nb * self.Tn:], self.dt) and is_sentinel(body[:, :row_lo], self.dt), \
            f"{what}: an output row below row_lo or beyond Tn was written"
        return body.to(F64)


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dt", DTS)
def test_swa_attn_every_window_and_row_lo(probe, dt, hd):
    scale = 1.0 / math.sqrt(hd)
    for kind in P.KINDS:
        for Tn in P.SWA_TN:
            for nb in (1, 3):
                x = P.win_input(dt, kind, hd, nb, Tn)
                for window in P.SWA_WINDOWS:
                    ref = P.win_reference(x, window, scale)
                    for row_lo in P.swa_row_los(Tn):
                        what = f"swa_attn_kernel {dt} {kind} hd {hd} Tn {Tn} batch {nb} window {window} row_lo {row_lo}"
                        img = Windowed(dt, x)
                        launch(probe, K_SWA, dt, img.args(window=window, row_lo=row_lo), what)
                        v = P.check_win(img.read_out(row_lo, what), ref, dt, row_lo, P.EXP_REL, what=what)
                        assert v, v.msg
                        record("swa_attn_kernel", dt, v, (hd,))


@pytest.mark.parametrize("hd,np_", P.WIN_INST)
def test_win_attn_every_instantiation(probe, hd, np_):
    dt, scale = "f32", 1.0 / math.sqrt(hd)
    for kind in P.KINDS:
        for Tn, window in P.win_cases(np_):
            what = f"win_attn_kernel<{hd},{np_}> {kind} Tn {Tn} window {window}"
            x = P.win_input(dt, kind, hd, 1, Tn)
            img = Windowed(dt, x)
            launch(probe, K_WIN, dt, img.args(window=window, np_=np_), what)
            v = P.check_win(img.read_out(0, what), P.win_reference(x, window, scale), dt, 0, P.EXPF_REL, what=what)
            assert v, v.msg
            record("win_attn_kernel", dt, v, (hd, np_))


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dt", DTS)
def test_rope_rows(probe, dt, hd):
    for Tn in (5, 130):
        cos, sin = P.win_rope_table(Tn, hd)
        tabs = (cos.to(torch.float32).cuda(), sin.to(torch.float32).cuda())
        for nb in (1, 3):
            x = P.win_input(dt, "random", hd, nb, Tn)
            want, ab = P.rope_rows_reference(x, cos, sin, dt)
            for row_lo in (0, 3):
                what = f"rope_rows_kernel {dt} hd {hd} Tn {Tn} batch {nb} row_lo {row_lo}"
                img = Windowed(dt, x)
                launch(probe, K_ROPE_ROWS, dt, img.args(row_lo=row_lo, tabs=tabs), what)
                assert is_sentinel(img.out, dt), f"{what}: the attention output was written"
                bits = ibits(img.qkv).view(-1, 3, img.NH, hd)
                bits0 = img.qkv0.view(-1, 3, img.NH, hd)
                assert torch.equal(bits[:, 2], bits0[:, 2]), f"{what}: the v third was written"
                assert torch.equal(bits[nb * Tn:], bits0[nb * Tn:]), f"{what}: written beyond the last row"
                body, body0 = bits[:nb * Tn].view(nb, Tn, 3, img.NH, hd), bits0[:nb * Tn].view(nb, Tn, 3, img.NH, hd)
                assert torch.equal(body[:, :row_lo], body0[:, :row_lo]), f"{what}: a row below row_lo was written"
                got = img.qkv.cpu()[:nb * Tn].to(F64).view(nb, Tn, 3, img.NH, hd)[:, :, :2]
                v = P.check_rope_rows(got, want, ab, dt, row_lo, what=what)
                assert v, v.msg
                record("rope_rows_kernel", dt, v, (hd,))


# ---- tally --------------------------------------------------------------------------------------------------------------------------
def test_zz_every_instantiation_was_reached():
    """Runs last: the per-kernel record, and every listed instantiation reached at least once (this test needs the whole module to have
    run)."""
    print("\nkernel / storage type: cases, largest err / bound, smallest bf16 exact fraction, smallest (exact fraction - derived floor)")
    for (name, dt), st in sorted(STATS.items()):
        margin = f"{st['min_margin']:+.4f}" if st["min_margin"] < 1.0 else "-"
        print(f"  {name:34s} {dt:5s} {st['cases']:6d}  {st['ratio']:.4g}  {st['min_exact']:.5f}  {margin}")
    for shape, (same, n) in sorted(IDENTICAL.items()):
        print(f"  flash_prefill_kernel{shape}: bit-identical to <4,false> in {same} of {n} cases")
    want = set()
    for dt in DTS:
        want |= {("qk_norm_rope_kv_kernel", dt), ("prefill_attn_kernel", dt), ("rope_rows_kernel", dt, 32), ("rope_rows_kernel", dt, 64),
                 ("rope_rows_kernel", dt, 128)}
        want |= {("qk_norm_rope_kv_pack_kernel", dt, pack) for pack in list(P.PACKS) + ["one"]}
        want |= {("swa_attn_kernel", dt, hd) for hd in (32, 64, 128)}
    want |= {(f"flash_prefill_kernel<{nw},{pr}>", "bf16") for nw, pr in ((4, "false"), (4, "true"), (8, "true"))}
    want |= {("flash_prefill_small_kernel", "bf16", pack) for pack in list(P.PACKS) + ["one"]}
    want |= {("win_attn_kernel", "f32", hd, np_) for hd, np_ in P.WIN_INST}
    missing = sorted(want - REACHED, key=str)
    assert not missing, f"instantiations never launched: {missing}"
