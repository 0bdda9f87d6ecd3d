"""Conformance of every decode-time attention kernel with the float64 reference of tests/_attn_ref.py.

Each case is launched through tools/microbench/libattn_probe.so on caches whose dead rows hold a NaN bit pattern (rows > pos, every
unused block of a paged pool, the tiles beyond pos) and whose rows below n_pad hold +/- 2^60; paged forms read a shuffled block table
into a pool larger than needed.  After every launch: every cache element except row pos of each kv head keeps its bit pattern (a done
loop: every element), row pos meets the K / V check, no output element is NaN, partial slots and outputs meet the checker's bound, and
nothing is written past the outputs.  Two operand sets per case: random, and the "which key" set (V row j = (1 + j // 128) * unit
vector j % 128 under nearly equal scores: output dim d is the probability of key d, so a dropped, doubled or misplaced key moves one
element by its whole value).  The forms the code comments promise to be bit-identical are compared bit for bit; the lane kernel has a
summation order of its own and is held to the bound only.

The last test prints, per kernel, the cases run and the largest err / bound, and asserts that every listed instantiation was reached.
Observed on the MI355X (a record: no bound is tuned to it; a value stored in bf16 sits up to half an ulp from the float64 reference, so
the bf16 figures approach 1 by construction -- the fp32 figures and the bf16 exact fraction carry the information):
  kernel                        fp32: largest err / bound    bf16: largest err / bound, smallest exact fraction
  attn_decode_kernel            0.0072 (partial slots)       0.0041 (slots are fp32 in both types)
  attn_decode_batch_kernel      0.0072                       0.0043
  combine_batch_kernel          0.00069                      0.90, 0.9961 (one element of 256)
  gemv PRO_COMBINE              0.00069                      0.89, 0.9961
  attn_decode_lane_kernel       0.00069                      0.89, 0.9961
  appended K row, fp32: 0.28 of C_K at most in the float32 model of the CPU self-test (the same arithmetic).
  __expf on [-90, 0]: largest relative error 3.835e-6 at x = -87.33 (normal results), 1.17e-38 absolute below 2^-126.
Cases that found a defect: pos < n_pad (no valid key at all) made combine_finish and the lane kernel write 0 / 0 = NaN; both now
write zeros (the case stays in POSITIONS: (64, 70) and (65, 70)).  In fp32 attn_pred_group_batch_kernel differed from
attn_pred_batch_kernel by one ulp (predictor, random operands, pos 1): T = float has no rounding between the RoPE products and their
sum, so the compiler fused one product into the sum, a different one per kernel; the predictor's norm + RoPE now forbids the fusion.
"""
import ctypes as C
import os
from collections import defaultdict

import pytest
import torch

import _attn_ref as A
import _gemm_ref as G
from _attn_ref import HD, KS, MAX_WORKERS, PART_STRIDE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libattn_probe.so")
F64 = torch.float64
K_SPLIT, K_MERGE, K_MERGE_GEMV, K_PRED, K_PRED_BATCH, K_PRED_GROUP, K_BATCH_SPLIT, K_LANE = range(8)
TE = {"bf16": 0, "f32": 2}
FL_POS_PTR, FL_DONE_PTR = 1, 2
vp, i32, f32c, clong = C.c_void_p, C.c_int32, C.c_float, C.c_long
pint = C.POINTER(C.c_int)
N_KV = A.N_KV
DTS = ("f32", "bf16")


class AttnProbeArgs(C.Structure):
    _fields_ = [("n_kv", i32), ("rep", i32), ("max_seq", i32), ("workers", i32), ("paged", i32), ("ni", i32), ("n_lanes", i32),
                ("n_blocks", i32), ("n_table", i32), ("qkv_stride", i32), ("out_stride", i32), ("flags", i32), ("eps", f32c),
                ("scale", f32c), ("kv_lane_stride", clong), ("part_stride", clong), ("qkv", vp), ("q_norm_w", vp), ("k_norm_w", vp),
                ("rope", vp), ("kcache", vp), ("vcache", vp), ("part", vp), ("out", vp), ("ident", vp), ("table", pint), ("pos", pint),
                ("done", pint), ("n_pad", pint)]


STATS = defaultdict(lambda: {"cases": 0, "ratio": 0.0, "min_exact": 1.0})       # per kernel and storage type
REACHED = set()                                                                  # instantiations launched


def record(kernel, dt, v, inst=()):
    st = STATS[(kernel, dt)]
    st["cases"] += 1
    st["ratio"] = max(st["ratio"], v.ratio)
    st["min_exact"] = min(st["min_exact"], v.exact)
    REACHED.add((kernel, dt) + tuple(inst))


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libattn_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.attn_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(AttnProbeArgs), vp]
    lib.attn_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(AttnProbeArgs)]
    lib.attn_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.attn_probe_expf.argtypes = [vp, vp, C.c_int, vp]
    assert lib.attn_probe_version() == 1 and lib.attn_probe_kinds() == 8
    buf = (C.c_long * 64)()
    n = lib.attn_probe_layout(buf, 64)
    want = [C.sizeof(AttnProbeArgs)] + [getattr(AttnProbeArgs, f[0]).offset for f in AttnProbeArgs._fields_]
    assert list(buf[:n - 5]) == want, "ctypes mirror of AttnProbeArgs is out of date"
    assert list(buf[n - 3:n]) == [128, MAX_WORKERS, PART_STRIDE]
    return lib


def launch(probe, kind, dt, p, what):
    assert probe.attn_probe_admits(kind, TE[dt], C.byref(p)) == 1, f"{what}: the probe refuses kind {kind}"
    rc = probe.attn_probe_run(kind, TE[dt], C.byref(p), None)
    assert rc == 0, f"{what}: kind {kind} returned {rc}"


# ---- device images -----------------------------------------------------------------------------------------------------------
def ibits(t):
    """The raw bits of a storage tensor as an integer view (NaN-safe comparisons)."""
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sentinel(shape, dt):
    v = G.SENTINEL[dt]
    t = torch.full(shape, v - (1 << 32) if v >= (1 << 31) else v, dtype=torch.int32, device="cuda")
    return t.to(torch.int16).view(torch.bfloat16) if dt == "bf16" else t.view(torch.float32)


def to_dev(x, dt):
    """float64 (T values; NaN = dead) -> storage on the device, NaN as the sentinel bit pattern."""
    t = G.to_storage(torch.nan_to_num(x, nan=0.0), dt).cuda()
    s = G.SENTINEL[dt]
    ibits(t)[torch.isnan(x).cuda()] = (s & 0xFFFF) - (1 << 16) if dt == "bf16" else s - (1 << 32)
    return t


def is_sentinel(t, dt):
    return bool((G.raw_bits(t.cpu()) == G.SENTINEL[dt]).all())


@pytest.fixture(scope="module")
def ident():
    cache = {}

    def get(dt, n):
        if (dt, n) not in cache:
            cache[(dt, n)] = torch.eye(n, dtype=torch.bfloat16 if dt == "bf16" else torch.float32, device="cuda")
        return cache[(dt, n)]
    return get


class Lanes:
    """The device image of B lanes (cases of one dt / n_kv / rep / max_seq): token rows, RoPE rows, caches, partial slots, outputs."""
    GUARD = 128

    def __init__(self, cases, *, paged, done=None, tables=None, table_seed=0):
        c0 = cases[0]
        self.cases, self.paged, self.dt = cases, paged, c0.dt
        self.B, self.n_kv, self.rep, self.max_seq = len(cases), c0.n_kv, c0.rep, c0.max_seq
        B, dt, n_kv, rep = self.B, self.dt, self.n_kv, self.rep
        self.done = list(done) if done is not None else [0] * B
        self.row = (rep + 2) * n_kv * HD
        self.qkv_stride = self.row + 8
        qkv = torch.full((B, self.qkv_stride), float("nan"), dtype=F64)
        qkv[:, :self.row] = torch.stack([c.qkv for c in cases])
        self.qkv = to_dev(qkv, dt)
        self.qw, self.kw = to_dev(c0.qw, dt), to_dev(c0.kw, dt)
        self.rope = torch.stack([torch.cat([c.cos, c.sin]) for c in cases]).to(torch.float32).cuda()
        self.n_tiles = (self.max_seq + KS - 1) // KS
        self.n_blocks = self.n_tiles + 3
        if paged:
            assert self.max_seq % KS == 0
            if tables is None:
                tables = []
                for l in range(B):
                    g = torch.Generator().manual_seed(1000 * table_seed + 17 * l + cases[l].pos)
                    t = torch.randperm(self.n_blocks, generator=g)[:self.n_tiles].tolist()
                    if t == sorted(t):
                        t = t[::-1]                      # (shuffled AND non-monotonic)
                    tables.append(t)
            self.tables = tables
            numel = self.n_blocks * n_kv * KS * HD
        else:
            self.tables = None
            numel = n_kv * self.max_seq * HD
        self.kv_stride = numel + self.GUARD
        imgs = [torch.full((B, self.kv_stride), float("nan"), dtype=F64) for _ in range(2)]
        for l, c in enumerate(cases):
            for img, X in zip(imgs, c.cache_image()):
                if paged:
                    pool = img[l, :numel].view(self.n_blocks, n_kv, KS, HD)
                    for t in range(self.n_tiles):
                        pool[self.tables[l][t]] = X[:, t * KS:(t + 1) * KS]
                else:
                    img[l, :numel] = X.flatten()
        self.K, self.V = to_dev(imgs[0], dt), to_dev(imgs[1], dt)
        self.K0, self.V0 = ibits(self.K).clone(), ibits(self.V).clone()
        self.part_elems = n_kv * MAX_WORKERS * rep * PART_STRIDE
        self.part_stride = self.part_elems + 4
        self.out_stride = c0.q_dim + 8
        self.fresh_outputs()
        # host arrays the probe reads (kept alive here)
        self.c_pos = (C.c_int * B)(*[c.pos for c in cases])
        self.c_done = (C.c_int * B)(*self.done)
        self.c_npad = (C.c_int * B)(*[c.n_pad for c in cases])
        flat = [e for t in self.tables for e in t] if paged else [0]
        self.c_table = (C.c_int * len(flat))(*flat)

    def fresh_outputs(self):
        self.part = sentinel((self.B, self.part_stride), "f32")
        self.out = sentinel((self.B, self.out_stride), self.dt)

    def args(self, *, workers=0, ni=0, flags=0, ident=None):
        c0 = self.cases[0]
        p = AttnProbeArgs()
        p.n_kv, p.rep, p.max_seq, p.workers, p.paged, p.ni, p.n_lanes = self.n_kv, self.rep, self.max_seq, workers, int(self.paged), ni, self.B
        p.n_blocks, p.n_table = (self.n_blocks, self.n_tiles) if self.paged else (0, 0)
        p.qkv_stride, p.out_stride, p.flags, p.eps, p.scale = self.qkv_stride, self.out_stride, flags, c0.eps, c0.scale
        p.kv_lane_stride, p.part_stride = self.kv_stride, self.part_stride
        p.qkv, p.q_norm_w, p.k_norm_w, p.rope = self.qkv.data_ptr(), self.qw.data_ptr(), self.kw.data_ptr(), self.rope.data_ptr()
        p.kcache, p.vcache, p.part, p.out = self.K.data_ptr(), self.V.data_ptr(), self.part.data_ptr(), self.out.data_ptr()
        p.ident = ident.data_ptr() if ident is not None else None
        p.table, p.pos, p.done, p.n_pad = self.c_table, self.c_pos, self.c_done, self.c_npad
        return p

    def row_offset(self, l, g):
        pos = self.cases[l].pos
        if self.paged:
            return ((self.tables[l][pos // KS] * self.n_kv + g) * KS + pos % KS) * HD
        return (g * self.max_seq + pos) * HD

    def check_cache(self, refs, what):
        """Every element keeps its bits except row pos of every kv head of a lane that is not done, which meets the K / V check."""
        worst = 0.0
        for X, X0, is_k in ((self.K, self.K0, True), (self.V, self.V0, False)):
            a = ibits(X).clone()
            for l in range(self.B):
                if not self.done[l]:
                    for g in range(self.n_kv):
                        o = self.row_offset(l, g)
                        a[l, o:o + HD] = X0[l, o:o + HD]
            diff = a != X0
            assert not bool(diff.any()), f"{what}: {int(diff.sum())} stray writes into the {'K' if is_k else 'V'} cache, first at (lane, element) " \
                                         f"{tuple(int(v) for v in torch.nonzero(diff)[0])}"
        for l in range(self.B):
            if self.done[l]:
                continue
            rows = [torch.stack([X[l, self.row_offset(l, g):self.row_offset(l, g) + HD] for g in range(self.n_kv)]).cpu().to(F64)
                    for X in (self.K, self.V)]
            v = A.check_kv_row(rows[0], rows[1], refs[l], self.dt, what=f"{what} lane {l}")
            assert v, v.msg
            worst = max(worst, v.ratio)
        return worst

    def read_out(self, what):
        """[B][heads][128] float64; nothing written past q_dim, no NaN inside."""
        q_dim = self.cases[0].q_dim
        o = self.out.cpu()
        assert is_sentinel(o[:, q_dim:], self.dt), f"{what}: written past the output row"
        vals = o[:, :q_dim].to(F64).view(self.B, -1, HD)
        assert not bool(torch.isnan(vals).any()), f"{what}: NaN (or an unwritten element) in the output"
        return vals

    def read_part(self, S, what):
        """[B][n_kv][8][rep][132] float64 (slots >= S and the pad words must keep the sentinel)."""
        pt = self.part.cpu()
        assert is_sentinel(pt[:, self.part_elems:], "f32"), f"{what}: written past the partial slots"
        pv = pt[:, :self.part_elems].view(self.B, self.n_kv, MAX_WORKERS, self.rep, PART_STRIDE)
        assert is_sentinel(pv[:, :, S:], "f32") and is_sentinel(pv[..., HD + 2:], "f32"), f"{what}: a slot >= S or a pad word was written"
        assert not bool(torch.isnan(pv[:, :, :S, :, :HD + 2]).any()), f"{what}: NaN (or an unwritten element) in a partial slot"
        return pv.to(F64)


def merge_both_ways(probe, ident, L, S, ref, what):
    """combine_batch_kernel and the PRO_COMBINE GEMV through the identity weight on the slots L.part holds: bit-identical, within the bound."""
    dt, q_dim = L.dt, L.cases[0].q_dim
    launch(probe, K_MERGE, dt, L.args(workers=S), what)
    got = L.read_out(what + " merge")
    bits_m = ibits(L.out).clone()
    L.out = sentinel((L.B, L.out_stride), dt)
    launch(probe, K_MERGE_GEMV, dt, L.args(workers=S, ident=ident(dt, q_dim)), what)
    L.read_out(what + " PRO_COMBINE gemv")
    assert torch.equal(ibits(L.out), bits_m), f"{what}: the PRO_COMBINE GEMV through the identity differs from combine_batch_kernel"
    v = A.check_output(got[0], ref, dt, what=what + " combine_batch_kernel")
    assert v, v.msg
    record("combine_batch_kernel", dt, v)
    record("gemv PRO_COMBINE", dt, v)
    return bits_m


def split_case(probe, ident, c, S, paged, i, *, done=0):
    what = f"split {c.dt} {c.kind} rep {c.rep} S {S} {'paged' if paged else 'contiguous'} pos {c.pos} n_pad {c.n_pad} done {done}"
    ref = A.reference(c, S)
    L = Lanes([c], paged=paged, done=[done], table_seed=i)
    flags = (FL_POS_PTR if i % 2 else 0) | (FL_DONE_PTR if (done or i % 3 == 0) else 0)
    launch(probe, K_SPLIT, c.dt, L.args(workers=S, flags=flags), what)
    part = L.read_part(S, what)
    assert is_sentinel(L.out, c.dt), f"{what}: the split kernel wrote the output buffer"
    v = A.check_partials(part[0], ref, what=what)
    assert v, v.msg
    record("attn_decode_kernel", c.dt, v, (c.rep, paged))
    L.check_cache([ref], what)
    merge_both_ways(probe, ident, L, S, ref, what)


# ---- the probe refuses what would leave the buffers (nothing is launched) ---------------------------------------------------------
def test_probe_refuses_out_of_bounds_arguments(probe):
    refused = probe.attn_probe_refused_code()
    cases = [A.make_case("bf16", "random", N_KV, 2, pos, 0, A.MAX_SEQ) for pos in (5, 70)]
    L = Lanes(cases, paged=True)

    def variants():
        base = lambda: L.args(workers=3, ni=4)
        yield "baseline", K_BATCH_SPLIT, base(), True
        yield "baseline lane", K_LANE, base(), True
        pos = (C.c_int * 2)(5, A.MAX_SEQ)
        p = base(); p.pos = pos
        yield "pos >= max_seq", K_LANE, p, False
        for bad in (-1, L.n_blocks):
            tab = (C.c_int * (2 * L.n_tiles))(*[e for t in L.tables for e in t])
            tab[L.n_tiles + 9] = bad
            p = base(); p.table = tab
            yield f"table entry {bad} outside the pool", K_BATCH_SPLIT, p, False
        p = base(); p.n_table = L.n_tiles - 1
        yield "fewer table entries than ceil(max_seq / 64)", K_BATCH_SPLIT, p, False
        for w in (0, 9):
            p = base(); p.workers = w
            yield f"workers {w}", K_BATCH_SPLIT, p, False
        p = base(); p.rep = 3
        yield "rep 3", K_LANE, p, False
        p = base(); p.n_lanes = 129
        yield "129 lanes", K_LANE, p, False
        p = base(); p.ni = 3
        yield "NI 3", K_LANE, p, False
        for name, d in (("qkv_stride", 1), ("out_stride", 4), ("part_stride", 2), ("kv_lane_stride", 4)):
            p = base(); setattr(p, name, getattr(p, name) + d)
            yield f"misaligned {name}", K_BATCH_SPLIT, p, False
        p = base(); p.n_lanes = 1; p.flags = 0
        done = (C.c_int * 1)(1)
        p.done = done
        yield "single-stream done without a done_ptr", K_SPLIT, p, False
        p = base(); p.max_seq = 17; p.n_lanes = 1; p.paged = 0
        pos = (C.c_int * 1)(17)
        p.pos = pos
        yield "predictor pos 17 of 17", K_PRED, p, False

    for name, kind, p, ok in variants():
        assert probe.attn_probe_admits(kind, 0, C.byref(p)) == int(ok), name
        if not ok:
            assert probe.attn_probe_run(kind, 0, C.byref(p), None) == refused, name
    assert is_sentinel(L.out, "bf16") and is_sentinel(L.part, "f32") and torch.equal(ibits(L.K), L.K0)


# ---- the exponential ---------------------------------------------------------------------------------------------------------------
def test_expf_grid(probe):
    """__expf on 2^16 + 1 arguments in [-90, 0] against float64 exp: the measured maximum relative error (over normal results) is what
    A.EXP_REL doubles."""
    x = torch.linspace(-90.0, 0.0, 65537, dtype=F64).to(torch.float32).cuda()
    y = torch.empty_like(x)
    assert probe.attn_probe_expf(x.data_ptr(), y.data_ptr(), x.numel(), None) == 0
    xe, ye = x.cpu().to(F64), y.cpu().to(F64)
    ref = torch.exp(xe)
    normal = ref >= 2.0 ** -126
    rel = ((ye - ref).abs() / ref)[normal]
    worst = int(torch.argmax(rel))
    flushed = (ye - ref).abs()[~normal]
    print(f"\n__expf: max relative error {float(rel.max()):.4g} at x = {float(xe[normal][worst]):.4f}; below 2^-126: max absolute error "
          f"{float(flushed.max()):.3g}")
    assert float(ye[-1]) == 1.0, "__expf(0) must be exactly 1 (a rescale by an unchanged maximum is exact)"
    assert float(flushed.max()) <= 2.0 ** -126
    assert 2.0 * float(rel.max()) <= A.EXP_REL, "update EXP_REL in tests/_attn_ref.py: it must be twice the measured error"


# ---- split-KV, single stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("S", A.WORKERS)
@pytest.mark.parametrize("rep", A.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_split_kv_every_position(probe, ident, dt, rep, S, paged):
    i = 0
    for kind in A.KINDS:
        for pos, n_pad in A.POSITIONS:
            split_case(probe, ident, A.make_case(dt, kind, N_KV, rep, pos, n_pad, A.MAX_SEQ), S, paged, i)
            i += 1
    for done in (1, 2):             # a done loop appends nothing; its partials are still valid
        for pos, n_pad in ((64, 0), (200, 70)):
            split_case(probe, ident, A.make_case(dt, "random", N_KV, rep, pos, n_pad, A.MAX_SEQ), S, paged, i, done=done)
            i += 1


@pytest.mark.parametrize("rep", A.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_split_kv_clamped_last_tile(probe, ident, dt, rep):
    """max_seq = 200 is no multiple of 64: the contiguous form clamps the reads of the last tile."""
    for i, (kind, (pos, n_pad)) in enumerate((k, p) for k in A.KINDS for p in A.CLAMP_CASE["positions"]):
        split_case(probe, ident, A.make_case(dt, kind, N_KV, rep, pos, n_pad, A.CLAMP_CASE["max_seq"]), A.CLAMP_CASE["S"], False, i)


# ---- lock-step batch forms ---------------------------------------------------------------------------------------------------------
def groups_of_3(positions):
    pad = positions + positions[:(-len(positions)) % 3]
    return [pad[i:i + 3] for i in range(0, len(pad), 3)]


def batch_split_launch(probe, cases, S, done, what, seed):
    """attn_decode_batch_kernel + combine_batch_kernel on B lanes; every lane against its own reference, and bit for bit against the
    single-stream paged kernel + combine_batch_kernel on the same image."""
    dt, rep = cases[0].dt, cases[0].rep
    L = Lanes(cases, paged=True, done=done, table_seed=seed)
    launch(probe, K_BATCH_SPLIT, dt, L.args(workers=S), what)
    part, out = L.read_part(S, what), L.read_out(what)
    refs = [A.reference(c, S) for c in cases]
    L.check_cache(refs, what)
    for l, c in enumerate(cases):
        wl = f"{what} lane {l} (pos {c.pos} n_pad {c.n_pad} done {done[l]})"
        if done[l]:
            sl = part[l][:, :S]
            assert bool((sl[..., :HD] == 0).all()) and bool((sl[..., HD] == 0).all()) and bool((sl[..., HD + 1] == 1).all()), \
                f"{wl}: a done lane's slots are not the neutral {{0, m = 0, l = 1}}"
            assert bool((out[l] == 0).all()), f"{wl}: a done lane's merged output is not zero"
            continue
        v = A.check_partials(part[l], refs[l], what=wl)
        assert v, v.msg
        record("attn_decode_batch_kernel", dt, v, (rep,))
        v = A.check_output(out[l], refs[l], dt, what=wl + " merged")
        assert v, v.msg
        record("combine_batch_kernel", dt, v)
        single = Lanes([c], paged=True, tables=[L.tables[l]])
        launch(probe, K_SPLIT, dt, single.args(workers=S), wl)
        launch(probe, K_MERGE, dt, single.args(workers=S), wl)
        assert torch.equal(ibits(single.part)[0], ibits(L.part)[l]), f"{wl}: partial slots differ from attn_decode_kernel<PAGED>"
        assert torch.equal(ibits(single.out)[0], ibits(L.out)[l]), f"{wl}: merged output differs from attn_decode_kernel<PAGED> + combine"
        o = single.row_offset(0, 0)
        assert torch.equal(ibits(single.K)[0, o:o + HD], ibits(L.K)[l, o:o + HD])
        REACHED.add(("attn_decode_kernel", dt, rep, True))


@pytest.mark.parametrize("S", A.WORKERS)
@pytest.mark.parametrize("rep", A.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_batch_split_every_position(probe, dt, rep, S):
    for kind in A.KINDS:
        for i, grp in enumerate(groups_of_3(A.POSITIONS)):
            cases = [A.make_case(dt, kind, N_KV, rep, pos, n_pad, A.MAX_SEQ) for pos, n_pad in grp]
            batch_split_launch(probe, cases, S, [0, 0, 0], f"batch split {dt} {kind} rep {rep} S {S}", i)


def three_lanes(dt, kind, rep):
    return [A.make_case(dt, kind, N_KV, rep, pos, n_pad, A.MAX_SEQ, seed=l) for l, (pos, n_pad) in enumerate(A.BATCH3)]


@pytest.mark.parametrize("done", [1, 2])
@pytest.mark.parametrize("rep", A.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_batch_split_three_different_lanes_one_done(probe, dt, rep, done):
    """Different pos, n_pad, caches and tables in one launch: one lane at pos 0, one done (it must not touch its cache)."""
    for kind in A.KINDS:
        for S in A.WORKERS:
            for which in range(3):
                d = [done if l == which else 0 for l in range(3)]
                batch_split_launch(probe, three_lanes(dt, kind, rep), S, d, f"batch split {dt} {kind} rep {rep} S {S}", which)


def lane_launch(probe, cases, ni, done, what, seed):
    dt, rep = cases[0].dt, cases[0].rep
    L = Lanes(cases, paged=True, done=done, table_seed=seed)
    launch(probe, K_LANE, dt, L.args(ni=ni), what)
    out = L.read_out(what)
    assert is_sentinel(L.part, "f32"), f"{what}: the lane kernel wrote the partial slots"
    refs = [A.reference(c) for c in cases]
    L.check_cache(refs, what)
    for l, c in enumerate(cases):
        wl = f"{what} lane {l} (pos {c.pos} n_pad {c.n_pad} done {done[l]})"
        if done[l]:
            assert bool((out[l] == 0).all()), f"{wl}: a done lane's output is not zero"
            continue
        v = A.check_output(out[l], refs[l], dt, what=wl)
        assert v, v.msg
        record("attn_decode_lane_kernel", dt, v, (rep, ni))


@pytest.mark.parametrize("ni", [2, 4])
@pytest.mark.parametrize("rep", A.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_lane_kernel_every_position(probe, dt, rep, ni):
    positions = A.POSITIONS + (A.LANE_NI2_EXTRA if ni == 2 else [])
    for kind in A.KINDS:
        for i, grp in enumerate(groups_of_3(positions)):
            cases = [A.make_case(dt, kind, N_KV, rep, pos, n_pad, A.MAX_SEQ) for pos, n_pad in grp]
            lane_launch(probe, cases, ni, [0, 0, 0], f"lane kernel {dt} {kind} rep {rep} NI {ni}", i)
        for done in (1, 2):
            for which in range(3):
                d = [done if l == which else 0 for l in range(3)]
                lane_launch(probe, three_lanes(dt, kind, rep), ni, d, f"lane kernel {dt} {kind} rep {rep} NI {ni}", which)


# ---- code predictor --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_predictor_every_position(probe, dt):
    """attn_pred_kernel, attn_pred_batch_kernel and attn_pred_group_batch_kernel at every position of the 17-slot cache: each lane
    against its reference, the three forms bit for bit."""
    rep = 2
    for kind in A.KINDS:
        for pos in A.PRED_POSITIONS:
            what = f"predictor {dt} {kind} pos {pos}"
            cases = [A.make_case(dt, kind, N_KV, rep, pos, 0, 17, seed=l) for l in range(3)]
            refs = [A.reference(c) for c in cases]
            bits = {}
            for kind_id, name in ((K_PRED_BATCH, "attn_pred_batch_kernel"), (K_PRED_GROUP, "attn_pred_group_batch_kernel")):
                L = Lanes(cases, paged=False)
                launch(probe, kind_id, dt, L.args(), what)
                out = L.read_out(f"{what} {name}")
                assert is_sentinel(L.part, "f32")
                L.check_cache(refs, f"{what} {name}")
                for l in range(3):
                    v = A.check_output(out[l], refs[l], dt, what=f"{what} {name} lane {l}")
                    assert v, v.msg
                    record(name, dt, v, (rep,) if kind_id == K_PRED_GROUP else ())
                bits[name] = (ibits(L.out).clone(), ibits(L.K).clone(), ibits(L.V).clone())
            for a, b in zip(bits["attn_pred_batch_kernel"], bits["attn_pred_group_batch_kernel"]):
                assert torch.equal(a, b), f"{what}: the group form differs from the per-head batch form"
            L1 = Lanes(cases[:1], paged=False)
            launch(probe, K_PRED, dt, L1.args(), what)
            out = L1.read_out(f"{what} attn_pred_kernel")
            L1.check_cache(refs[:1], f"{what} attn_pred_kernel")
            v = A.check_output(out[0], refs[0], dt, what=f"{what} attn_pred_kernel")
            assert v, v.msg
            record("attn_pred_kernel", dt, v)
            assert torch.equal(ibits(L1.out)[0], bits["attn_pred_batch_kernel"][0][0]), f"{what}: attn_pred_kernel differs from the batch form"
            n = L1.K.shape[1]
            assert torch.equal(ibits(L1.K)[0], bits["attn_pred_batch_kernel"][1][0, :n])


# ---- the merge alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_part", [1, 3, 8])
@pytest.mark.parametrize("rep", A.REPS)
@pytest.mark.parametrize("dt", DTS)
def test_merge_alone_on_synthetic_slots(probe, ident, dt, rep, n_part):
    """Slots >= n_part hold NaN and must be ignored; empty slots {m = -1e30, l = 0} sit between live ones; the maxima spread over 60
    units (weights underflow towards 0 without harming the rest)."""
    B, q_dim = 2, N_KV * rep * HD
    gen = torch.Generator().manual_seed(900 + 10 * rep + n_part)
    part_elems = N_KV * MAX_WORKERS * rep * PART_STRIDE
    for trial in range(4):
        slots = torch.full((B, N_KV, MAX_WORKERS, rep, PART_STRIDE), float("nan"), dtype=F64)
        num = torch.randn(B, N_KV, n_part, rep, HD, generator=gen, dtype=F64) * 3.0
        m = torch.rand(B, N_KV, n_part, rep, generator=gen, dtype=F64) * 60.0 - 30.0
        l = 1.0 + 49.0 * torch.rand(B, N_KV, n_part, rep, generator=gen, dtype=F64)
        empty = torch.rand(B, N_KV, n_part, rep, generator=gen) < 0.3
        empty[:, :, trial % n_part] = False                     # at least one live slot per head
        num[empty], m[empty], l[empty] = 0.0, A.EMPTY_M, 0.0
        slots[:, :, :n_part, :, :HD], slots[:, :, :n_part, :, HD], slots[:, :, :n_part, :, HD + 1] = num, m, l
        s32 = G.rnd(torch.nan_to_num(slots, nan=0.0), "f32")
        img = torch.full((B, part_elems + 4), float("nan"), dtype=F64)
        img[:, :part_elems] = slots.view(B, -1)
        part = to_dev(img, "f32")
        out = sentinel((B, q_dim + 8), dt)
        p = AttnProbeArgs()
        p.n_kv, p.rep, p.workers, p.n_lanes, p.out_stride, p.part_stride = N_KV, rep, n_part, B, q_dim + 8, part_elems + 4
        p.part, p.out = part.data_ptr(), out.data_ptr()
        what = f"merge alone {dt} rep {rep} n_part {n_part} trial {trial}"
        launch(probe, K_MERGE, dt, p, what)
        o = out.cpu()
        assert is_sentinel(o[:, q_dim:], dt), f"{what}: written past the output row"
        got = o[:, :q_dim].to(F64).view(B, -1, HD)
        for lane in range(B):
            v = A.check_merge(got[lane], s32[lane, :, :, :, :HD], s32[lane, :, :, :, HD], s32[lane, :, :, :, HD + 1], n_part, dt,
                              what=f"{what} lane {lane}")
            assert v, v.msg
            record("combine_batch_kernel", dt, v)
        out1 = sentinel((1, q_dim + 8), dt)
        p.n_lanes, p.out, p.ident = 1, out1.data_ptr(), ident(dt, q_dim).data_ptr()
        launch(probe, K_MERGE_GEMV, dt, p, what)
        assert torch.equal(ibits(out1)[0], ibits(out)[0]), f"{what}: the PRO_COMBINE GEMV through the identity differs from combine_batch_kernel"
        REACHED.add(("gemv PRO_COMBINE", dt))
        assert torch.equal(G.raw_bits(part.cpu()), G.raw_bits(to_dev(img, "f32").cpu())), f"{what}: the merge wrote its input"


# ---- tally --------------------------------------------------------------------------------------------------------------------------
def test_zz_every_instantiation_was_reached():
    """Runs last: the per-kernel record, and every listed kernel, rep, dtype, PAGED and NI instantiation reached at least once (this
    test needs the whole module to have run)."""
    print("\nkernel / storage type: cases, largest err / bound, smallest bf16 exact fraction")
    for (name, dt), st in sorted(STATS.items()):
        print(f"  {name:32s} {dt:5s} {st['cases']:6d}  {st['ratio']:.4g}  {st['min_exact']:.5f}")
    want = set()
    for dt in DTS:
        want |= {("attn_decode_kernel", dt, rep, paged) for rep in A.REPS for paged in (False, True)}
        want |= {("attn_decode_batch_kernel", dt, rep) for rep in A.REPS}
        want |= {("attn_decode_lane_kernel", dt, rep, ni) for rep in A.REPS for ni in (2, 4)}
        want |= {("combine_batch_kernel", dt), ("gemv PRO_COMBINE", dt), ("attn_pred_kernel", dt), ("attn_pred_batch_kernel", dt),
                 ("attn_pred_group_batch_kernel", dt, 2)}
    missing = sorted(want - REACHED, key=str)
    assert not missing, f"instantiations never launched: {missing}"
