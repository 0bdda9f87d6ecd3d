"""Conformance of the continuation prefill kernels with the float64 reference of tests/_prefill_cont_ref.py.

Each kernel is launched alone through tools/microbench/libprefill_cont_probe.so, with the conventions of
tests/test_gpu_prefill_attn_reference.py: the pool is larger than needed and read through a shuffled block table; every unowned block,
every cache row the kernel must not touch (below start, beyond start + n), the k | v thirds of the attention kinds' qkv, the guard rows
behind qkv / out / the split workspace hold a NaN sentinel bit pattern and are compared bit for bit afterwards.  The dead rows of OWNED
blocks (beyond start + n in the last tile) hold +/- 2^60 for the flash kernel -- finite, per its contract -- and the sentinel for the
wave kernel.  Operand sets: random, and "which key".  Head ratio 2, both storage types for the norm and wave kernels.

Cases: tests/_prefill_cont_ref.py (start in {0, 1, 63, 64, 65, 130, 200, 448} x n in {1, 16, 17, 63, 64, 65, 130}, the longer starts
for the split counts, and split counts forced by hand).  With S > 1 the flash kernel must leave `out` alone (it writes records only) and
the merge kernel is launched on its own afterwards.  The last test asserts that every instantiation and every split count the launcher
can choose up to 1100 keys was reached, and prints cases, largest err / bound and smallest bf16 exact fraction per kernel as a record.

Observed on the MI355X (a record: no bound or floor is tuned to it; a value stored in bf16 sits up to half an ulp from the float64
reference, so the bf16 err / bound figures approach 1 by construction):
  kernel                               type   cases   largest err / bound   smallest exact fraction
  qk_norm_rope_kv_cont_kernel          f32       56   0.2955 of C_K         -
  qk_norm_rope_kv_cont_kernel          bf16      56   bit-exact             1.00000
  prefill_attn_cont_kernel             f32      116   0.0012                -
  prefill_attn_cont_kernel             bf16     116   0.9581                0.99805
  flash_prefill_cont_kernel (S = 1)    bf16     102   0.9917                0.99609
  flash_prefill_cont_kernel + merge    bf16      30   0.9895                0.99609
  split counts reached: 1, 2, 3, 4, 5.  No case found a defect: no NaN, no touched sentinel, no element outside its bound."""
import ctypes as C
import os
from collections import defaultdict

import pytest
import torch

import _prefill_attn_ref as P
import _prefill_cont_ref as R
from _attn_ref import BIG
from _prefill_attn_ref import HD, KS, N_KV
from test_gpu_attn_reference import ibits, is_sentinel, sentinel, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libprefill_cont_probe.so")
F64 = torch.float64
K_NORM, K_WAVE, K_FLASH, K_MERGE = range(4)
TE = {"bf16": 0, "f32": 2}
vp, i32, f32c = C.c_void_p, C.c_int32, C.c_float
GUARD = 2
NH, PER = R.NH, R.NH + 2 * N_KV


class ContProbeArgs(C.Structure):
    _fields_ = [("NH", i32), ("NKV", i32), ("start", i32), ("n", i32), ("qkv_rows", i32), ("rope_len", i32), ("rope_delta", i32),
                ("n_blocks", i32), ("n_table", i32), ("S", i32), ("ws_floats", C.c_long), ("eps", f32c), ("scale", f32c), ("qkv", vp),
                ("q_norm_w", vp), ("k_norm_w", vp), ("cos_tab", vp), ("sin_tab", vp), ("kpool", vp), ("vpool", vp), ("out", vp), ("ws", vp),
                ("table", C.POINTER(C.c_int))]


STATS = defaultdict(lambda: {"cases": 0, "ratio": 0.0, "min_exact": 1.0})
SPLITS_REACHED = set()


def record(kernel, dt, v):
    st = STATS[(kernel, dt)]
    st["cases"] += 1
    st["ratio"] = max(st["ratio"], v.ratio)
    st["min_exact"] = min(st["min_exact"], v.exact)


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libprefill_cont_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.cont_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(ContProbeArgs), vp]
    lib.cont_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(ContProbeArgs)]
    lib.cont_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.cont_probe_splits.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long]
    assert lib.cont_probe_version() == 1 and lib.cont_probe_kinds() == 4 and lib.cont_probe_record_floats() == R.REC
    buf = (C.c_long * 64)()
    n = lib.cont_probe_layout(buf, 64)
    assert list(buf[:n]) == [C.sizeof(ContProbeArgs)] + [getattr(ContProbeArgs, f[0]).offset for f in ContProbeArgs._fields_]
    return lib


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def table_for(tiles, n_blocks, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    perm = torch.randperm(n_blocks, generator=g).tolist()
    while any(perm[i] == i for i in range(tiles)):               # no owned tile in the block the identity table would name
        perm = torch.randperm(n_blocks, generator=g).tolist()
    return perm[:tiles]


class Image:
    """One continuation in an oversized pool.  mode "finite" / "nan": attention (the new rows' q, the cache filled up to start + n, dead
    rows of the last owned tile +/- 2^60 or NaN); "norm": the new rows before the norm, every pool row a sentinel."""

    def __init__(self, dt, kind, start, n, mode, seed=0):
        self.dt, self.start, self.n, self.mode = dt, start, n, mode
        L = start + n
        self.tiles = (L + KS - 1) // KS
        self.n_blocks = self.tiles + 3
        self.table = table_for(self.tiles, self.n_blocks, seed + 7 * start + n)
        pools = [torch.full((self.n_blocks, N_KV, KS, HD), float("nan"), dtype=F64) for _ in range(2)]
        qkv = torch.full((n + GUARD, PER, HD), float("nan"), dtype=F64)
        if mode == "norm":
            qkv[:n] = R.norm_input(dt, L)[start:]
        else:
            q, K, V = R.operands(dt, kind, start, n)
            qkv[:n, :NH] = q[start:]
            r = torch.arange(KS * self.tiles)
            sign = 1.0 - 2.0 * ((r[:, None] + torch.arange(HD)[None, :]) % 2).to(F64)
            for pool, X in zip(pools, (K, V)):
                full = torch.full((N_KV, KS * self.tiles, HD), float("nan"), dtype=F64)
                full[:, :L] = X
                if mode == "finite":
                    full[:, L:] = (BIG * sign)[L:]
                for t in range(self.tiles):
                    pool[self.table[t]] = full[:, t * KS:(t + 1) * KS]
        self.K, self.V, self.qkv = to_dev(pools[0], dt), to_dev(pools[1], dt), to_dev(qkv, dt)
        self.K0, self.V0, self.qkv0 = ibits(self.K).clone(), ibits(self.V).clone(), ibits(self.qkv).clone()
        self.out = sentinel((n + GUARD, NH, HD), dt)
        self.c_table = (C.c_int * self.tiles)(*self.table)
        self.ws = None

    def args(self, S=1, delta=0):
        p = ContProbeArgs()
        p.NH, p.NKV, p.start, p.n, p.qkv_rows = NH, N_KV, self.start, self.n, self.n
        p.rope_len, p.rope_delta, p.n_blocks, p.n_table, p.S = R.ROPE_LEN, delta, self.n_blocks, self.tiles, S
        p.eps, p.scale = P.EPS, P.SCALE
        p.qkv, p.out, p.kpool, p.vpool = self.qkv.data_ptr(), self.out.data_ptr(), self.K.data_ptr(), self.V.data_ptr()
        p.table = C.cast(self.c_table, C.POINTER(C.c_int))
        if self.mode == "norm":
            import _attn_ref as A
            qw, kw = A.base_gains(self.dt, "random")
            ct, st = P.rope_table(R.ROPE_LEN)
            self.keep = (to_dev(qw, self.dt), to_dev(kw, self.dt), ct.to(torch.float32).cuda(), st.to(torch.float32).cuda())
            p.q_norm_w, p.k_norm_w, p.cos_tab, p.sin_tab = (t.data_ptr() for t in self.keep)
        if S > 1:
            self.ws_n = S * self.n * NH * R.REC
            self.ws = sentinel((self.ws_n + 64,), "f32")
            p.ws, p.ws_floats = self.ws.data_ptr(), self.ws_n
        return p

    def inputs_unchanged(self, what):
        for t, t0, name in ((self.K, self.K0, "K pool"), (self.V, self.V0, "V pool"), (self.qkv, self.qkv0, "qkv")):
            assert torch.equal(ibits(t), t0), f"{what}: the {name} changed"

    def logical(self, pool):
        return torch.cat([pool[self.table[t]] for t in range(self.tiles)], dim=1)


def launch(probe, kind, dt, p, what):
    assert probe.cont_probe_admits(kind, TE[dt], C.byref(p)) == 1, f"{what}: the probe refuses kind {kind}"
    rc = probe.cont_probe_run(kind, TE[dt], C.byref(p), None)
    assert rc == 0, f"{what}: kind {kind} returned {rc}"


def from_dev(t, dt):
    """storage -> float64 with the sentinel as NaN"""
    import _gemm_ref as G
    x = t.cpu()
    out = x.to(F64)
    out[G.raw_bits(x) == G.SENTINEL[dt]] = float("nan")
    return out


def test_probe_refuses_out_of_bounds_arguments(probe):
    refused = probe.cont_probe_refused_code()
    img = Image("bf16", "random", 200, 17, "finite")
    def variants():
        yield "baseline", K_FLASH, 0, img.args(), True
        yield "flash in fp32", K_FLASH, 2, img.args(), False
        p = img.args(); p.n_table = 3
        yield "fewer table entries than ceil((start + n) / 64)", K_WAVE, 0, p, False
        for bad in (-1, img.n_blocks):
            tab = (C.c_int * img.tiles)(*img.table); tab[1] = bad
            p = img.args(); p.table = C.cast(tab, C.POINTER(C.c_int))
            yield f"table entry {bad} outside the pool", K_WAVE, 0, p, False
        p = img.args(); p.qkv_rows = 16
        yield "more rows than the buffers hold", K_WAVE, 0, p, False
        p = img.args(); p.start = -1
        yield "negative start", K_WAVE, 0, p, False
        p = img.args(S=2); p.ws_floats -= 1
        yield "a workspace one float short", K_FLASH, 0, p, False
        p = img.args(); p.S = 17
        yield "17 splits", K_FLASH, 0, p, False
        p = img.args(); p.S = 2
        yield "splits without a workspace", K_FLASH, 0, p, False
        p = img.args(); p.S = 1
        yield "a merge of one split", K_MERGE, 0, p, False
        yield "norm kernel without gains and tables", K_NORM, 0, img.args(), False
    for name, kind, te, p, ok in variants():
        assert probe.cont_probe_admits(kind, te, C.byref(p)) == int(ok), name
        if not ok:
            assert probe.cont_probe_run(kind, te, C.byref(p), None) == refused, name
    assert is_sentinel(img.out, "bf16")
    img.inputs_unchanged("refused launches")


def test_split_rule_of_the_launcher(probe):
    for start, n in R.CASES:
        assert probe.cont_probe_splits(start, n, NH, n_cu(), R.WS_FLOATS) == R.splits(start, n, n_cu=n_cu()), (start, n)
    # the product shape of the issue: 128 new rows, 16 heads, behind 3968 keys: blocks x heads x S within half to one times the CUs
    S = probe.cont_probe_splits(3968, 128, 16, n_cu(), 8 << 20)
    assert n_cu() // 2 <= 2 * 16 * S <= n_cu() and (3968 + 128) // 64 // S >= R.MIN_TILES, S


def run_attention(probe, dt, kind, start, n, kernel, S, seed):
    what = f"{dt} {kind} start {start} n {n} {kernel} S {S}"
    img = Image(dt, kind, start, n, "nan" if kernel == "wave" else "finite", seed)
    if kernel == "wave":
        launch(probe, K_WAVE, dt, img.args(), what)
    else:
        p = img.args(S=S)
        launch(probe, K_FLASH, dt, p, what)
        if S > 1:
            assert is_sentinel(img.out, dt), f"{what}: the split launch wrote the output"
            assert is_sentinel(img.ws[img.ws_n:], "f32"), f"{what}: written beyond the records"
            assert not bool(torch.isnan(img.ws[:img.ws_n]).any()), f"{what}: a record was not written"
            launch(probe, K_MERGE, dt, p, what + " merge")
            assert is_sentinel(img.ws[img.ws_n:], "f32")
        SPLITS_REACHED.add(S)
    img.inputs_unchanged(what)
    o = img.out.cpu()
    assert is_sentinel(o[n:], dt), f"{what}: written beyond the new rows' output"
    ref = R.case_reference(dt, kind, start, n)
    v = R.check_attn_cont(o[:n].to(F64), ref, start, dt, kernel, S, what=what)
    assert v, v.msg
    record("prefill_attn_cont_kernel" if kernel == "wave" else ("flash_prefill_cont_kernel" + (" + merge" if S > 1 else "")), dt, v)
    return ibits(img.out[:n]).clone()


@pytest.mark.parametrize("start", R.STARTS)
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_wave_and_flash_every_start_and_n(probe, dt, start):
    for kind in R.KINDS:
        for i, n in enumerate(R.NS):
            run_attention(probe, dt, kind, start, n, "wave", 1, i)
            if dt == "bf16":
                run_attention(probe, dt, kind, start, n, "flash", R.splits(start, n, n_cu=n_cu()), i)


@pytest.mark.parametrize("start,n", R.LONG_CASES)
def test_flash_key_splits_at_longer_starts(probe, start, n):
    for kind in R.KINDS:
        S = R.splits(start, n, n_cu=n_cu())
        assert S > 1
        run_attention(probe, "bf16", kind, start, n, "flash", S, 1)
    run_attention(probe, "bf16", "which", start, n, "wave", 1, 1)
    run_attention(probe, "f32", "which", start, n, "wave", 1, 1)


@pytest.mark.parametrize("start,n,S", R.FORCED)
def test_flash_forced_split_counts_and_determinism(probe, start, n, S):
    for kind in R.KINDS:
        a = run_attention(probe, "bf16", kind, start, n, "flash", S, 2)
        b = run_attention(probe, "bf16", kind, start, n, "flash", S, 2)
        assert torch.equal(a, b), "the same launch gave other bits"


@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_norm_rope_kv_write_with_a_position_base(probe, dt):
    for i, (start, n) in enumerate(R.BASE_CASES):
        delta = R.ROPE_DELTAS[i % 3]
        what = f"{dt} norm start {start} n {n} delta {delta}"
        img = Image(dt, "random", start, n, "norm", i)
        launch(probe, K_NORM, dt, img.args(delta=delta), what)
        # bit for bit: unowned blocks, the k | v thirds and the guard rows of qkv
        owned = torch.zeros(img.n_blocks, dtype=torch.bool)
        owned[img.table] = True
        for t, t0 in ((img.K, img.K0), (img.V, img.V0)):
            assert torch.equal(ibits(t)[~owned.cuda()], t0[~owned.cuda()]), f"{what}: an unowned block changed"
        assert torch.equal(ibits(img.qkv)[:, NH:], img.qkv0[:, NH:]) and torch.equal(ibits(img.qkv)[n:], img.qkv0[n:]), f"{what}: qkv outside q"
        assert is_sentinel(img.out, dt)
        k_after, v_after = img.logical(from_dev(img.K, dt)), img.logical(from_dev(img.V, dt))
        before = torch.full_like(k_after, float("nan"))
        ref = R.norm_reference(dt, start, n, delta)
        v = R.check_norm_cont(from_dev(img.qkv, dt)[:n, :NH], k_after, v_after, before, before, ref, start, n, dt, what=what)
        assert v, v.msg
        record("qk_norm_rope_kv_cont_kernel", dt, v)


def test_zz_every_instantiation_and_split_count_was_reached(probe):
    want = {("qk_norm_rope_kv_cont_kernel", "f32"), ("qk_norm_rope_kv_cont_kernel", "bf16"), ("prefill_attn_cont_kernel", "f32"),
            ("prefill_attn_cont_kernel", "bf16"), ("flash_prefill_cont_kernel", "bf16"), ("flash_prefill_cont_kernel + merge", "bf16")}
    assert want <= set(STATS), sorted(want - set(STATS))
    reachable = {probe.cont_probe_splits(s, n, NH, n_cu(), R.WS_FLOATS) for s in range(0, 1101) for n in R.NS}
    assert reachable <= SPLITS_REACHED, sorted(reachable - SPLITS_REACHED)
    assert 1 in SPLITS_REACHED
    print()
    for (kernel, dt), st in sorted(STATS.items()):
        print(f"  {kernel:40s} {dt:5s} cases {st['cases']:4d}  largest err / bound {st['ratio']:.4f}  smallest exact fraction {st['min_exact']:.5f}")
    print(f"  split counts reached: {sorted(SPLITS_REACHED)}")
