"""Conformance of the PACKED continuation prefill kernels (qk_norm_rope_kv_cont_pack_kernel, flash_prefill_cont_pack_kernel,
flash_cont_pack_merge_kernel) with the float64 references of tests/_prefill_cont_ref.py, per sequence, and -- bit for bit -- with the
single-sequence kernels run alone through tools/microbench/libprefill_cont_probe.so.

Each kernel is launched alone through tools/microbench/libprefill_pack_cont_probe.so.  All sequences of a pack live in ONE pool with
shuffled, interleaved block ids (tests/_prefill_pack_cont_ref.py); every unowned block, every cache row the norm kernel must not touch,
the guard rows behind qkv / out and the floats behind the split records hold a NaN sentinel bit pattern and are compared bit for bit
afterwards.  The dead rows of owned blocks hold +/- 2^60 for the flash kernel (finite, per its contract).  Sequence q's V rows carry
the factor ``v_scale(q)`` and the output is divided by it before the unchanged single-sequence checker sees it.

Packs: A (five sequences around the tile edges, rope deltas cycling), B (a single sequence), C (64 sequences, the kMaxPack edge),
D (mixed split counts in one launch; forced S of 1, 3 and 5).

Observed on the MI355X (a record: no bound is tuned to it; a value stored in bf16 sits up to half an ulp from the float64 reference, so
the err / bound figures approach 1 by construction): 228 (pack, sequence) attention checks, largest err / bound 0.9899, smallest bf16
exact fraction 0.99609; every sequence of every pack bit-identical to the single-sequence kernels; no touched sentinel."""
import ctypes as C
import os

import pytest
import torch

import _attn_ref as A
import _prefill_attn_ref as P
import _prefill_cont_ref as R1
import _prefill_pack_cont_ref as R
import test_gpu_prefill_cont_reference as T1
from _attn_ref import BIG
from _prefill_attn_ref import HD, KS, N_KV
from test_gpu_attn_reference import ibits, is_sentinel, sentinel, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libprefill_pack_cont_probe.so")
F64 = torch.float64
K_NORM, K_FLASH, K_MERGE = range(3)
TE = {"bf16": 0, "f32": 2}
vp, i32, f32c = C.c_void_p, C.c_int32, C.c_float
IP = C.POINTER(C.c_int)
GUARD = 2
NH, PER = R.NH, R.NH + 2 * N_KV


class PackContProbeArgs(C.Structure):
    _fields_ = [("NH", i32), ("NKV", i32), ("n_seq", i32), ("qkv_rows", i32), ("rope_len", i32), ("n_blocks", i32), ("n_table", i32),
                ("n_cu", i32), ("ws_floats", C.c_long), ("eps", f32c), ("scale", f32c), ("qkv", vp), ("q_norm_w", vp), ("k_norm_w", vp),
                ("cos_tab", vp), ("sin_tab", vp), ("kpool", vp), ("vpool", vp), ("out", vp), ("ws", vp), ("start", IP), ("cnt", IP),
                ("rope_delta", IP), ("S", IP), ("toff", IP), ("table", IP)]


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libprefill_pack_cont_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.pack_cont_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(PackContProbeArgs), vp]
    lib.pack_cont_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(PackContProbeArgs)]
    lib.pack_cont_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.pack_cont_probe_splits.argtypes = [IP, IP, C.c_int, C.c_int, C.c_int, C.c_long, IP]
    lib.pack_cont_probe_splits.restype = C.c_long
    assert lib.pack_cont_probe_version() == 1 and lib.pack_cont_probe_kinds() == 3 and lib.pack_cont_probe_record_floats() == R.REC
    assert lib.pack_cont_probe_max_pack() == R.MAX_PACK
    buf = (C.c_long * 64)()
    n = lib.pack_cont_probe_layout(buf, 64)
    assert list(buf[:n - 1]) == [C.sizeof(PackContProbeArgs)] + [getattr(PackContProbeArgs, f[0]).offset for f in PackContProbeArgs._fields_]
    assert buf[n - 1] <= 3072                                   # the by-value descriptor stays well inside the kernel-argument segment
    return lib


@pytest.fixture(scope="module")
def single():
    """The probe of the single-sequence continuation kernels, as tests/test_gpu_prefill_cont_reference.py loads it."""
    lib = C.CDLL(T1.PROBE)
    lib.cont_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(T1.ContProbeArgs), vp]
    lib.cont_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(T1.ContProbeArgs)]
    return lib


def ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def rule(probe, pack, ws_floats=R.WS_FLOATS):
    """The launcher's splits for this device, from the probe; they must be the mirror's."""
    starts, cnts = [s for s, _ in pack], [n for _, n in pack]
    S = (C.c_int * len(pack))()
    rec = probe.pack_cont_probe_splits(ints(starts), ints(cnts), len(pack), NH, n_cu(), ws_floats, S)
    want = R.pack_splits(starts, cnts, n_cu=n_cu(), ws_floats=ws_floats)
    assert list(S) == want and rec == R.pack_ws_floats(cnts, want), (list(S), want)
    return want


class PackImage:
    """One pack in one oversized pool.  mode "finite": attention (the new rows' q, each cache filled up to start + n, dead rows of the
    last owned tile +/- 2^60); "norm": the new rows before the norm, every pool row a sentinel."""

    def __init__(self, dt, pack, mode, seed=0):
        self.dt, self.pack, self.mode, self.n = dt, pack, mode, len(pack)
        self.starts, self.cnts = [s for s, _ in pack], [n for _, n in pack]
        self.off = R.pack_offsets(self.cnts)
        self.Lt = self.off[-1]
        self.n_blocks, self.tables = R.pack_tables(pack, seed=seed)
        pools = [torch.full((self.n_blocks, N_KV, KS, HD), float("nan"), dtype=F64) for _ in range(2)]
        qkv = torch.full((self.Lt + GUARD, PER, HD), float("nan"), dtype=F64)
        self.full = []                                           # per sequence: (K, V) logical rows of its owned tiles, as stored
        for q, (start, n) in enumerate(pack):
            L, tiles, o = start + n, len(self.tables[q]), self.off[q]
            if mode == "norm":
                qkv[o:o + n] = R1.norm_input(dt, L)[start:]
                continue
            qq, K, V = R1.operands(dt, R.kind_of(q), start, n)
            qkv[o:o + n, :NH] = qq[start:]
            r = torch.arange(KS * tiles)
            sign = 1.0 - 2.0 * ((r[:, None] + torch.arange(HD)[None, :]) % 2).to(F64)
            fulls = []
            for pool, X, f in zip(pools, (K, V), (1.0, R.v_scale(q))):
                full = torch.full((N_KV, KS * tiles, HD), float("nan"), dtype=F64)
                full[:, :L] = X * f
                full[:, L:] = (BIG * sign)[L:]
                for t in range(tiles):
                    pool[self.tables[q][t]] = full[:, t * KS:(t + 1) * KS]
                fulls.append(full)
            self.full.append(fulls)
        self.K, self.V, self.qkv = to_dev(pools[0], dt), to_dev(pools[1], dt), to_dev(qkv, dt)
        self.K0, self.V0, self.qkv0 = ibits(self.K).clone(), ibits(self.V).clone(), ibits(self.qkv).clone()
        self.out = sentinel((self.Lt + GUARD, NH, HD), dt)
        flat = [b for t in self.tables for b in t]
        toff = [0]
        for t in self.tables:
            toff.append(toff[-1] + len(t))
        self.keep = dict(start=ints(self.starts), cnt=ints(self.cnts), toff=ints(toff), table=ints(flat))
        self.n_table = len(flat)
        self.ws, self.ws_n = None, 0

    def args(self, S=None, deltas=None, ws_floats=R.WS_FLOATS):
        p = PackContProbeArgs()
        p.NH, p.NKV, p.n_seq, p.qkv_rows, p.rope_len = NH, N_KV, self.n, self.Lt, R1.ROPE_LEN
        p.n_blocks, p.n_table, p.n_cu, p.eps, p.scale = self.n_blocks, self.n_table, n_cu(), P.EPS, P.SCALE
        p.qkv, p.out, p.kpool, p.vpool = self.qkv.data_ptr(), self.out.data_ptr(), self.K.data_ptr(), self.V.data_ptr()
        for k in ("start", "cnt", "toff", "table"):
            setattr(p, k, C.cast(self.keep[k], IP))
        self.keep["delta"] = ints(deltas if deltas is not None else [0] * self.n)
        p.rope_delta = C.cast(self.keep["delta"], IP)
        if S is not None:
            self.keep["S"] = ints(S)
            p.S = C.cast(self.keep["S"], IP)
        if self.mode == "norm":
            qw, kw = A.base_gains(self.dt, "random")
            ct, st = P.rope_table(R1.ROPE_LEN)
            self.keep["norm"] = (to_dev(qw, self.dt), to_dev(kw, self.dt), ct.to(torch.float32).cuda(), st.to(torch.float32).cuda())
            p.q_norm_w, p.k_norm_w, p.cos_tab, p.sin_tab = (t.data_ptr() for t in self.keep["norm"])
        else:
            Sv = S if S is not None else R.pack_splits(self.starts, self.cnts, n_cu=n_cu(), ws_floats=ws_floats)
            self.ws_n = R.pack_ws_floats(self.cnts, Sv)
            # forced splits: a workspace of exactly the records; the launcher's rule: the workspace the rule is told about
            size = self.ws_n if S is not None else ws_floats
            self.ws = sentinel((size + 64,), "f32")
            p.ws, p.ws_floats = self.ws.data_ptr(), size
        return p

    def inputs_unchanged(self, what):
        for t, t0, name in ((self.K, self.K0, "K pool"), (self.V, self.V0, "V pool"), (self.qkv, self.qkv0, "qkv")):
            assert torch.equal(ibits(t), t0), f"{what}: the {name} changed"

    def logical(self, pool, q):
        return torch.cat([pool[b] for b in self.tables[q]], dim=1)


def launch(probe, kind, dt, p, what):
    assert probe.pack_cont_probe_admits(kind, TE[dt], C.byref(p)) == 1, f"{what}: the probe refuses kind {kind}"
    rc = probe.pack_cont_probe_run(kind, TE[dt], C.byref(p), None)
    assert rc == 0, f"{what}: kind {kind} returned {rc}"


def run_pack_attention(probe, pack, S, seed=0, forced=True, what=""):
    """Flash launch (+ merge launch when a sequence splits) of the whole pack; every sequence held to its own bound.  Returns the
    image and the output bits."""
    img = PackImage("bf16", pack, "finite", seed)
    p = img.args(S=S if forced else None)
    launch(probe, K_FLASH, "bf16", p, what)
    assert is_sentinel(img.ws[img.ws_n:], "f32"), f"{what}: written beyond the records"
    assert not bool(torch.isnan(img.ws[:img.ws_n]).any()), f"{what}: a record was not written"
    for q, s in enumerate(S):
        rows = img.out[img.off[q]:img.off[q + 1]]
        assert is_sentinel(rows, "bf16") == (s > 1), f"{what}: sequence {q} (S {s}) after the flash launch"
    if any(s > 1 for s in S):
        launch(probe, K_MERGE, "bf16", p, what + " merge")
        assert is_sentinel(img.ws[img.ws_n:], "f32")
    img.inputs_unchanged(what)
    o = img.out.cpu()
    assert is_sentinel(o[img.Lt:], "bf16"), f"{what}: written beyond the pack's output rows"
    for q, (start, n) in enumerate(pack):
        ref = R.case_reference("bf16", R.kind_of(q), start, n)
        got = o[img.off[q]:img.off[q + 1]].to(F64) / R.v_scale(q)
        w = f"{what} sequence {q} (start {start}, n {n}, S {S[q]})"
        v = R.check_attn_cont(got, ref, start, "bf16", "flash", S[q], what=w)
        print(f"  {w}: err / bound {v.ratio:.4f}, exact fraction {v.exact:.5f}")
        assert v, v.msg
    return img, ibits(img.out[:img.Lt]).clone()


def single_attention(single, img, q, S):
    """Sequence q of the pack image through flash_prefill_cont_kernel (+ merge) alone, on the same stored values."""
    start, n = img.pack[q]
    one = T1.Image("bf16", R.kind_of(q), start, n, "finite", seed=q)
    for pool, full in zip((one.K, one.V), img.full[q]):
        for t in range(one.tiles):
            pool[one.table[t]] = to_dev(full[:, t * KS:(t + 1) * KS], "bf16")
    assert torch.equal(ibits(one.qkv[:n, :NH]), ibits(img.qkv[img.off[q]:img.off[q] + n, :NH]))
    p = one.args(S=S)
    for kind in (T1.K_FLASH,) + ((T1.K_MERGE,) if S > 1 else ()):
        assert single.cont_probe_run(kind, 0, C.byref(p), None) == 0
    return ibits(one.out[:n]).clone()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_probe_refuses_out_of_bounds_arguments(probe):
    refused = probe.pack_cont_probe_refused_code()
    img = PackImage("bf16", R.PACK_D, "finite")
    S = [3, 4, 1]
    def variants():
        yield "baseline", K_FLASH, 0, img.args(S=S), True
        yield "flash in fp32", K_FLASH, 2, img.args(S=S), False
        p = img.args(S=S); p.start = C.cast(ints([704, -1, 0]), IP)
        yield "a negative start", K_FLASH, 0, p, False
        p = img.args(S=S); p.cnt = C.cast(ints([64, 0, 130]), IP)
        yield "cnt 0", K_FLASH, 0, p, False
        p = img.args(S=S); p.n_seq = 65
        yield "65 sequences", K_FLASH, 0, p, False
        toff = list(img.keep["toff"]); toff[2] -= 8; toff[3] -= 8
        p = img.args(S=S); p.toff = C.cast(ints(toff), IP)
        yield "a table short of start", K_FLASH, 0, p, False
        p = img.args(S=S); p.ws_floats = img.ws_n - 1
        yield "records beyond the workspace", K_FLASH, 0, p, False
        p = img.args(S=S); p.ws_floats = img.ws_n - 1
        yield "a merge of records beyond the workspace", K_MERGE, 0, p, False
        p = img.args(S=[3, 17, 1])
        yield "17 splits", K_FLASH, 0, p, False
        p = img.args(S=S); p.qkv_rows = img.Lt - 1
        yield "more rows than the buffers hold", K_FLASH, 0, p, False
        tab = list(img.keep["table"]); tab[5] = img.n_blocks
        p = img.args(S=S); p.table = C.cast(ints(tab), IP)
        yield "a table entry outside the pool", K_FLASH, 0, p, False
        yield "norm kernel without gains and tables", K_NORM, 0, img.args(S=S), False
    keep = []
    for name, kind, te, p, ok in variants():
        keep.append(p)
        assert probe.pack_cont_probe_admits(kind, te, C.byref(p)) == int(ok), name
        if not ok:
            assert probe.pack_cont_probe_run(kind, te, C.byref(p), None) == refused, name
    assert is_sentinel(img.out, "bf16")
    img.inputs_unchanged("refused launches")


def test_split_rule_of_the_launcher(probe):
    for start, n in R1.CASES:
        assert rule(probe, [(start, n)]) == [R1.splits(start, n, n_cu=n_cu())], (start, n)
    for name, pack in R.PACKS.items():
        S = rule(probe, pack)
        assert all(s == 1 or R.tiles_of(st, n) // s >= R.MIN_TILES for s, (st, n) in zip(S, pack)), name
    rule(probe, R.PACK_D, ws_floats=64 * NH * R.REC * 3)                 # the shrink loop
    assert len(set(rule(probe, R.PACK_D))) > 1


# ---- attention -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.PACKS))
def test_flash_pack_bounds_and_bit_identity_with_the_single_kernel(probe, single, name):
    """S[] forced to each sequence's single-kernel splits(start, n): every sequence within its bound, and its output the bits of
    flash_prefill_cont_kernel (+ merge) run alone.  The same call twice gives the same bits."""
    pack = R.PACKS[name]
    S = [R1.splits(s, n, n_cu=n_cu()) for s, n in pack]
    img, bits = run_pack_attention(probe, pack, S, what=f"pack {name} forced {S}")
    _img2, again = run_pack_attention(probe, pack, S, what=f"pack {name} again")
    assert torch.equal(bits, again), "the same call gave other bits"
    for q, (start, n) in enumerate(pack):
        alone = single_attention(single, img, q, S[q])
        assert torch.equal(bits[img.off[q]:img.off[q + 1]], alone), f"pack {name} sequence {q} (start {start}, n {n}, S {S[q]}): not the single kernel's bits"


@pytest.mark.parametrize("name", sorted(R.PACKS))
def test_flash_pack_through_the_launchers_rule(probe, single, name):
    pack = R.PACKS[name]
    S = rule(probe, pack)
    img, bits = run_pack_attention(probe, pack, S, seed=1, forced=False, what=f"pack {name} rule {S}")
    if name == "B":                                              # a pack of one through the rule: the single kernel, bit for bit
        start, n = pack[0]
        assert S == [R1.splits(start, n, n_cu=n_cu())]
        assert torch.equal(bits, single_attention(single, img, 0, S[0]))


@pytest.mark.parametrize("S", R.FORCED_D)
def test_flash_pack_forced_splits_on_pack_d(probe, S):
    run_pack_attention(probe, R.PACK_D, [S] * len(R.PACK_D), seed=2, what=f"pack D forced S {S}")


# ---- norm + RoPE + K/V write -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.PACKS))
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_norm_rope_kv_write_of_the_pack(probe, single, dt, name):
    pack = R.PACKS[name]
    deltas = [R.ROPE_DELTAS[q % 3] for q in range(len(pack))]
    what = f"{dt} norm pack {name}"
    img = PackImage(dt, pack, "norm", seed=3)
    launch(probe, K_NORM, dt, img.args(deltas=deltas), what)
    owned = torch.zeros(img.n_blocks, dtype=torch.bool)
    owned[[b for t in img.tables for b in t]] = True
    for t, t0 in ((img.K, img.K0), (img.V, img.V0)):
        assert torch.equal(ibits(t)[~owned.cuda()], t0[~owned.cuda()]), f"{what}: an unowned block changed"
    assert torch.equal(ibits(img.qkv)[:, NH:], img.qkv0[:, NH:]) and torch.equal(ibits(img.qkv)[img.Lt:], img.qkv0[img.Lt:]), f"{what}: qkv outside q"
    assert is_sentinel(img.out, dt)
    Kf, Vf, qf = T1.from_dev(img.K, dt), T1.from_dev(img.V, dt), T1.from_dev(img.qkv, dt)
    seen = set()
    for q, (start, n) in enumerate(pack):
        # every sequence against float64: its new rows within the bound, every other row of its blocks still the sentinel -- so no
        # other sequence wrote into them
        k_after, v_after = img.logical(Kf, q), img.logical(Vf, q)
        before = torch.full_like(k_after, float("nan"))
        ref = R1.norm_reference(dt, start, n, deltas[q])
        v = R.check_norm_cont(qf[img.off[q]:img.off[q + 1], :NH], k_after, v_after, before, before, ref, start, n, dt,
                              what=f"{what} sequence {q} (start {start}, n {n}, delta {deltas[q]})")
        assert v, v.msg
        if (start, n, deltas[q]) in seen:
            continue
        seen.add((start, n, deltas[q]))
        # bit identity with qk_norm_rope_kv_cont_kernel run alone
        one = T1.Image(dt, "random", start, n, "norm", q)
        p = one.args(delta=deltas[q])
        assert single.cont_probe_run(T1.K_NORM, TE[dt], C.byref(p), None) == 0
        assert torch.equal(ibits(one.qkv[:n, :NH]), ibits(img.qkv[img.off[q]:img.off[q + 1], :NH])), f"{what} sequence {q}: q bits"
        for a, b in ((one.K, img.K), (one.V, img.V)):
            mine = torch.cat([ibits(b)[blk] for blk in img.tables[q]], dim=1)[:, start:start + n]
            theirs = one.logical(ibits(a))[:, start:start + n]
            assert torch.equal(mine, theirs), f"{what} sequence {q}: K / V bits"
