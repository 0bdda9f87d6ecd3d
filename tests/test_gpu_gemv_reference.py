"""Conformance of every decode GEMV kernel with the float64 reference of tests/_gemv_ref.py.

Each launch goes alone through tools/microbench/libgemv_probe.so.  Operands are seeded, wide-range and partly cancelling; the output
and xn_out images are sentinel-filled with guard rows and a leading dimension wider than the row; token rows >= B, weight rows >= N
(row-major) and between the gate and the up half, x / gain beyond K, bias beyond N and partial slots >= n_part hold the NaN sentinel:
the kernels clamp instead of reading them, so a NaN in an output is a finding, and every element outside [0, B) x [0, N) must keep the
sentinel.  Bit identities asserted: gemv_kernel NT = true / false, R = 1 / 2, xn_out set / null, res aliasing y; gemv_batch_kernel
every group and every token against gemv_kernel on that token alone; the matrix-core kernels NT = n / NT = 0, DUAL / one panel,
fragment-major Wp / row-major, res aliasing y; the norm kernel's xn_out rows against rmsnorm_batch_kernel's rows.

The last test prints the per-family record and asserts that every instantiation the probe builds was launched.
Observed on the MI355X (a record: nothing is tuned to it; a value stored in bf16 sits up to half an ulp from the float64 reference, so
the bf16 err / bound figures approach 0.5 by construction -- the fp32 figures and the bf16 exact fraction carry the information).
Exact fraction: over the scored rows; "per case" = the smallest of the cases of MIN_SCORED scored elements or more, "pooled" = the
elements of the smaller cases together (tests/_gemv_ref.py); both must reach 0.99:
  kernel                          type  cases checked  launches  largest err / bound  exact per case   exact pooled
  gemv_kernel                     fp32       625         2093        0.113               -                -
  gemv_kernel                     bf16       625         2093        0.498             0.99870          1260 of 1260
  gemv_batch_kernel               fp32        88          268        0.072               -                -
  gemv_batch_kernel               bf16        88          270        0.447             0.99968          1642 of 1642
  gemv_batch_mfma_norm_kernel     bf16       104          578        0.499             0.99851          8288 of 8288
  gemv_batch_mfma_plain_kernel    bf16       208          754        0.499             0.99806          26682 of 26684
  rmsnorm_batch_kernel            bf16         5          114        bit-exact            -                -
  Largest error in ulps of the reference: 12 (gemv_kernel bf16), 5 (gemv_batch_kernel bf16), 191 (norm kernel), 18 (plain kernel), all on
  the nearly cancelling rows, where the bound is c S; fp32 8.0e5 / 5.8e5 fp32 ulps on the same rows (0.11 / 0.07 of the bound).
  Every bf16 xn_out row (NORM, COMBINE, PLAIN) was bit-exact; every asserted bit identity held.
  Instantiations launched: gemv_kernel 212 of 212, gemv_batch_kernel 32 of 32, rmsnorm_batch_kernel 2 of 2,
  gemv_batch_mfma_norm_kernel 64 of 64, gemv_batch_mfma_plain_kernel 80 of 80.
No case found a defect in device code: no NaN, no touched sentinel, no element outside its bound.  The defect found by reading -- the
PRO_COMBINE prologue stages only the first 2048 elements of K = q_dim -- is closed by the guard (fq3_ctx_create and the probe refuse
q_dim > 2048; tests/test_abi.py, test_probe_refuses_what_would_leave_the_buffers); that configuration is never launched here.
"""
import ctypes as C
import os
from collections import defaultdict

import pytest
import torch

import _gemm_ref as G
import _gemv_ref as R
from _gemv_ref import EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, PRO_COMBINE, PRO_NORM, PRO_PLAIN, F64
from test_gpu_attn_reference import ibits, sentinel, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libgemv_probe.so")
K_GEMV, K_BATCH, K_RMSNORM, K_MFMA_NORM, K_MFMA_PLAIN = range(5)
KIND_NAME = ("gemv_kernel", "gemv_batch_kernel", "rmsnorm_batch_kernel", "gemv_batch_mfma_norm_kernel", "gemv_batch_mfma_plain_kernel")
TE = {"bf16": 0, "f32": 2}
ESZ = {"bf16": 2, "f32": 4}
vp, i32, f32c = C.c_void_p, C.c_int32, C.c_float
GUARD, PAD = 2, 8
REFUSED = 100000


class GemvProbeArgs(C.Structure):
    _fields_ = [("N", i32), ("K", i32), ("B", i32), ("pro", i32), ("epi", i32), ("nt", i32), ("rows", i32), ("group", i32), ("dual", i32),
                ("ntiles", i32), ("up_off", i32), ("n_part", i32), ("rep", i32), ("x_stride", i32), ("y_stride", i32), ("res_stride", i32),
                ("xn_stride", i32), ("part_stride", C.c_long), ("eps", f32c), ("W", vp), ("Wp", vp), ("x", vp), ("norm_w", vp), ("bias", vp),
                ("y", vp), ("res", vp), ("xn_out", vp), ("part", vp)]


STATS = defaultdict(lambda: {"cases": 0, "launches": 0, "ulp": 0.0, "ratio": 0.0, "min_exact": 1.0, "pool": R.ExactPool()})
REACHED = defaultdict(set)          # kind -> instantiation ids launched


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libgemv_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.gemv_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(GemvProbeArgs), vp]
    lib.gemv_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(GemvProbeArgs)]
    lib.gemv_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.gemv_probe_pack.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.gemv_probe_most_chunks.argtypes = [C.c_int, C.c_int]
    assert all(lib.gemv_probe_most_chunks(pro, m) == R.most_nch(pro, m) for pro in (PRO_PLAIN, PRO_NORM, PRO_COMBINE) for m in (1, 2))
    assert lib.gemv_probe_version() == 1 and lib.gemv_probe_kinds() == 5 and lib.gemv_probe_refused_code() == REFUSED
    buf = (C.c_long * 64)()
    n = lib.gemv_probe_layout(buf, 64)
    want = [C.sizeof(GemvProbeArgs)] + [getattr(GemvProbeArgs, f[0]).offset for f in GemvProbeArgs._fields_]
    assert list(buf[:n - 6]) == want, "ctypes mirror of GemvProbeArgs is out of date"
    assert list(buf[n - 6:n]) == [R.MAX_LANES, R.TOK_TILE, 8, R.COMBINE_MAX_K, R.MAX_WORKERS, R.PART_STRIDE]
    return lib


def values(t, dt):
    """A device storage tensor as float64 with NaN for the untouched sentinel and inf for any other NaN."""
    cpu = t.cpu()
    v = cpu.to(F64)
    sent = G.raw_bits(cpu) == G.SENTINEL[dt]
    v[torch.isnan(v) & ~sent] = float("inf")
    return v


def padded(x, rows, cols):
    """x [r][c] float64 -> [rows][cols] with NaN around it."""
    out = torch.full((rows, cols), float("nan"), dtype=F64)
    out[:x.shape[0], :x.shape[1]] = x
    return out


class Dev:
    """The device image of a case: every operand with NaN guards, the strides the launches use."""

    def __init__(self, c: R.Case):
        R.build(c)
        self.c, dt = c, c.dt
        self.esz = ESZ[dt]
        B, N, K = c.B, c.N, c.K
        self.xs, self.ys = K + PAD, N + 3
        self.x = to_dev(padded(c.x, B + GUARD, self.xs), dt) if c.x is not None else None
        self.W = to_dev(padded(c.W, c.n_rows + GUARD, K), dt) if c.W is not None else None
        self.gain = to_dev(padded(c.gain[None], 1, K + PAD), dt) if c.gain is not None else None
        self.bias = to_dev(padded(c.bias_v[None], 1, N + PAD), dt) if c.bias_v is not None else None
        self.res = to_dev(padded(c.res, B + GUARD, self.ys), dt) if c.res is not None else None
        self.part = None
        if c.slots is not None:
            self.part_elems = c.slots[0].numel()
            self.part = to_dev(padded(c.slots.reshape(B, -1), B, self.part_elems + 4), "f32")
        self.Wp = None
        self.inputs = [t for t in (self.x, self.W, self.gain, self.bias, self.res, self.part) if t is not None]
        self.inputs0 = [ibits(t).clone() for t in self.inputs]

    def pack(self, probe):
        if self.Wp is None:
            n = self.c.n_rows
            clean = torch.nan_to_num(self.W[:n].float(), nan=0.0).to(torch.bfloat16).contiguous()      # (the gap rows of a SwiGLU matrix: zeros)
            self.Wp = torch.empty_like(clean)
            assert probe.gemv_probe_pack(clean.data_ptr(), self.Wp.data_ptr(), n, self.c.K, None) == 0
        return self.Wp

    def args(self, B, tok0=0):
        c, p = self.c, GemvProbeArgs()
        p.N, p.K, p.B, p.pro, p.epi, p.up_off, p.n_part, p.rep, p.eps = c.N, c.K, B, c.pro, c.epi, c.up_off, c.n_part, c.rep, R.EPS
        p.x_stride, p.y_stride, p.res_stride, p.xn_stride = self.xs, self.ys, self.ys, self.xs
        p.W = self.W.data_ptr() if self.W is not None else None
        p.x = self.x.data_ptr() + tok0 * self.xs * self.esz if self.x is not None else None
        p.norm_w = self.gain.data_ptr() if self.gain is not None else None
        p.bias = self.bias.data_ptr() if self.bias is not None else None
        p.res = self.res.data_ptr() + tok0 * self.ys * self.esz if self.res is not None else None
        if self.part is not None:
            p.part_stride = self.part_elems + 4
            p.part = self.part.data_ptr() + tok0 * p.part_stride * 4
        self.tok0 = tok0
        return p

    def unchanged(self, what):
        for t, t0 in zip(self.inputs, self.inputs0):
            assert torch.equal(ibits(t), t0), f"{what}: a launch wrote one of its inputs"


def launch(probe, kind, d: Dev, p, what, *, xn=True, alias=False):
    """One launch on fresh sentinel outputs; returns (y image [B + GUARD][ys] float64, xn image or None, y bits)."""
    c, dt, B = d.c, d.c.dt, p.B
    ycols = d.xs if kind == K_RMSNORM else d.ys
    y = sentinel((B + GUARD, ycols), dt)
    if alias:                                                   # the residual lives in the output buffer
        y[:B] = d.res[d.tok0:d.tok0 + B]
        p.res = y.data_ptr()
    xo = sentinel((B + GUARD, d.xs), dt) if xn else None
    p.y, p.xn_out = y.data_ptr(), (xo.data_ptr() if xn else None)
    if kind == K_RMSNORM:
        p.y_stride = d.xs
    assert probe.gemv_probe_admits(kind, TE[dt], C.byref(p)) == 1, f"{what}: the probe refuses the launch"
    rc = probe.gemv_probe_run(kind, TE[dt], C.byref(p), None)
    assert rc == 0, f"{what}: the probe returned {rc}"
    REACHED[kind].add(probe.gemv_probe_last_inst())
    STATS[KIND_NAME[kind], dt]["launches"] += 1
    return values(y, dt), (values(xo, dt) if xn else None), ibits(y).cpu()


def verify(kind, d: Dev, ref, img, xo, what, pool, *, rows=None, xn_tokens=None):
    """The image against the reference: stray writes, NaN, bounds, exact fraction (a case too small for it goes to `pool`); the
    xn_out image (its first xn_tokens rows) likewise."""
    c = d.c
    B = img.shape[0] - GUARD
    ncols = c.K if kind == K_RMSNORM else c.N
    msg = R.check_image(img, B, ncols, what)
    assert msg == "", msg
    st = STATS[KIND_NAME[kind], c.dt]
    if kind == K_RMSNORM:
        v = R.check_xn(img[:B, :ncols], ref, c, what, rows=rows)
    else:
        v = R.check_y(img[:B, :ncols], ref, c, what, rows=rows)
        pool.add(v)
        st["pool"].add(v)
        if v.n_scored >= R.MIN_SCORED:
            st["min_exact"] = min(st["min_exact"], v.exact)
    assert v.ok, v.msg
    st["cases"] += 1
    st["ulp"] = max(st["ulp"], v.max_ulp)                         # in ulps of the reference, both checkers
    st["ratio"] = max(st["ratio"], v.ratio)
    if xo is not None:
        nx = xo.shape[0] - GUARD if xn_tokens is None else xn_tokens
        msg = R.check_image(xo, nx, c.K, what + " xn_out")
        assert msg == "", msg
        vx = R.check_xn(xo[:nx, :c.K], ref, c, what, rows=(rows if xn_tokens is None else slice(0, xn_tokens)))
        assert vx.ok, vx.msg


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_probe_refuses_what_would_leave_the_buffers(probe):
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    ptr = buf.data_ptr()

    def base(kind, pro=PRO_PLAIN, epi=EPI_STORE, N=16, K=256, B=17):
        p = GemvProbeArgs()
        p.N, p.K, p.B, p.pro, p.epi, p.eps = N, K, B, pro, epi, R.EPS
        p.x_stride = p.xn_stride = K
        p.y_stride = p.res_stride = N
        p.W = p.x = p.norm_w = p.y = p.res = ptr
        if kind in (K_MFMA_NORM, K_MFMA_PLAIN):
            p.nt = (B + 15) // 16 if B <= 64 else 0
            p.ntiles = (B + 15) // 16
        if kind == K_GEMV:
            p.B = min(B, 2)
        if epi == EPI_SWIGLU:
            p.up_off = N
        if kind == K_RMSNORM:
            p.y_stride = K
        if pro == PRO_COMBINE:
            p.part, p.n_part, p.rep, p.part_stride = ptr, 3, 1, (K // 128) * 8 * 132
        return p

    def admits(kind, p, dt="bf16"):
        a = probe.gemv_probe_admits(kind, TE[dt], C.byref(p))
        if not a:
            assert probe.gemv_probe_run(kind, TE[dt], C.byref(p), None) == REFUSED       # nothing is launched
        return a

    kinds = ((K_GEMV, PRO_PLAIN, EPI_RESIDUAL), (K_BATCH, PRO_NORM, EPI_STORE), (K_MFMA_NORM, PRO_NORM, EPI_STORE),
             (K_MFMA_PLAIN, PRO_PLAIN, EPI_RESIDUAL), (K_RMSNORM, PRO_NORM, EPI_STORE))
    for kind, pro, epi in kinds:
        assert admits(kind, base(kind, pro, epi)) == 1
        for field, bad in (("K", 260), ("K", 0), ("N", 0), ("B", 0), ("x_stride", 255), ("y_stride", 15 if kind != K_RMSNORM else 255), ("y", None), ("x", None)):
            p = base(kind, pro, epi)
            setattr(p, field, bad)
            assert admits(kind, p) == 0, f"kind {kind}: {field} = {bad} admitted"
        if epi == EPI_RESIDUAL:
            p = base(kind, pro, epi)
            p.res_stride = 15
            assert admits(kind, p) == 0
            p = base(kind, pro, epi)
            p.res = None
            assert admits(kind, p) == 0
        p = base(kind, pro, epi)
        p.xn_out, p.xn_stride = ptr, 248
        assert admits(kind, p) == 0
    # the fragment-major copy needs whole 16-row blocks; SwiGLU an up half that starts on one
    for kind, pro, epi in ((K_MFMA_NORM, PRO_NORM, EPI_STORE), (K_MFMA_PLAIN, PRO_PLAIN, EPI_STORE)):
        p = base(kind, pro, epi, N=24)
        assert admits(kind, p) == 1
        p.Wp = ptr
        assert admits(kind, p) == 0
    p = base(K_MFMA_NORM, PRO_NORM, EPI_SWIGLU)
    p.Wp = ptr
    assert admits(K_MFMA_NORM, p) == 1
    p.up_off = 24
    assert admits(K_MFMA_NORM, p) == 0
    p.Wp, p.up_off = None, 8
    assert admits(K_MFMA_NORM, p) == 0                           # an up half inside the gate rows
    # tile counts that do not cover B exactly
    for kind, pro in ((K_MFMA_NORM, PRO_NORM), (K_MFMA_PLAIN, PRO_PLAIN)):
        for nt, ntiles in ((1, 2), (3, 2), (0, 1), (0, 3)):
            p = base(kind, pro)
            p.nt, p.ntiles = nt, ntiles
            assert admits(kind, p) == 0, (kind, nt, ntiles)
        p = base(kind, pro, K=384)
        assert admits(kind, p) == 0                              # not a built K
        p = base(kind, pro)
        assert admits(kind, p, "f32") == 0
    p = base(K_MFMA_NORM, PRO_NORM, B=16)
    p.dual = 1
    assert admits(K_MFMA_NORM, p) == 0                           # the two-panel form loads a second tile's tokens
    p = base(K_MFMA_NORM, PRO_NORM, K=2048, B=17)
    p.dual = 1
    assert admits(K_MFMA_NORM, p) == 0                           # not built
    # VALU batch: group over the LDS budget / the group maximum / B
    p = base(K_BATCH, PRO_PLAIN, K=6144, B=17)
    p.x_stride = 6144
    for dt, g, ok in (("f32", 4, 1), ("f32", 5, 0), ("f32", 8, 0), ("bf16", 8, 1), ("bf16", 9, 0)):
        p.group = g
        assert admits(K_BATCH, p, dt) == ok, (dt, g)
    p = base(K_BATCH, PRO_PLAIN, K=256, B=3)
    p.group = 4
    assert admits(K_BATCH, p) == 0
    p = base(K_BATCH, PRO_NORM, K=2056)
    p.x_stride = 2056
    assert admits(K_BATCH, p) == 0                               # a normalising GEMV reads K <= 2048
    # gemv_kernel: the split-KV merge stages K <= 2048 in whole heads; two tokens need their own slots
    for K, ok in ((2048, 1), (2176, 0), (3072, 0), (192, 0)):
        p = base(K_GEMV, PRO_COMBINE, EPI_RESIDUAL, K=K, B=1)
        assert admits(K_GEMV, p) == ok, K
    p = base(K_GEMV, PRO_COMBINE, EPI_RESIDUAL, K=1024, B=2)
    assert admits(K_GEMV, p) == 1
    p.part_stride -= 1
    assert admits(K_GEMV, p) == 0
    for field, bad in (("n_part", 0), ("n_part", 9), ("rep", 3), ("part", None)):
        p = base(K_GEMV, PRO_COMBINE, EPI_RESIDUAL, K=1024, B=1)
        setattr(p, field, bad)
        assert admits(K_GEMV, p) == 0, field
    p = base(K_GEMV, PRO_PLAIN, EPI_STORE, K=3080, B=2)
    p.x_stride = 3080
    assert admits(K_GEMV, p) == 0                                # a two-token pass holds K <= 3072
    p = base(K_GEMV, PRO_PLAIN, EPI_STORE, B=2)
    p.nt = 1
    assert admits(K_GEMV, p) == 0
    p = base(K_GEMV, PRO_NORM, EPI_RESIDUAL)
    assert admits(K_GEMV, p) == 0                                # not a pair the product launches


# ---- gemv_kernel ---------------------------------------------------------------------------------------------------------------------
def gemv_token(probe, d, t, *, nt=0, rows=0, xn=True, alias=False, what=""):
    p = d.args(1, t)
    p.nt, p.rows = nt, rows
    return launch(probe, K_GEMV, d, p, what, xn=xn, alias=alias)


@pytest.mark.parametrize("pro,epi", R.PAIRS, ids=[R.PAIR_NAME[p] for p in R.PAIRS])
@pytest.mark.parametrize("dt", R.DTS)
def test_gemv_kernel(probe, dt, pro, epi):
    pool = R.ExactPool()
    for c in R.gemv_cases(dt, pro, epi):
        d, ref = Dev(c), R.reference(c)
        what = c.name
        bits = []
        for t in range(c.B):
            img, xo, b0 = gemv_token(probe, d, t, what=f"{what} token {t}")
            verify(K_GEMV, d, ref, img, xo, f"{what} token {t}", pool, rows=slice(t, t + 1))
            bits.append(b0)
            variants = [dict(nt=1), dict(xn=False)] + ([dict(rows=1), dict(rows=1, nt=1)] if c.N > 1024 else [])
            if epi == EPI_RESIDUAL:
                variants.append(dict(alias=True))
            for kw in variants if t == 0 else variants[:1]:
                _, _, b1 = gemv_token(probe, d, t, what=f"{what} {kw}", **kw)
                assert torch.equal(b1, b0), f"{what} token {t}: {kw} changed the output bits"
        if R.gemv_chunks(c.K, R.most_nch(pro, 2)):
            for rows in ((0, 1) if c.N > 1024 else (0,)):
                p = d.args(2)
                p.rows = rows
                img, xo, _ = launch(probe, K_GEMV, d, p, f"{what} M=2 rows={rows}")
                verify(K_GEMV, d, ref, img, xo, f"{what} M=2 rows={rows}", pool, xn_tokens=1)       # (xn_out holds token 0 only)
        d.unchanged(what)
    pool.check(f"gemv_kernel {dt} {R.PAIR_NAME[(pro, epi)]}")


# ---- gemv_batch_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pro,epi", R.PAIRS[:4], ids=[R.PAIR_NAME[p] for p in R.PAIRS[:4]])
@pytest.mark.parametrize("dt", R.DTS)
def test_gemv_batch_kernel(probe, dt, pro, epi):
    pool = R.ExactPool()
    for c in R.batch_cases(dt, pro, epi):
        d, ref = Dev(c), R.reference(c)
        what = c.name
        p = d.args(c.B)
        img, xo, b0 = launch(probe, K_BATCH, d, p, what)
        verify(K_BATCH, d, ref, img, xo, what, pool)
        for kw in ([dict(group=c.group)] if c.group else []) + [dict(xn=False)] + ([dict(alias=True)] if epi == EPI_RESIDUAL else []):
            p = d.args(c.B)
            p.group = kw.get("group", 0)
            _, _, b1 = launch(probe, K_BATCH, d, p, f"{what} {kw}", xn=kw.get("xn", True), alias=kw.get("alias", False))
            assert torch.equal(b1[:c.B, :c.N], b0[:c.B, :c.N]), f"{what}: {kw} changed the output bits"
        for t in range(c.B):                                     # the header's promise: each token as gemv_kernel computes it alone
            _, _, bt = gemv_token(probe, d, t, what=f"{what} gemv_kernel token {t}")
            assert torch.equal(bt[0, :c.N], b0[t, :c.N]), f"{what}: token {t} differs from gemv_kernel on that token alone"
        d.unchanged(what)
    pool.check(f"gemv_batch_kernel {dt} {R.PAIR_NAME[(pro, epi)]}")


# ---- the matrix-core kernels -----------------------------------------------------------------------------------------------------------
def tile_variants(c, kind):
    need = (c.B + 15) // 16
    nts = ([need] if need <= 4 else []) + [0]
    out = []
    for nt in nts:
        for wp in ((False, True) if c.N % 16 == 0 else (False,)):
            out.append(dict(nt=nt, wp=wp, dual=0))
            if kind == K_MFMA_NORM and c.K <= 1024 and c.B > 16 and nt != 1:
                out.append(dict(nt=nt, wp=wp, dual=1))
    return out


def mfma_launch(probe, kind, d, kw, what, **lk):
    c = d.c
    p = d.args(c.B)
    p.nt, p.ntiles, p.dual = kw["nt"], (c.B + 15) // 16, kw["dual"]
    p.Wp = d.pack(probe).data_ptr() if kw["wp"] else None
    return launch(probe, kind, d, p, f"{what} {kw}", **lk)


@pytest.mark.parametrize("epi", (EPI_STORE, EPI_SWIGLU), ids=("STORE", "SWIGLU"))
@pytest.mark.parametrize("ks", R.NORM_KSTEPS)
def test_mfma_norm_kernel(probe, ks, epi):
    pool = R.ExactPool()
    for c in R.norm_cases(ks, epi):
        d, ref = Dev(c), R.reference(c)
        what = c.name
        first = None
        for kw in tile_variants(c, K_MFMA_NORM):
            img, xo, b = mfma_launch(probe, K_MFMA_NORM, d, kw, what)
            if first is None:
                verify(K_MFMA_NORM, d, ref, img, xo, what, pool)
                first = (b, xo)
                # the rows rmsnorm_batch_kernel writes are the panel rows
                p = d.args(c.B)
                rimg, rxo, _ = launch(probe, K_RMSNORM, d, p, f"{what} rmsnorm_batch_kernel")
                assert torch.equal(rimg[:c.B, :c.K], xo[:c.B, :c.K]) and torch.equal(rxo[:c.B, :c.K], xo[:c.B, :c.K]), \
                    f"{what}: rmsnorm_batch_kernel rows differ from the norm kernel's xn_out rows"
            else:
                assert torch.equal(b, first[0]), f"{what}: {kw} changed the output bits"
                assert torch.equal(torch.nan_to_num(xo), torch.nan_to_num(first[1])), f"{what}: {kw} changed xn_out"
        _, _, b = mfma_launch(probe, K_MFMA_NORM, d, dict(nt=0, wp=False, dual=0), what, xn=False)
        assert torch.equal(b, first[0]), f"{what}: a null xn_out table changed the output bits"
        d.unchanged(what)
    pool.check(f"norm kernel KSTEPS {ks} epi {epi}")


@pytest.mark.parametrize("epi", (EPI_STORE, EPI_RESIDUAL), ids=("STORE", "RESIDUAL"))
@pytest.mark.parametrize("K", R.PLAIN_K)
def test_mfma_plain_kernel(probe, K, epi):
    pool = R.ExactPool()
    for c in R.plain_cases(K, epi):
        d, ref = Dev(c), R.reference(c)
        what = c.name
        first = None
        for kw in tile_variants(c, K_MFMA_PLAIN):
            img, _, b = mfma_launch(probe, K_MFMA_PLAIN, d, kw, what, xn=False)
            if first is None:
                verify(K_MFMA_PLAIN, d, ref, img, None, what, pool)
                first = b
            else:
                assert torch.equal(b, first), f"{what}: {kw} changed the output bits"
        if epi == EPI_RESIDUAL:
            for kw in tile_variants(c, K_MFMA_PLAIN)[:2]:
                _, _, b = mfma_launch(probe, K_MFMA_PLAIN, d, kw, what, xn=False, alias=True)
                assert torch.equal(b[:c.B, :c.N], first[:c.B, :c.N]), f"{what}: res aliasing y changed the output bits ({kw})"
        d.unchanged(what)
    pool.check(f"plain kernel K {K} epi {epi}")


def test_rmsnorm_batch_kernel(probe):
    for c in R.rmsnorm_cases():
        d, ref = Dev(c), R.reference(c)
        p = d.args(c.B)
        img, xo, _ = launch(probe, K_RMSNORM, d, p, c.name)
        verify(K_RMSNORM, d, ref, img, xo, c.name, None)
        img2, _, _ = launch(probe, K_RMSNORM, d, d.args(c.B), c.name, xn=False)
        assert torch.equal(img2[:c.B, :c.K], img[:c.B, :c.K])
        d.unchanged(c.name)


# ---- tally --------------------------------------------------------------------------------------------------------------------------
def test_zz_every_instantiation_was_reached(probe):
    """Runs last and needs the WHOLE module to have run in this process (it reads what the other tests recorded: a -k selection, another
    order or a distributed run leaves it nothing to count): the per-family record, and every instantiation the probe builds launched."""
    assert REACHED, "no launch was recorded: run the whole module in one process (this test only counts what the others launched)"
    print("\nkernel / storage type: cases checked, launches, largest error (ulp of the reference), largest err / bound, smallest bf16 exact "
          "fraction of a case of MIN_SCORED scored elements, pooled exact fraction of the smaller cases (exact of n)")
    for (name, dt), st in sorted(STATS.items()):
        pl = st["pool"]
        print(f"  {name:30s} {dt:5s} {st['cases']:5d} {st['launches']:6d}  {st['ulp']:.4g}  {st['ratio']:.4g}  {st['min_exact']:.5f}  "
              f"{pl.exact:.5f} ({pl.k} of {pl.n})")
    for kind in range(5):
        built = probe.gemv_probe_built(kind)
        print(f"  {KIND_NAME[kind]}: {len(REACHED[kind])} of {built} built instantiations launched")
    for kind in range(5):
        assert len(REACHED[kind]) == probe.gemv_probe_built(kind), \
            f"{KIND_NAME[kind]}: {len(REACHED[kind])} of {probe.gemv_probe_built(kind)} instantiations launched (was the whole module run?)"
