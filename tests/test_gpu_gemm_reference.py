"""Conformance of every GEMM kernel family and epilogue with the float64 reference of tests/_gemm_ref.py.

Each case is launched through tools/microbench/libgemm_probe.so on every family whose guard admits it, into sentinel-filled outputs
with guard rows before / after every segment and a leading dimension wider than N: every element outside {m_lo <= m < M, n < N} must
keep the sentinel, none inside may be NaN, and every computed element must meet the checker's bound and exact fraction.  The families
that keep one ascending K chain per element (all but skinny and split-K) must also agree with each other bit for bit.

When the module ends it prints, per family, the cases run, the largest error in ulps and the smallest exact fraction.  Observed on the MI355X
(the calibration of k, c, f in _gemm_ref.py): bf16 tile families exact fraction >= 0.9948 (the wide-range / cancelling operands),
>= 0.9996 elsewhere; skinny (every RB, NORM, SK_SWIGLU) >= 0.99976, split-K >= 0.99976; bf16 x 2 >= 0.773 (K = 7168); resunit bf16
0.99968, bf16 x 2 0.807; the largest ulp errors sit in elements whose
exact sum cancels and are covered by the c * S floor.  No kernel defect was found at these cases."""
import ctypes as C
import math
import os
from collections import defaultdict

import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libgemm_probe.so")
F64 = torch.float64

(F_CONV_64x32, F_CONV_64x64, F_CONV_128x32, F_CONV_128x64, F_CONV_128x96, F_SPLITK, F_GLDS4_128x64_S2, F_GLDS8_64x128_S3,
 F_GLDS8_64x64_S3, F_GLDS8_128x64_S3, F_GLDS8_128x64_S2, F_CHAIN_8x8, F_CHAIN_16x4, F_BIG_TR_PAIR, F_BIG_PAIR, F_BIG_TR_RING,
 F_BIG_RING, F_BIG_TR_128, F_BIG_128, F_SKINNY, F_SKINNY_SWIGLU, F_SWIGLU_HALVES, F_RESUNIT, F_LAUNCH) = range(24)
NAMES = ["conv64x32", "conv64x64", "conv128x32", "conv128x64", "conv128x96", "splitK", "glds4_128x64_s2", "glds8_64x128_s3",
         "glds8_64x64_s3", "glds8_128x64_s3", "glds8_128x64_s2", "chain8x8", "chain16x4", "big_tr_pair", "big_pair", "big_tr_ring",
         "big_ring", "big_tr_128", "big_128", "skinny", "skinny_swiglu", "swiglu_halves", "resunit", "launch"]
TILE_FAMILIES = [F_CONV_64x32, F_CONV_64x64, F_CONV_128x32, F_CONV_128x64, F_CONV_128x96, F_GLDS4_128x64_S2, F_GLDS8_64x128_S3,
                 F_GLDS8_64x64_S3, F_GLDS8_128x64_S3, F_GLDS8_128x64_S2, F_CHAIN_8x8, F_CHAIN_16x4, F_BIG_TR_PAIR, F_BIG_PAIR,
                 F_BIG_TR_RING, F_BIG_RING, F_BIG_TR_128, F_BIG_128, F_LAUNCH]
TE = {"bf16": 0, "bfs": 1, "f32": 2}
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


class GemmArgs(C.Structure):
    _fields_ = [("A", vp), ("lda", i32), ("M", i32), ("a_rows", i32), ("m_lo", i32), ("n_taps", i32), ("tap_off", i32 * 8), ("Cin", i32),
                ("W", vp), ("N", i32), ("bias", vp), ("bias_mod", i32), ("scale", vp), ("res", vp), ("ldr", i32), ("Y", vp), ("ldy", i32),
                ("act", i32), ("sn_a", vp), ("sn_ib", vp), ("Y2", vp), ("act2", i32), ("ws", vp), ("ws_floats", i64), ("ksplit", i32),
                ("n_seg", i32), ("a_seg", i64), ("y_seg", i64), ("r_seg", i64), ("glds_min_wgs", i32), ("big_pair", i32), ("Wp", vp),
                ("Wi", vp), ("no_skinny", i32), ("glds_cap8", i32), ("chain", i32), ("glds_waves", i32), ("xcd_map", i32),
                ("epi_legacy", i32)]


class ProbeArgs(C.Structure):
    _fields_ = [("g", GemmArgs), ("g2", GemmArgs), ("y", vp), ("rb_force", i32), ("mt", i32), ("ssq_out", vp), ("ssq_ld", i32),
                ("ssq", vp), ("gain", vp), ("eps", C.c_float)]


GLDS = [F_GLDS4_128x64_S2, F_GLDS8_64x128_S3, F_GLDS8_64x64_S3, F_GLDS8_128x64_S3, F_GLDS8_128x64_S2]
BIG_TR = [F_BIG_TR_PAIR, F_BIG_TR_RING, F_BIG_TR_128]

STATS = defaultdict(lambda: {"cases": 0, "max_ulp": 0.0, "min_exact": 1.0})     # per family, printed when the module ends


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libgemm_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.gemm_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(ProbeArgs), vp]
    lib.gemm_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(ProbeArgs)]
    lib.gemm_probe_pack.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.gemm_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    assert lib.gemm_probe_version() == 1 and lib.gemm_probe_families() == len(NAMES)
    buf = (C.c_long * 64)()
    n = lib.gemm_probe_layout(buf, 64)
    names = [f[0] for f in GemmArgs._fields_]
    want = [C.sizeof(GemmArgs), C.sizeof(ProbeArgs)] + [getattr(GemmArgs, f).offset for f in names] + \
           [getattr(ProbeArgs, f[0]).offset for f in ProbeArgs._fields_[1:]]
    assert list(buf[:n]) == want, "ctypes mirror of GemmArgs / ProbeArgs is out of date"
    return lib


# ---- device buffers -----------------------------------------------------------------------------------------------------------
def dev(x, dt):
    return R.to_storage(x, dt).cuda().contiguous()


def sentinel_buffer(shape, dt):
    v = R.SENTINEL[dt]
    t = torch.full(shape, v - (1 << 32) if v >= (1 << 31) else v, dtype=torch.int32, device="cuda")
    if dt == "bf16":
        return t.to(torch.int16).view(torch.bfloat16)
    if dt == "f32":
        return t.view(torch.float32)
    return t


class Launch:
    """Device image of one Gemm: operands, and sentinel-guarded outputs [n_seg][G + M + G][ldy]."""
    G = 3

    def __init__(self, g: R.Gemm, *, extra_ld=4):
        self.g, dt = g, g.dt
        self.keep = []                                # device copies of bias / scale / SnakeBeta constants: alive while launches run
        nseg, rows_alloc, Cin = g.A.shape
        self.A = dev(g.A, dt)
        wdt = "f32" if dt == "f32" else "bf16"
        W = g.W
        if dt == "bfs":                               # K columns duplicated against the [rows][2 Cin] bf16 image of A
            W = W.repeat_interleave(2, dim=1)
        self.W = dev(W, wdt)
        self.n_out = g.N // 2 if g.act == 2 else g.N
        self.ldy = self.n_out + extra_ld
        a = GemmArgs()
        a.A, a.lda, a.M, a.a_rows, a.m_lo = self.A.data_ptr(), Cin, g.M, g.a_rows, g.m_lo
        a.n_taps = len(g.taps)
        for i, o in enumerate(g.taps):
            a.tap_off[i] = o
        a.Cin, a.W, a.N, a.bias_mod = Cin, self.W.data_ptr(), g.N, g.bmod
        a.n_seg, a.a_seg = nseg, rows_alloc * Cin
        a.act, a.act2 = g.act, g.act2
        for name in ("bias", "scale", "sn_a", "sn_ib"):
            v = getattr(g, name)
            if v is not None:
                t = dev(v, dt)
                self.keep.append(t)
                setattr(a, name, t.data_ptr())
        if g.res is not None:
            self.ldr = g.N + extra_ld
            res = torch.zeros(nseg, g.M, self.ldr, dtype=F64)
            res[:, :, :g.N] = g.res
            self.res = dev(res, dt)
            a.res, a.ldr, a.r_seg = self.res.data_ptr(), self.ldr, g.M * self.ldr
        a.ldy, a.y_seg = self.ldy, (g.M + 2 * self.G) * self.ldy
        self.a = a

    def outputs(self, p: ProbeArgs, swiglu_y=False):
        g, dt = self.g, self.g.dt
        shape = (self.g.n_seg, g.M + 2 * self.G, self.n_out if swiglu_y else self.ldy)    # (gemm_swiglu_halves: y is dense [M][I])
        self.Y = sentinel_buffer(shape, dt) if g.y else None
        self.Y2 = sentinel_buffer(shape, dt) if g.y2 else None
        p.g = self.a
        p.g.Y = self.Y[:, self.G:].data_ptr() if g.y and not swiglu_y else None
        p.g.Y2 = self.Y2[:, self.G:].data_ptr() if g.y2 else None
        if swiglu_y:            # gemm_swiglu_halves: Y = the [M][2 I] gate | up image (third form), y = the [M][I] output
            self.GU = torch.zeros(g.M, g.N, dtype=torch.bfloat16 if dt == "bf16" else torch.float32, device="cuda")
            p.g.Y, p.g.ldy = self.GU.data_ptr(), g.N
            p.y = self.Y[:, self.G:].data_ptr()
        return p


def check_sentinels(buf, g, n_out, what):
    bits = R.raw_bits(buf.cpu())
    sent = R.SENTINEL[g.dt]
    G = Launch.G
    inside = torch.zeros(bits.shape, dtype=torch.bool)
    inside[:, G + g.m_lo:G + g.M, :n_out] = True
    outside_bad = (bits != sent) & ~inside
    assert not bool(outside_bad.any()), f"{what}: {int(outside_bad.sum())} elements written outside the output, first at " \
                                        f"{tuple(int(v) for v in torch.nonzero(outside_bad)[0])} (segment, guard-offset row, column)"
    vals = R.from_storage(buf.cpu(), g.dt)[:, G + g.m_lo:G + g.M, :n_out]
    assert not bool(torch.isnan(vals).any()), f"{what}: NaN (or an unwritten sentinel) inside the output"
    return vals


def record(fam_name, v):
    st = STATS[fam_name]
    st["cases"] += 1
    st["max_ulp"] = max(st["max_ulp"], v.max_ulp)
    st["min_exact"] = min(st["min_exact"], v.exact)


def run_case(probe, case, g, families, *, expect_refused, rows=None, p_extra=None, ws_floats=0, ksplit=0, bit_identity=True, extra_ld=4,
             ref=None):
    """Launch g on every family in `families`; the probe must refuse exactly `expect_refused` (the shapes their guards reject) and every
    other family must match the reference.  Returns the families that ran."""
    te = TE[g.dt]
    ref = ref or R.reference(g, rows)
    rows_idx = torch.arange(g.m_lo, g.M) if rows is None else rows
    L = Launch(g, extra_ld=extra_ld)
    outs = {}
    refused, ran = [], []
    for fam in families:
        p = ProbeArgs()
        ws = None
        L.outputs(p)
        p.g.ws, p.g.ws_floats, p.g.ksplit = None, 0, 0
        if fam == F_SPLITK:
            ws = sentinel_buffer((ws_floats + 256,), "f32")
            p.g.ws, p.g.ws_floats, p.g.ksplit = ws.data_ptr(), ws_floats, ksplit
        if p_extra:
            p_extra(p, fam)
        if not probe.gemm_probe_admits(fam, te, C.byref(p)):
            refused.append(fam)
            continue
        rc = probe.gemm_probe_run(fam, te, C.byref(p), None)
        assert rc == 0, f"{case} / {NAMES[fam]}: launch returned {rc}"
        torch.cuda.synchronize()
        what = f"{case} [{g.dt}] / {NAMES[fam]}"
        if ws is not None:
            tail = R.raw_bits(ws[ws_floats:].cpu())
            assert bool((tail == R.SENTINEL["f32"]).all()), f"{what}: split-K partials written past ws_floats"
        for buf, r, s, e in ((L.Y, ref.y, ref.s_y, ref.e_y), (L.Y2, ref.y2, ref.s_y2, ref.e_y2)):
            if buf is None:
                continue
            vals = check_sentinels(buf, g, L.n_out, what + (" Y2" if buf is L.Y2 else ""))
            got = vals[:, rows_idx - g.m_lo]
            v = R.check(got, r, s, g.dt, ref.K, what=what + (" Y2" if buf is L.Y2 else ""), rows=rows_idx, extra=e)
            assert v.ok, v.msg
            record(NAMES[fam] + ("" if g.dt == "bf16" else f"[{g.dt}]"), v)
        ran.append(fam)
        if bit_identity and fam not in (F_SPLITK, F_SKINNY, F_SKINNY_SWIGLU):
            outs[fam] = tuple(R.raw_bits(b.cpu()) for b in (L.Y, L.Y2) if b is not None)
    assert sorted(refused) == sorted(expect_refused), \
        f"{case}: refused {[NAMES[f] for f in refused]}, expected {[NAMES[f] for f in expect_refused]}"
    if bit_identity and len(outs) > 1:
        base_f, base = next(iter(outs.items()))
        for f, o in outs.items():
            assert all(torch.equal(x, y) for x, y in zip(o, base)), f"{case}: {NAMES[f]} differs from {NAMES[base_f]} bit for bit"
    return ran


def but(*fams):
    """TILE_FAMILIES without fams: the expected refusals of a case that only those families admit."""
    return [f for f in TILE_FAMILIES if f not in fams]


# ---- operands ------------------------------------------------------------------------------------------------------------------
def operands(dt, *, M, N, Cin, taps=(0,), nseg=1, rows_alloc=None, a_rows=None, m_lo=0, act=0, bias=True, bias_mod=0, scale=False,
             res=False, y=True, y2=False, act2=0, seed=0, wide=False):
    gen = torch.Generator().manual_seed(seed)
    rows_alloc = rows_alloc or M
    K = len(taps) * Cin
    A = torch.randn(nseg, rows_alloc, Cin, generator=gen, dtype=F64)
    W = torch.randn(N, K, generator=gen, dtype=F64) / math.sqrt(K)
    if wide:
        # wide dynamic range (2^-12 .. 2^12 per input channel), and odd rows whose exact sums nearly cancel: the second half of K
        # repeats the first half of the row against the negated first half of W times (1 + 2^-7)
        A = A * torch.pow(2.0, torch.randint(-12, 12, (1, 1, Cin), generator=gen).to(F64))
        h = K // 2
        A[:, 1::2, h:] = A[:, 1::2, :h]
        W[:, h:] = -R.rnd(W[:, :h], "bf16") * (1 + 2.0 ** -7)
    if act == 8:
        A, W = A.abs(), W.abs()
    A, W = R.rnd(A, dt), R.rnd(W, "f32" if dt == "f32" else "bf16")
    bm = bias_mod or N
    g = R.Gemm(A=A, W=W, M=M, a_rows=M if a_rows is None else a_rows, taps=list(taps), m_lo=m_lo, dt=dt, act=act, bias_mod=bias_mod,
               y=y, y2=y2, act2=act2)
    if bias:
        g.bias = R.rnd(torch.randn(bm, generator=gen, dtype=F64) * 0.3, dt)
    if scale:
        g.scale = R.rnd(torch.rand(N, generator=gen, dtype=F64) + 0.5, dt)
    if res:
        g.res = R.rnd(torch.randn(nseg, M, N, generator=gen, dtype=F64), dt)
    if y2 and act2 == 0:
        g.sn_a = R.rnd(torch.rand(bm, generator=gen, dtype=F64) + 0.5, dt)
        g.sn_ib = R.rnd(torch.rand(bm, generator=gen, dtype=F64) + 0.5, dt)
    return g


# ---- edge shapes -----------------------------------------------------------------------------------------------------------------
EDGE_M = [1, 15, 16, 17, 31, 33, 63, 65, 127, 129, 255, 257, 513]


@pytest.mark.parametrize("M", EDGE_M)
def test_edge_rows_every_tile_family(probe, M):
    # plain (bias only) at N = 256, K = 4 x 64: every tile family, the transposed big tiles included
    g = operands("bf16", M=M, N=256, Cin=64, taps=(-1, 0, 1, 2), a_rows=M, seed=M)
    run_case(probe, f"edge M={M} plain", g, TILE_FAMILIES, expect_refused=[])
    # full epilogue at a ragged N (N % 4 != 0, odd bias_mod, odd ldy): the per-element fallbacks
    g = operands("bf16", M=M, N=100, Cin=96, bias_mod=25, act=1, scale=True, res=True, y2=True, seed=M + 1)
    run_case(probe, f"edge M={M} ragged N", g, TILE_FAMILIES, extra_ld=5, expect_refused=GLDS + BIG_TR + [F_BIG_PAIR, F_BIG_128])


@pytest.mark.parametrize("dt", ["bf16", "bfs"])
def test_taps_below_m_lo_short_a_rows_and_segments(probe, dt):
    # m_lo > 0 with 7 taps at dilation 3 that read rows below it, a_rows < M, SnakeBeta second output and residual
    g = operands(dt, M=300, N=192, Cin=128, taps=[-3 * (6 - i) for i in range(7)], m_lo=37, a_rows=280, rows_alloc=310, res=True,
                 y2=True, seed=11)
    run_case(probe, "m_lo 37, a_rows 280, k7 d3", g, TILE_FAMILIES, expect_refused=[F_GLDS8_64x128_S3] + BIG_TR + [F_BIG_128])
    # three segments with negative taps (the batched decode): segment g must read zeros, not segment g - 1's rows
    g = operands(dt, M=45, N=128, Cin=64, taps=(-4, -2, 0), nseg=3, res=True, seed=12)
    run_case(probe, "n_seg 3, taps -4 -2 0", g, TILE_FAMILIES, expect_refused=BIG_TR)
    g = operands(dt, M=70, N=64, Cin=64, taps=(-9, 0), nseg=2, m_lo=5, seed=13, y2=True)
    run_case(probe, "n_seg 2, m_lo 5", g, TILE_FAMILIES, expect_refused=[F_GLDS8_64x128_S3] + BIG_TR + [F_BIG_128])


@pytest.mark.parametrize("act", [1, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_activations_and_elu_second_output(probe, act, dt):
    # the reference-audio GEMMs (acts 4 .. 8, ELU Y2; fp32 in the product) and the codec's GELU / SiLU
    refused = [F_GLDS8_64x128_S3] + BIG_TR + [F_BIG_128] if dt == "bf16" else but(F_CONV_64x64, F_LAUNCH)
    g = operands(dt, M=100, N=64, Cin=64, taps=(-2, -1, 0), act=act, y2=act in (5, 7), act2=1, scale=act == 1, res=act == 3, seed=20 + act)
    run_case(probe, f"act {act}", g, TILE_FAMILIES, expect_refused=refused)
    if act == 5:
        # Y null, only Y2 written
        g = operands(dt, M=130, N=64, Cin=64, act=5, y=False, y2=True, act2=1, seed=29)
        run_case(probe, "Y null, ELU Y2 only", g, TILE_FAMILIES, expect_refused=refused)


def test_single_k_step_odd_steps_and_wide_range(probe):
    run_case(probe, "single K step", operands("bf16", M=70, N=64, Cin=32, seed=30), TILE_FAMILIES,
             expect_refused=GLDS + BIG_TR + [F_BIG_PAIR, F_BIG_128])
    run_case(probe, "K = 7 x 32", operands("bf16", M=129, N=128, Cin=224, res=True, seed=31), TILE_FAMILIES,
             expect_refused=GLDS + BIG_TR + [F_BIG_PAIR])
    run_case(probe, "wide range, cancelling rows", operands("bf16", M=200, N=256, Cin=512, wide=True, seed=32), TILE_FAMILIES,
             expect_refused=[])


@pytest.mark.parametrize("plain_order", [0, -1])
def test_tile_orders(probe, plain_order):
    g = operands("bf16", M=1000, N=768, Cin=256, res=True, seed=40)

    def order(p, fam):
        p.g.xcd_map = plain_order
    run_case(probe, f"xcd_map {plain_order}", g, TILE_FAMILIES, p_extra=order, expect_refused=BIG_TR)


def test_codec_shapes(probe):
    # transposed conv: N = 2 Cout, bias / SnakeBeta channel n % Cout (bias_mod < N), two taps
    g = operands("bf16", M=600, N=384, Cin=192, taps=(-1, 0), bias_mod=192, y2=True, seed=50)
    run_case(probe, "upsample bias_mod 192", g, TILE_FAMILIES, expect_refused=BIG_TR)
    # k7 at dilation 9, the codec's block 3
    g = operands("bf16", M=900, N=192, Cin=192, taps=[-9 * (6 - i) for i in range(7)], res=True, y2=True, seed=51)
    run_case(probe, "k7 d9", g, TILE_FAMILIES, expect_refused=[F_GLDS8_64x128_S3] + BIG_TR + [F_BIG_128])
    # the frame transformer's act 2 GEMM: [gate | up] in 16-column groups (only tiles with 64-wide column pairs)
    g = operands("bf16", M=200, N=1024, Cin=512, act=2, bias=False, seed=52)
    run_case(probe, "act 2 (SwiGLU epilogue)", g, TILE_FAMILIES, expect_refused=but(F_CONV_64x64, F_CONV_128x64, F_GLDS4_128x64_S2, F_LAUNCH))
    # streaming chunk dec.0: 52 rows against K = 7 x 1024 (chain GEMM territory), bf16 x 2
    g = operands("bfs", M=52, N=1536, Cin=1024, taps=range(-6, 1), seed=53)
    run_case(probe, "chunk dec.0 bf16x2", g, TILE_FAMILIES, expect_refused=BIG_TR)


def test_large_codec_conv_row_sample(probe):
    # block 4 of a 370-frame decode: 709845 rows, 96 channels, 7 taps.  Every column on a row sample -- the first and last row of
    # every 64-row slice of [m_lo, M) (so of every tile of every family), the rows around m_lo, the last rows, 512 seeded random
    # rows -- and the sentinels on the whole buffer
    M, m_lo = 709845, 1000
    gen = torch.Generator().manual_seed(60)
    g = operands("bf16", M=M, N=96, Cin=96, taps=range(-6, 1), m_lo=m_lo, res=True, y2=True, seed=60)
    rel = torch.arange(0, M - m_lo)
    edges = m_lo + rel[(rel % 64 == 0) | (rel % 64 == 63)]
    rows = torch.cat([edges, torch.arange(m_lo, m_lo + 10), torch.arange(M - 300, M), torch.randint(m_lo, M, (512,), generator=gen)]).unique()
    run_case(probe, "709845 rows k7 C96", g, [F_CONV_128x96, F_CONV_128x32, F_BIG_RING, F_LAUNCH], rows=rows, expect_refused=[])


# ---- prefill / batch shapes: skinny, split-K, SwiGLU halves -----------------------------------------------------------------------
def _pack(probe, W, swiglu_I):
    P = torch.empty_like(W)
    assert probe.gemm_probe_pack(W.data_ptr(), P.data_ptr(), W.shape[0], W.shape[1], swiglu_I, None) == 0
    return P


@pytest.mark.parametrize("M,N,K,rb_refused", [(16, 1024, 1024, {3}), (200, 4096, 1024, {3}), (52, 2048, 2048, {3}), (416, 1024, 3072, {3}),
                                              (33, 1024, 6144, {2, 3}), (200, 6144, 1024, set()), (64, 12288, 2048, set())])
def test_prefill_gemms(probe, M, N, K, rb_refused):
    # 0.6B / 1.7B prefill widths: qkv 4096, o / down 1024 / 2048, gate | up 6144 / 12288 (as one store: RB = 3 where N / 16 % 3 == 0)
    g = operands("bf16", M=M, N=N, Cin=K, bias=False, res=True, seed=M + N)
    ref = R.reference(g)
    run_case(probe, f"prefill {M}x{N}x{K}", g, TILE_FAMILIES, expect_refused=BIG_TR, ref=ref)
    L = Launch(g)
    Wp = _pack(probe, L.W, 0)
    for rb in (0, 1, 2, 3):
        outs = []
        for wp in (None, Wp):
            def extra(p, f, wp=wp, rb=rb):
                p.g.Wp = wp.data_ptr() if wp is not None else None
                p.rb_force = rb
            outs.append(run_skinny(probe, f"prefill {M}x{N}x{K} Wp={wp is not None} rb={rb}", g, ref, extra, refused=rb in rb_refused))
        assert outs[0] is None or torch.equal(outs[0], outs[1]), f"prefill {M}x{N}x{K} rb={rb}: the fragment-major copy changed the output"
    S = 4 if K % 128 == 0 and K // 128 >= 12 else 0
    if S:
        run_case(probe, f"prefill {M}x{N}x{K} split-K {S}", g, [F_SPLITK], ws_floats=S * M * N, ksplit=S, expect_refused=[], ref=ref)


def run_skinny(probe, case, g, ref, extra, *, refused, swiglu=False, norm=None):
    """One skinny launch (SK_STORE / SK_RESIDUAL, or SK_SWIGLU into the dense [M][N / 2] output); returns the output's bits, or None
    when the probe refused it as it must (`refused`)."""
    fam = F_SKINNY_SWIGLU if swiglu else F_SKINNY
    L = Launch(g)
    p = ProbeArgs()
    if swiglu:
        L.n_out = g.N // 2
    L.outputs(p, swiglu_y=swiglu)
    if norm is not None:
        p.ssq, p.gain, p.eps = norm[0].data_ptr(), norm[1].data_ptr(), g.eps
    extra(p, fam)
    adm = probe.gemm_probe_admits(fam, 0, C.byref(p))
    assert adm == (0 if refused else 1), f"{case}: the probe {'admitted' if adm else 'refused'} {NAMES[fam]}"
    if refused:
        return None
    assert probe.gemm_probe_run(fam, 0, C.byref(p), None) == 0
    torch.cuda.synchronize()
    vals = check_sentinels(L.Y, g, L.n_out, case)
    v = R.check(vals, ref.y, ref.s_y, "bf16", ref.K, what=case, extra=ref.e_y)
    assert v.ok, v.msg
    record(NAMES[fam] + ("[norm]" if norm is not None else ""), v)
    return R.raw_bits(L.Y.cpu())


def _norm_operands(M, N, K, seed):
    gen = torch.Generator().manual_seed(seed)
    X = R.rnd(torch.randn(1, M, K, generator=gen, dtype=F64) * 2.0, "bf16")
    gain = R.rnd(torch.rand(K, generator=gen, dtype=F64) + 0.5, "bf16")
    ssq = (X[0].to(torch.float32).double() ** 2).reshape(M, K // 16, 16).sum(-1).to(torch.float32)
    W = R.rnd(torch.randn(N, K, generator=gen, dtype=F64) / math.sqrt(K), "bf16")
    g = R.Gemm(A=X, W=W, M=M, a_rows=M, dt="bf16", ssq=ssq, gain=gain)
    return g, (ssq.cuda(), R.to_storage(gain, "bf16").cuda())


@pytest.mark.parametrize("I,K", [(3072, 1024), (6144, 2048)])
@pytest.mark.parametrize("norm", [False, True])
def test_skinny_swiglu_gate_up(probe, I, K, norm):
    # the prefill's gate | up (0.6B: I = 3072, K = 1024; 1.7B: I = 6144, K = 2048) and the batch decode's normalising SK_SWIGLU: every
    # rb_force (the launcher takes RB = 3 at both widths), with the row-major and the fragment-major (8 gate + 8 up rows) weight
    M = 128 if norm else 200
    if norm:
        g, nd = _norm_operands(M, 2 * I, K, seed=I + K)
    else:
        g, nd = operands("bf16", M=M, N=2 * I, Cin=K, bias=False, seed=I + K), None
    ref = R.swiglu_halves_ref(g)
    Wp = _pack(probe, Launch(g).W, I)
    for rb in (0, 1, 2, 3):
        outs = []
        for wp in (None, Wp):
            def extra(p, f, wp=wp, rb=rb):
                p.g.Wp = wp.data_ptr() if wp is not None else None
                p.rb_force = rb
            outs.append(run_skinny(probe, f"SK_SWIGLU{' NORM' if norm else ''} {M}x{I}x{K} Wp={wp is not None} rb={rb}", g, ref, extra,
                                   refused=False, swiglu=True, norm=nd))
        assert torch.equal(outs[0], outs[1]), f"rb={rb}: the fragment-major copy changed the output"


@pytest.mark.parametrize("K,M", [(1024, 64), (2048, 200)])
def test_skinny_norm_and_ssq_producer(probe, K, M):
    # the normalising SK_STORE (qkv of the batch decode) at every rb_force: N = 3072 has N / 16 % 3 == 0
    N = 3072
    g, nd = _norm_operands(M, N, K, seed=K + M)
    ref = R.reference(g)
    for rb in (0, 1, 2, 3):
        def extra(p, f, rb=rb):
            p.rb_force = rb
        run_skinny(probe, f"skinny NORM K={K} M={M} rb={rb}", g, ref, extra, refused=False, norm=nd)
    # the producer: SK_RESIDUAL with per-16-column sums of squares of the stored values
    g2 = operands("bf16", M=M, N=K, Cin=1024, bias=False, res=True, seed=K)
    ref2 = R.reference(g2)
    L2 = Launch(g2)
    out = torch.full((M, K // 16 + 3), float("nan"), dtype=torch.float32, device="cuda")
    p = ProbeArgs()
    L2.outputs(p)
    p.ssq_out, p.ssq_ld = out.data_ptr(), K // 16 + 3
    assert probe.gemm_probe_run(F_SKINNY, 0, C.byref(p), None) == 0
    torch.cuda.synchronize()
    vals = check_sentinels(L2.Y, g2, K, "skinny ssq producer")
    v = R.check(vals, ref2.y, ref2.s_y, "bf16", ref2.K, what="skinny SK_RESIDUAL + ssq_out", extra=ref2.e_y)
    assert v.ok, v.msg
    got = out.cpu().double()
    want = (vals[0] ** 2).reshape(M, K // 16, 16).sum(-1)
    assert torch.allclose(got[:, :K // 16], want, rtol=4e-6, atol=0), "ssq_out differs from the sum of squares of the stored values"
    assert bool(torch.isnan(got[:, K // 16:]).all()), "ssq_out written past K / 16 columns"


@pytest.mark.parametrize("act", [0, 1, 3, 5])
def test_splitk_epilogues(probe, act):
    # split-K's second pass (splitk_reduce_kernel) runs the whole epilogue: bias, GELU / SiLU, scale, residual, SnakeBeta Y2, at a ragged
    # N and M and every slice count the guard admits; acts >= 4 and the ELU second output are not in that epilogue: refused
    M, N, K = 77, 200, 1536
    g = operands("bf16", M=M, N=N, Cin=K, act=act, scale=act != 3, res=act != 1, y2=True, act2=1 if act == 5 else 0, seed=80 + act)
    ref = R.reference(g)
    for S in (2, 3, 4, 8):
        run_case(probe, f"split-K S={S} act {act}", g, [F_SPLITK], ws_floats=S * M * N, ksplit=S, ref=ref,
                 expect_refused=[F_SPLITK] if act == 5 else [])
    # a workspace one slice short is refused (ws_floats bounds the partials)
    run_case(probe, f"split-K workspace short act {act}", g, [F_SPLITK], ws_floats=4 * M * N - 1, ksplit=4, ref=ref, expect_refused=[F_SPLITK])


@pytest.mark.parametrize("M,I,K,form", [(200, 1536, 1024, "skinny"), (2000, 3072, 1024, "ring"), (2560, 1024, 2048, "pair"),
                                        (517, 3072, 1024, "pair"), (600, 512, 1024, "pair")])
def test_swiglu_halves(probe, M, I, K, form):
    _swiglu_halves(probe, M, I, K, form)


def _swiglu_halves(probe, M, I, K, form):
    # gemm_swiglu_halves in its three forms.  Which one ran is asserted through the [M][2 I] gate | up image: only the GEMM + silu_mul
    # pair writes it.  The ring tile over the interleaved copy must equal the pair bit for bit.
    g = operands("bf16", M=M, N=2 * I, Cin=K, bias=False, seed=M + I)
    gen = torch.Generator().manual_seed(M)
    rows = None if M <= 600 else torch.cat([torch.arange(0, 64), torch.arange(M - 64, M), torch.randint(0, M, (256,), generator=gen)]).unique()
    ref = R.swiglu_halves_ref(g, rows)
    L = Launch(g)
    Wi = R.interleave16(g.W)
    Wi_dev = _pack(probe, L.W, -I)
    assert torch.equal(Wi_dev.cpu(), R.to_storage(Wi, "bf16")), "16-row-interleaved copy differs from the documented layout"
    ws = torch.empty(1 << 20, dtype=torch.float32, device="cuda")
    Wp = _pack(probe, L.W, I) if form == "skinny" else None
    L.n_out = I

    def launch(use_form):
        p = ProbeArgs()
        L.outputs(p, swiglu_y=True)
        L.GU.view(torch.int16).fill_(R.SENTINEL["bf16"] - (1 << 16))
        p.g.Wi = Wi_dev.data_ptr() if use_form == "ring" else None
        if use_form == "skinny":
            p.g.ws, p.g.ws_floats, p.g.Wp = ws.data_ptr(), 1 << 20, Wp.data_ptr()
        assert probe.gemm_probe_run(F_SWIGLU_HALVES, 0, C.byref(p), None) == 0
        torch.cuda.synchronize()
        gu_written = bool((R.raw_bits(L.GU.cpu()) != R.SENTINEL["bf16"]).all())
        gu_untouched = bool((R.raw_bits(L.GU.cpu()) == R.SENTINEL["bf16"]).all())
        assert gu_written if use_form == "pair" else gu_untouched, f"swiglu halves {M}x{I}x{K}: not the {use_form} form"
        vals = check_sentinels(L.Y, g, I, f"swiglu halves {use_form}")
        if rows is not None:
            vals = vals[:, rows]
        v = R.check(vals, ref.y, ref.s_y, "bf16", ref.K, what=f"swiglu halves {use_form} {M}x{I}x{K}", extra=ref.e_y)
        assert v.ok, v.msg
        record(f"swiglu_halves[{use_form}]", v)
        return R.raw_bits(L.Y.cpu())
    y = launch(form)
    if form == "ring":
        assert torch.equal(y, launch("pair")), f"swiglu halves {M}x{I}x{K}: the ring tile differs from GEMM + silu_mul bit for bit"
    return [F_SWIGLU_HALVES]


# ---- the fused residual unit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,ch", [("bf16", 96), ("bf16", 192), ("bfs", 96)])
def test_resunit(probe, dt, ch):
    _resunit(probe, dt, ch, 700, 45)


def _resunit(probe, dt, ch, M, m_lo):
    g1 = operands(dt, M=M, N=ch, Cin=ch, taps=[-3 * (6 - i) for i in range(7)], m_lo=m_lo, y=False, y2=True, seed=ch)
    ref1 = R.reference(g1)                                           # mid = SnakeBeta(conv1 + b1)
    mid = torch.zeros(1, M, ch, dtype=F64)
    mid[0, m_lo:] = ref1.y2[0]
    g2 = operands(dt, M=M, N=ch, Cin=ch, m_lo=m_lo, res=True, y2=True, seed=ch + 1)
    g2.A = mid
    ref2 = R.reference(g2)
    L1, L2 = Launch(g1, extra_ld=0), Launch(g2, extra_ld=0)         # (resunit_ok: ldy = ldr = C)
    p = ProbeArgs()
    L2.outputs(p)
    c2 = GemmArgs.from_buffer_copy(p.g)
    L1.outputs(p)
    p.g2 = c2
    p.g.Y2 = None
    assert probe.gemm_probe_admits(F_RESUNIT, TE[dt], C.byref(p)) == 1
    assert probe.gemm_probe_run(F_RESUNIT, TE[dt], C.byref(p), None) == 0
    torch.cuda.synchronize()
    # mid is itself a rounded output: its allowed flips (one ulp, the SnakeBeta sine) enter conv2 through |W2|
    e_mid = torch.zeros(1, M, ch, dtype=F64)
    e_mid[0, m_lo:] = ref1.e_y2[0] + R.ulp(ref1.y2[0], dt)
    e_acc = e_mid[:, m_lo:] @ g2.W.abs().t()
    sn = (1.0 + (g2.sn_ib * g2.sn_a).abs())
    # two chained GEMMs: the exact fraction of bf16 x 2 is that of a K = 7 C GEMM fed with a K = 7 C GEMM's flips (0.807 observed at C = 96)
    f = 0.75 if dt == "bfs" else None
    for buf, r, s, e in ((L2.Y, ref2.y, ref2.s_y, ref2.e_y + e_acc), (L2.Y2, ref2.y2, ref2.s_y2, ref2.e_y2 + e_acc * sn)):
        vals = check_sentinels(buf, g2, ch, "resunit")
        v = R.check(vals, r, s, dt, ref2.K, what=f"resunit C={ch} [{dt}]", rows=torch.arange(m_lo, M), extra=e, f=f)
        assert v.ok, v.msg
        record(f"resunit[{dt}]", v)
    return [F_RESUNIT]


# ---- the product dispatchers with their switches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", [dict(), dict(xcd_map=-1), dict(glds_waves=-1), dict(chain=-1), dict(glds_cap8=64)])
def test_dispatcher_switches(probe, sw):
    def extra(p, fam):
        for k, v in sw.items():
            setattr(p.g, k, v)
    for dt in ("bf16", "bfs"):
        g = operands(dt, M=416, N=768, Cin=256, taps=(-2, -1, 0), res=True, y2=True, seed=70)
        run_case(probe, f"gemm_launch {sw}", g, [F_LAUNCH, F_CONV_64x64], p_extra=extra, expect_refused=[])
    g = operands("f32", M=150, N=96, Cin=64, taps=(-1, 0), act=1, scale=True, res=True, y2=True, act2=1, seed=71)
    run_case(probe, f"gemm_launch<float> {sw}", g, [F_LAUNCH, F_CONV_64x64], p_extra=extra, expect_refused=[])


# ---- refusals and coverage ------------------------------------------------------------------------------------------------------
def test_probe_refuses_what_the_guards_refuse(probe):
    g = operands("bf16", M=64, N=100, Cin=96, act=2, bias=False)
    L = Launch(g)
    p = ProbeArgs()
    L.outputs(p)
    # act 2: only the 64- and 128-row tiles with 64-wide column pairs, the four-wave LDS-DMA tile (here N % 64 != 0), and the dispatcher
    admitted = [f for f in range(len(NAMES)) if probe.gemm_probe_admits(f, 0, C.byref(p))]
    assert [NAMES[f] for f in admitted] == ["conv64x64", "conv128x64", "launch"], [NAMES[f] for f in admitted]
    assert probe.gemm_probe_run(F_CONV_64x32, 0, C.byref(p), None) == probe.gemm_probe_refused_code()
    # bf16 x 2 never takes the transposed (bf16-store) big tiles, skinny or split-K
    g = operands("bfs", M=64, N=256, Cin=64)
    L = Launch(g)
    p = ProbeArgs()
    L.outputs(p)
    refused = [NAMES[f] for f in range(len(NAMES)) if not probe.gemm_probe_admits(f, 1, C.byref(p))]
    assert refused == ["splitK", "big_tr_pair", "big_tr_ring", "big_tr_128", "skinny", "skinny_swiglu", "swiglu_halves", "resunit"], refused
    # the transposed big tiles only at the widths gemm_launch sends there (N % 256, N % 128 for the 128-wide one)
    g = operands("bf16", M=64, N=128, Cin=64)
    L = Launch(g)
    p = ProbeArgs()
    L.outputs(p)
    assert [NAMES[f] for f in BIG_TR if probe.gemm_probe_admits(f, 0, C.byref(p))] == ["big_tr_128"]


def test_every_family_runs(probe):
    # self-contained: one small admitted case per family (the other tests cover the shapes); no family id may go unexercised
    ran = set()
    ran |= set(run_case(probe, "coverage tiles", operands("bf16", M=300, N=256, Cin=64, seed=90), TILE_FAMILIES, expect_refused=[]))
    g = operands("bf16", M=64, N=64, Cin=1536, seed=91)
    ran |= set(run_case(probe, "coverage split-K", g, [F_SPLITK], ws_floats=2 * 64 * 64, ksplit=2, expect_refused=[]))
    g = operands("bf16", M=16, N=1024, Cin=1024, bias=False, seed=92)
    if run_skinny(probe, "coverage skinny", g, R.reference(g), lambda p, f: None, refused=False) is not None:
        ran.add(F_SKINNY)
    g = operands("bf16", M=16, N=1024, Cin=1024, bias=False, seed=93)
    if run_skinny(probe, "coverage skinny swiglu", g, R.swiglu_halves_ref(g), lambda p, f: None, refused=False, swiglu=True) is not None:
        ran.add(F_SKINNY_SWIGLU)
    ran |= set(_swiglu_halves(probe, 64, 512, 1024, "pair"))
    ran |= set(_resunit(probe, "bf16", 96, 200, 10))
    missing = [NAMES[f] for f in range(len(NAMES)) if f not in ran]
    assert not missing, f"families that never ran: {missing}"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_big_tile_on_second_device(probe):
    for dev_i in (0, 1):
        with torch.cuda.device(dev_i):
            for Cin in (128, 96):            # PAIR (Cin % 64 == 0) and the ring of four
                g = operands("bf16", M=600, N=512, Cin=Cin, res=True, seed=Cin)
                run_case(probe, f"big tile on device {dev_i} Cin {Cin}", g, [F_BIG_RING, F_BIG_PAIR, F_BIG_128, F_CONV_64x64],
                         expect_refused=[F_BIG_PAIR] if Cin % 64 else [])


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nfamily                      cases  max ulp  min exact")
    for name in sorted(STATS):
        st = STATS[name]
        print(f"{name:28s}{st['cases']:5d}  {st['max_ulp']:7.3f}  {st['min_exact']:.5f}")
