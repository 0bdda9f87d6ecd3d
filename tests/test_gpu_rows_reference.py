"""Conformance of the vocoder's and the analysers' row kernels with the float64 references of tests/_rows_ref.py.

Each kernel is launched alone through tools/microbench/librows_probe.so with its call site's launch geometry.  Every output buffer is
filled with the NaN sentinel and has guard rows before and after; every element the kernel must not write is compared bit for bit
afterwards, every input is compared bit for bit too (unless it is the in-place output), and every input row the kernel must not read
holds the sentinel, so a NaN in an output is a finding.  Kernels with a batch axis run with 1 and 3 utterances of distinct data.
The cases are those of tests/_rows_ref.py (SUITE); tests/test_rows_reference_cpu.py shows that the judge rejects the listed mutants of
each reference on these very cases.

Bit-exact in all three storage types: rvq_gather, rvq_gather_new (and _new against the full form), prefix_rows, keep_rows (raw bits, NaN
payloads included), pad_rows, emb against embT of codebook_prepare, rope_rows_pos against rope_rows at base = row_lo.  Everything else:
|got - ref| <= k ulp_T(ref) + c S + extra and the exact fraction of _gemm_ref.TOL, unchanged.  rvq_encode: the id of every (frame, level)
must be the float64 argmin (lowest index on equal distance) or a near tie within c (d(j) + d(j*)), at most 2 % of a case's decisions and
none in the separated set; the reference continues from the kernel's id.

Arguments that would leave the buffers are refused by the probe's `admits` and asserted as refusals (test_refusals), never launched.

Observed on the MI355X (a record: no bound or floor is tuned to it).  "exact" = the fraction of elements equal to the emulated value
over all cases of the kernel and type (smallest over its outputs and K); it is asked of bf16 (0.99) and bf16 x 2 (0.9 - 0.004 sqrt(K))
only, the fp32 column is a record.
  kernel                  cases per type   largest err / bound (bf16, bfs, f32)   exact (bf16, bfs, f32)
  rvq_gather, _new                    96   bit-exact                              1, 1, 1
  prefix_rows, keep_rows              27   bit-exact                              1, 1, 1
  rmsnorm_rows                       104   0.0000  0.1920  0.0660                 1.00000  0.98320  0.76784
  rmsnorm_rows_vec<2>                  5   0.0000  0.1485  0.0145                 1.00000  0.98597  0.78414
  rmsnorm_rows_vec<4>                  5   0.0000  0.1895  0.0148                 1.00000  0.98295  0.76582
  layernorm_rows                     104   0.4781  0.1210  0.2616                 1.00000  0.99342  0.82665
  dwconv7                            192   0.0000  0.1210  0.1453                 1.00000  0.98776  0.76420
  silu_mul                             6   0.1333  0.1356  0.1410                 1.00000  0.97933  0.77264
  rope_rows_pos                       42   0.0000  0.2094  0.0833                 1.00000  0.99358  0.82423
  rope_rows (helper kind)             42   0.0000  0.1986  0.0833                 1.00000  0.99389  0.84306
  final_conv                        1152   0.4963  0.1165  0.0521                 0.99975  0.86898  0.44022
  snake_consts                         2   0.0000  0.0000  0.1395                 1.00000  1.00000  0.94020
  conv_in 12 cases 0.0905; pad_rows 48 bit-exact; codebook_prepare 2 bit-exact (IEEE division), emb = embT; dft_mag 4 cases 0.0827;
  col_stats 82 cases 0.1085 (on the variance); se_scale 4 cases 0.0000; rvq_encode 76 cases, 1016 decisions over the five
  instantiations: every id the float64 argmin, no near tie in any set, the lowest index on every exact tie.
  The vec kernels against rmsnorm_rows_kernel on the same rows: bf16 67584 of 67584 elements equal, bf16 x 2 67454 of 67584, fp32
  62325 of 67584 (only the order of the sum of squares differs).  final_conv against the float32 model of the stated chain (the
  one-utterance cases with C <= 128): 44130 of 44130 (bf16), 51957 of 51957 (bf16 x 2), 51957 of 51957 (fp32) samples equal bit for bit.
  final_conv runs the whole rows x t_lo list at each of its six channel counts (spw 256, 256, 192, 128, 64 and 64 above 64 KB of
  LDS), each pair in all three operand sets and with 1 and 3 utterances.
No case found a defect: no NaN, no touched sentinel, no element outside its bound, every bit identity held.  Three findings were errors
of a derivation, not of a kernel, and are stated where they are made in tests/_rows_ref.py: (1) the exact fraction says nothing of a
case of three elements, so it is asked per sizeable case and of all cases together; (2) in layernorm_rows an element whose sum cancels
(x ~ mean: the all-equal and mean = 100 std rows) cannot keep the rounding of the exact value through an fp32 mean, so the fraction
counts the elements with S <= 4 |y| (bf16 x 2 before that: 0.001 on such a row of 1000; the bound, which carries S, held throughout);
(3) silu_mul returns -0.0 at g = -90 where the exact value is -9e-38: 1 + exp(90) is beyond fp32, granted as |g| / FLT_MAX.
Also: exp(80) fits fp32, so the max subtraction of col_stats only shows beyond logits of [-80, 80]: two cases with a logit of 100.
"""
import ctypes as C
import os
from collections import defaultdict

import pytest
import torch

import _rows_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "librows_probe.so")
vp = C.c_void_p


class RowsArgs(C.Structure):
    _fields_ = [("p", vp * 8), ("tab", vp * 128), ("pos", C.c_int * 128), ("n", C.c_long * 16), ("f", C.c_float * 4),
                ("hc", C.POINTER(C.c_longlong))]


STATS = defaultdict(lambda: {"cases": 0, "ratio": 0.0, "min_exact": 1.0, "near": 0, "decisions": 0, "note": ""})
LAUNCHED = set()
POOL = R.Pool()
ESZ = {"bf16": 2, "bfs": 4, "f32": 4, "i64": 8}


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/librows_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.rows_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(RowsArgs), vp]
    lib.rows_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(RowsArgs)]
    lib.rows_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.rows_probe_final_spw.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_long)]
    assert lib.rows_probe_version() == 1 and lib.rows_probe_kinds() == len(R.KINDS)
    buf = (C.c_long * 16)()
    n = lib.rows_probe_layout(buf, 16)
    assert list(buf[:n]) == [C.sizeof(RowsArgs)] + [getattr(RowsArgs, f[0]).offset for f in RowsArgs._fields_]
    return lib


def to_device(bits, fmt):
    """raw bits (int64) -> the storage tensor on the device"""
    if fmt == "i64":
        return bits.cuda()
    if fmt == "bf16":
        return torch.where(bits >= (1 << 15), bits - (1 << 16), bits).to(torch.int16).cuda()
    return torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32).cuda()


def from_device(t, fmt):
    b = t.cpu().to(torch.int64)
    return b if fmt == "i64" else b & (0xFFFF if fmt == "bf16" else 0xFFFFFFFF)


class Launch:
    """One problem on the device: buffers, the argument block, the launch, the outputs as raw bits."""

    def __init__(self, pb):
        self.pb = pb
        self.init = {name: pb.initial_bits(name) for name in list(pb.bufs) + [n for n in pb.outs if n not in pb.bufs]}
        self.dev = {name: to_device(b, pb.storage_fmt(name)) for name, b in self.init.items()}
        a = RowsArgs()
        ptr = lambda ref: None if ref is None else self.dev[ref[0]].data_ptr() + ref[1] * ESZ[pb.storage_fmt(ref[0])]
        for i, ref in enumerate(pb.p):
            a.p[i] = ptr(ref)
        for i, ref in pb.tab.items():
            a.tab[i] = ptr(ref)
        for i, v in enumerate(pb.pos):
            a.pos[i] = v
        for i, v in enumerate(pb.n):
            a.n[i] = v
        for i, v in enumerate(pb.f):
            a.f[i] = v
        if pb.hc:
            host = pb.bufs[pb.hc].tolist()
            self.hc = (C.c_longlong * len(host))(*host)
            a.hc = C.cast(self.hc, C.POINTER(C.c_longlong))
        self.args = a

    def run(self, lib):
        pb = self.pb
        kind, te = R.KIND[pb.kind], R.TE[pb.dt]
        assert lib.rows_probe_admits(kind, te, C.byref(self.args)) == 1, f"{pb.kind} {pb.dt} {pb.note}: refused"
        torch.cuda.synchronize()
        rc = lib.rows_probe_run(kind, te, C.byref(self.args), None)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:       # a device fault: nothing more may run on this GPU in this session
            pytest.exit(f"{pb.kind} {pb.dt} {pb.note}: {e}", returncode=3)
        if rc != 0:
            pytest.exit(f"{pb.kind} {pb.dt} {pb.note}: launch returned HIP error {rc}", returncode=3)
        LAUNCHED.add((pb.kind, pb.dt))
        for name in pb.bufs:
            if name not in pb.outs:
                assert torch.equal(from_device(self.dev[name], pb.storage_fmt(name)), self.init[name]), f"{pb.kind} {pb.note}: input {name} changed"
        self.got = {name: from_device(self.dev[name], pb.storage_fmt(name)) for name in pb.outs}
        return self.got


def run_case(lib, pb, fails, key=None):
    la = Launch(pb)
    got = la.run(lib)
    st = STATS[key or (pb.kind, pb.dt)]
    st["cases"] += 1
    results = R.judge(pb, got)
    POOL.add(results)
    for r in results:
        if not r.ok:
            fails.append(r.msg)
        st["ratio"] = max(st["ratio"], r.ratio)
        st["min_exact"] = min(st["min_exact"], r.exact)
        st["near"] += r.near
        st["decisions"] += r.decisions
    return got


def written(pb, name):
    o = pb.outs[name]
    return o.mask if o.mask is not None else ~torch.isnan(o.ref)


@pytest.mark.parametrize("name", list(R.SUITE))
def test_kernel(probe, name):
    build, cases, dts = R.SUITE[name]
    fails = []
    for dt in dts:
        for c in cases(dt):
            pb = build(c, dt)
            got = run_case(probe, pb, fails)
            if name == "rvq_gather_new":            # the new frames alone = the full code tensor
                full = Launch(R.rvq_gather(c, dt)).run(probe)
                for out in ("first", "rest"):
                    if not torch.equal(full[out], got[out]):
                        fails.append(f"rvq_gather_new {dt} {c}: {out} differs from rvq_gather on the full codes")
            if name in ("rmsnorm_vec2", "rmsnorm_vec4"):   # the row-loop kernel on the same rows: both within the bound; equal elements counted
                pr = R.rmsnorm(c, dt)
                loop = run_case(probe, pr, fails, key=("rmsnorm_rows at C = %d" % c["C"], dt))
                m = written(pb, "y")
                st = STATS[(pb.kind, dt)]
                st["_eq"] = tuple(a + b for a, b in zip((int((loop["y"][m] == got["y"][m]).sum()), int(m.sum())), st.get("_eq", (0, 0))))
                st["note"] = "equal to rmsnorm_rows: %d of %d" % st["_eq"]
            if name == "rope_rows_pos":             # base = row_lo: rope_rows_kernel bit for bit
                c2 = dict(c, base_is_row_lo=True)
                a = Launch(R.rope(c2, dt)).run(probe)
                b = Launch(R.rope(c2, dt, plain=True)).run(probe)
                if not torch.equal(a["qkv"], b["qkv"]):
                    fails.append(f"rope_rows_pos {dt} {c}: differs from rope_rows at base = row_lo")
            if name == "codebook_prepare":
                K, D = c["K"], c["D"]
                e = got["emb"].reshape(-1)[R.GUARD * D:(R.GUARD + K) * D].view(K, D)
                eT = got["embT"].reshape(-1)[R.GUARD * K:(R.GUARD + D) * K].view(D, K)
                if not torch.equal(e.t(), eT):
                    fails.append(f"codebook_prepare {c}: emb and embT differ")
            if name == "final_conv":
                lds = C.c_long()
                assert (probe.rows_probe_final_spw(c["C"], R.TE[dt], C.byref(lds)), lds.value) == R.final_spw(c["C"], dt)
                if c["C"] <= 128 and c["NS"] == 1:          # a record: samples equal to the float32 model of the stated chain
                    model = R.encode(R.final_conv_f32_chain(c, dt), "f32")
                    g = got["pcm"][4:4 + model.numel()]
                    st = STATS[(pb.kind, dt)]
                    st["_eq"] = tuple(a + b for a, b in zip((int((g == model).sum()), model.numel()), st.get("_eq", (0, 0))))
                    st["note"] = "equal to the fp32 chain model: %d of %d" % st["_eq"]
    kinds = {name, "rmsnorm_rows"} if name.startswith("rmsnorm_vec") else {name}
    fails += [m for m in POOL.failures() if m.split("'")[1] in kinds]
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:12])


def test_refusals(probe):
    """What would leave the buffers is refused, not launched."""
    refused = probe.rows_probe_refused_code()

    def expect_refused(pb, change, what):
        la = Launch(pb)
        kind, te = R.KIND[pb.kind], R.TE[pb.dt]
        assert probe.rows_probe_admits(kind, te, C.byref(la.args)) == 1, what
        change(la)
        kind = getattr(la, "kind", kind)
        te = getattr(la, "te", te)
        assert probe.rows_probe_admits(kind, te, C.byref(la.args)) == 0, what
        assert probe.rows_probe_run(kind, te, C.byref(la.args), None) == refused, what
        torch.cuda.synchronize()
        for name in pb.outs:
            assert torch.equal(from_device(la.dev[name], pb.storage_fmt(name)), la.init[name]), what + ": something ran"

    def setn(i, v):
        def f(la):
            la.args.n[i] = v
        return f

    for dt in R.DTS:
        gc = R.rvq_gather_cases()[-1]
        for ident in (R.BOOK_ROWS, -1):
            def bad_code(la, ident=ident):
                la.hc[len(la.hc) - 1] = ident
            expect_refused(R.rvq_gather(gc, dt), bad_code, f"rvq_gather {dt}: code id {ident}")
            expect_refused(R.rvq_gather(gc, dt, new=True), bad_code, f"rvq_gather_new {dt}: code id {ident}")
        rc = R.rope_cases()[-1]

        def beyond(la):
            la.args.pos[len(la.pb.pos) - 1] += 1
        expect_refused(R.rope(rc, dt), beyond, f"rope_rows_pos {dt}: a position beyond the table")
        expect_refused(R.rope(rc, dt, plain=True), setn(5, rc["rows"] - 1), f"rope_rows {dt}: a table shorter than the rows")
        fc = R.final_conv_cases(dt)[0]
        expect_refused(R.final_conv(fc, dt), setn(2, 12), f"final_conv {dt}: C = 12")
        expect_refused(R.final_conv(fc, dt), setn(2, 4096), f"final_conv {dt}: C beyond the LDS")
        cc = R.copy_cases()[4]
        epc = 16 // R.esz(dt)
        for keep in (False, True):
            nm = "keep_rows" if keep else "prefix_rows"
            expect_refused(R.copy_rows(cc, dt, keep=keep), setn(7, cc["nbytes"] // R.esz(dt) - 1), f"{nm} {dt}: n_cols no multiple of 16 bytes")
            expect_refused(R.copy_rows(cc, dt, keep=keep), setn(5 if not keep else 3, epc + 1), f"{nm} {dt}: column offset no multiple of 16 bytes")
            expect_refused(R.copy_rows(cc, dt, keep=keep), setn(8, 129), f"{nm} {dt}: more utterances than the pointer table holds")
            expect_refused(R.copy_rows(cc, dt, keep=keep), setn(6, cc["n_rows"] + 2), f"{nm} {dt}: rows beyond the tensor")
    ec = R.encode_cases()[0]
    for K in (300, 128, 8192, 512):
        expect_refused(R.rvq_encode(ec), setn(2, K), f"rvq_encode: K = {K} in the K = 256 instantiation")

    def as_bf16(la):
        la.te = 0
    for name in ("conv_in", "pad_rows", "codebook_prepare", "rvq_encode", "dft_mag", "col_stats", "se_scale"):
        build, cases, _ = R.SUITE[name]
        expect_refused(build(cases("f32")[0], "f32"), as_bf16, f"{name}: the analysers are fp32 only")


def test_zz_summary():
    """Prints the record and asserts that every instantiation the probe builds was launched and that no pooled fraction misses."""
    want = {(k, dt) for i, k in enumerate(R.KINDS) for dt in (R.DTS if i < R.N_CODEC else ("f32",))}
    print()
    print(f"  {'kernel':34s} {'type':5s} {'cases':>6s}   {'largest err / bound':>20s}   {'exact fraction (pooled)':>24s}   note")
    for (kernel, dt), st in sorted(STATS.items(), key=lambda kv: (R.KIND.get(kv[0][0], 99), kv[0][0], R.TE[kv[0][1]])):
        note = st["note"]
        if st["decisions"]:
            note = f"near ties {st['near']} of {st['decisions']} decisions ({st['near'] / st['decisions']:.4%})"
        frac = POOL.fraction(kernel, dt) if (kernel, dt) in LAUNCHED else st["min_exact"]
        print(f"  {kernel:34s} {dt:5s} {st['cases']:6d}   {st['ratio']:20.4f}   {frac:24.5f}   {note}")
    assert LAUNCHED >= want, f"never launched: {sorted(want - LAUNCHED)}"
    assert not POOL.failures(), POOL.failures()
