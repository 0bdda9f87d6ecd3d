"""Float64 references of the row kernels between the GEMM, attention and sampler launches (csrc/codec_kernels.cuh, the vector RMSNorm of
csrc/prefill_kernels.cuh, csrc/refenc_kernels.cuh), the cases the GPU test runs, and the judge both tests share.

Written from the comments above each kernel and the rounding contract of tests/_gemm_ref.py (one rounding to the storage type T, through
fp32, at each ``DT<T>::rnd`` / ``st``), not from the kernel bodies:

* rvq_gather / rvq_gather_new: per frame and half ([0, n_first) -> first, [n_first, nq) -> rest) the SEQUENTIAL sum of the codebook rows
  the codes name, rounded after every addition; the first term is taken as it is; an empty half stores 0.  _new: the code tensor holds
  the new frames only.  Bit-exact.
* prefix_rows / keep_rows: 16-byte copies between a pointer table and an utterance-major tensor.  Raw bits.
* rmsnorm_rows (and the vec form): y = rnd(w * rnd(x * rs)), rs = 1 / sqrt(mean(x^2) + eps) in fp32.
* layernorm_rows: y = rnd((x - mean) * rstd * w + b), biased variance, one rounding.
* dwconv7: causal, y[t][c] = rnd(sum_k w[c][k] x[t - 6 + k][c] + b[c]), rows before the utterance's first read as zero, one rounding.
* silu_mul: y = rnd(rnd(silu(g)) * u).  In fp32 1 + exp(-g) overflows for g < -88.7 and the quotient becomes 0: the true value there is
  below |g| / FLT_MAX (2.7e-37), which the bound grants as an absolute term, with one FLT_MIN for results that reach the denormals
  (the range of the number format, not a tolerance).
* rope_rows / rope_rows_pos: y0 = rnd(rnd(x0 cs) + rnd(-x1 sn)), y1 = rnd(rnd(x1 cs) + rnd(x0 sn)) on the q and k thirds, rotate_half pairs
  (j, j + HD / 2); position = row, or base[u] + row - row_lo.
* final_conv: pcm[t] = clamp(rnd(sum_{k, c} w[k][c] x[t - 6 + k][c] + b), -1, 1), zero outside the utterance's rows, fp32 out.
* snake_consts: a = rnd(exp(alpha)), ib = rnd(1 / rnd(rnd(exp(beta)) + 1e-9f)).
* conv_in: y = b + sum_k w[c][k] x[t - (K - 1) + k], e = ELU(y).  pad_rows: reflect (no edge repeat; clamped where T <= pad) or
  replicate, optionally the sum of two sources.  codebook_prepare: embed_sum / max(usage, eps), stored as [K][D] and [D][K].
  dft_mag: sqrt(re^2 + im^2 + 1e-9f).  col_stats: (softmax- or uniformly) weighted mean and sqrt(max(biased variance, eps)).
  se_scale: x * gate + res.
* rvq_encode: per (frame, level) the nearest codebook row, lowest index on equal distance; residual -= that row in fp32; part 0 = levels
  [0, n_sem) on columns [0, D), part 1 = levels [n_sem, nq) on columns [D, 2 D).

Every reference returns S, the scale of its sum, for the checker of _gemm_ref.py (TOL unchanged), and the flips of its earlier rounding
points as `extra`.  The bound is asked of every element of every case.  The exact fraction f is a statement about many elements, and
the cases here go down to one element: it is asked of every case of PER_CASE elements or more on its own, and of all cases of a kernel,
type, output and K together (Pool).  Two derivations restrict which elements count for it, both stated where they are made: layernorm
counts the elements whose sum cancels by at most two bits (S <= 4 |y|), silu_mul leaves out the gates whose exponential leaves fp32.

Outputs are described as whole buffers: NaN in `ref` = an element the kernel must not write (it keeps its bits);
NaN in an input = an element the kernel must not read (the NaN sentinel on the device)."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Optional

import torch

import _gemm_ref as G
from _gemm_ref import F64, rnd, rnd_trunc, ulp

NAN = float("nan")
F32_1E9 = float(torch.tensor(1e-9, dtype=torch.float32))
FLT_MAX = 3.4028234663852886e38
DTS = ("bf16", "bfs", "f32")
TE = {"bf16": 0, "bfs": 1, "f32": 2}
GUARD = 2
KINDS = ["rvq_gather", "rvq_gather_new", "prefix_rows", "keep_rows", "rmsnorm_rows", "rmsnorm_vec2", "rmsnorm_vec4", "layernorm_rows",
         "dwconv7", "silu_mul", "rope_rows_pos", "rope_rows", "final_conv", "snake_consts", "conv_in", "pad_rows", "codebook_prepare",
         "rvq_encode_1_1", "rvq_encode_1_2", "rvq_encode_4_1", "rvq_encode_4_2", "rvq_encode_4_4", "dft_mag", "col_stats", "se_scale"]
KIND = {k: i for i, k in enumerate(KINDS)}
N_CODEC = KIND["conv_in"]                         # kinds below: all three storage types; from here on fp32 only
ENC_KIND = {256: "rvq_encode_1_1", 512: "rvq_encode_1_2", 1024: "rvq_encode_4_1", 2048: "rvq_encode_4_2", 4096: "rvq_encode_4_4"}
ENC_VEC = {256: 1, 512: 1, 1024: 4, 2048: 4, 4096: 4}
ENC_PER = {256: 1, 512: 2, 1024: 1, 2048: 2, 4096: 4}


def esz(dt):
    return 2 if dt == "bf16" else 4


def final_spw(C, dt):
    """Mirror of final_conv_spw (codec_kernels.cuh): samples per workgroup and LDS bytes; the GPU test asserts it against the helper."""
    pitch = C + 16 // esz(dt)
    for spw in (256, 192, 128, 64):
        b = (((spw + 6) * pitch * esz(dt) + 15) & ~15) + 7 * C * 4
        if b <= 64 * 1024 or (spw == 64 and b <= 150 * 1024):
            return spw, b
    return 0, 0


# ---- raw bits <-> float64 ----------------------------------------------------------------------------------------------------
def encode(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 (NaN = sentinel) or int64 -> raw bits (int64) of format fmt (bf16 / bfs / f32 / i64)."""
    if fmt == "i64":
        return x.to(torch.int64)
    bits = G.raw_bits(G.to_storage(torch.nan_to_num(x, nan=0.0), fmt))
    return torch.where(torch.isnan(x), torch.full_like(bits, G.SENTINEL[fmt]), bits)


def decode(bits: torch.Tensor, fmt: str) -> torch.Tensor:
    if fmt == "i64":
        return bits.to(F64)
    if fmt == "bf16":
        return _bf16(bits)
    w = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    return G.from_storage(w.view(torch.float32) if fmt == "f32" else w, fmt)


def _bf16(bits):
    w = (bits & 0xFFFF) << 16
    w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    return w.view(torch.float32).to(F64)


# ---- the description of one launch ---------------------------------------------------------------------------------------------
@dataclass
class Out:
    ref: Optional[torch.Tensor] = None        # whole buffer, NaN = not written
    S: Optional[torch.Tensor] = None
    extra: Optional[torch.Tensor] = None
    mode: str = "check"                       # check (bound + exact fraction) | exact (equal bits of ref) | bits (equal raw bits `bits`)
    bits: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None       # written elements (default: ref is not NaN)
    init: Optional[str] = None                # the buffer is an input too (in place): what it held before
    store: Optional[str] = None               # storage format where it is not T (final_conv: f32)
    square: bool = False                      # col_stats: compare got^2 with ref (the variance)
    pre_clamp: Optional[torch.Tensor] = None  # final_conv: the value before the clamp
    K: Optional[int] = None
    frac: Optional[torch.Tensor] = None       # elements that count for the exact fraction (default: all written ones)


@dataclass
class Problem:
    kind: str
    dt: str
    K: int = 1
    bufs: dict = field(default_factory=dict)
    fmt: dict = field(default_factory=dict)   # name -> format where it is not T
    p: list = field(default_factory=list)     # (name, element offset) or None per pointer slot
    n: list = field(default_factory=list)
    f: list = field(default_factory=list)
    tab: dict = field(default_factory=dict)   # index -> (name, element offset)
    pos: list = field(default_factory=list)
    hc: Optional[str] = None
    outs: dict = field(default_factory=dict)
    enc: Optional[dict] = None                # rvq_encode: what the decision judge needs
    note: str = ""

    def fmt_of(self, name):
        if name in self.outs and self.outs[name].store:
            return self.outs[name].store
        return self.fmt.get(name, self.dt)

    def initial_bits(self, name):
        """What the device buffer `name` holds before the launch."""
        if name in self.bufs:
            b = self.bufs[name]
            return b.clone() if self.fmt.get(name) == "bits" else encode(b, self.fmt_of(name))
        o = self.outs[name]
        if o.init:
            return self.initial_bits(o.init)
        shape = (o.ref if o.ref is not None else o.bits).shape
        f = self.fmt_of(name)
        return torch.full(shape, -7 if f == "i64" else G.SENTINEL[f], dtype=torch.int64)

    def storage_fmt(self, name):
        f = self.fmt_of(name)
        return self.dt if f == "bits" else f


@dataclass
class Result:
    name: str
    ok: bool
    msg: str
    ratio: float = 0.0
    exact: float = 1.0
    n: int = 0
    near: int = 0
    decisions: int = 0
    n_exact: int = 0                          # of n_frac elements that count for the exact fraction, which must reach f
    n_frac: int = 0
    f: float = 0.0
    key: tuple = ()


def bound_of(ref, S, dt, K, extra):
    t = G.TOL[dt]
    c = t["c"] if t["c"] is not None else 8.0 * math.sqrt(max(K, 1)) * 2.0 ** -24
    return t["k"] * ulp(ref, dt) + c * S + (extra if extra is not None else 0.0)


# The bf16 floor f = 0.99 goes with an expectation of about one flipped rounding in 10^3 elements (_gemm_ref.py).  A fraction over n
# elements moves in steps of 1 / n: at n = 96 a single flip (expected in one case of ten) already falls below 0.99, at n = 1024 the
# floor allows 10 flips where 1 is expected (Poisson tail below 1e-8).  1024, the first power of two with a tenfold margin, is the size
# from which a case is asked on its own; smaller cases are asked through the pool only.  Not to be tuned to results.
PER_CASE = 1024


def need_f(dt, K):
    f = G.TOL[dt]["f"]
    return max(0.5, 0.9 - 0.004 * math.sqrt(K)) if f is None else f


class Pool:
    """The exact fraction over all cases of one (kernel, type, output, K): the cases are as small as one element, where a fraction
    says nothing, so the floor f of _gemm_ref.TOL is asked of each sizeable case and of the union."""

    def __init__(self):
        self.acc = {}

    def add(self, results):
        for r in results:
            if r.key and r.n_frac:
                a = self.acc.setdefault(r.key, [0, 0, r.f])
                a[0] += r.n_exact
                a[1] += r.n_frac

    def fraction(self, kind, dt):
        fr = [a[0] / a[1] for k, a in self.acc.items() if k[0] == kind and k[1] == dt]
        return min(fr) if fr else 1.0

    def failures(self):
        return [f"{k}: exact fraction {a[0] / a[1]:.5f} of {a[1]} elements over all cases (need {a[2]:.4f})"
                for k, a in self.acc.items() if a[0] < a[2] * a[1]]


def judge(pb: Problem, got: dict, fraction: bool = True) -> list:
    """got: name -> raw bits (int64) of every output buffer after the launch.  One Result per output."""
    if pb.enc is not None:
        return [judge_encode(pb, got["codes"])]
    res = []
    for name, o in pb.outs.items():
        f = pb.storage_fmt(name)
        gb = got[name]
        init = pb.initial_bits(name)
        mask = o.mask if o.mask is not None else ~torch.isnan(o.ref)
        what = f"{pb.kind} {pb.dt} {pb.note} [{name}]"
        if not torch.equal(gb[~mask], init[~mask]):
            res.append(Result(name, False, f"{what}: {int((gb[~mask] != init[~mask]).sum())} elements outside the kernel's range changed"))
            continue
        n = int(mask.sum())
        if o.mode == "bits":
            bad = int((gb[mask] != o.bits[mask]).sum())
            res.append(Result(name, bad == 0, f"{what}: {bad} / {n} elements differ in their bits", exact=1.0 - bad / max(n, 1), n=n))
            continue
        if o.mode == "exact":
            eb = encode(o.ref, f)
            bad = int((gb[mask] != eb[mask]).sum())
            res.append(Result(name, bad == 0, f"{what}: {bad} / {n} elements differ from the emulated bits", exact=1.0 - bad / max(n, 1), n=n))
            continue
        gv = decode(gb, f)[mask]
        if o.square:
            gv = gv * gv
        rv = o.ref[mask]
        S = o.S[mask]
        ex = o.extra[mask] if o.extra is not None else None
        K = o.K or pb.K
        v = G.check(gv.view(1, 1, -1), rv.view(1, 1, -1), S.view(1, 1, -1), pb.dt, K, what=what, extra=None if ex is None else ex.view(1, 1, -1), f=0.0)
        err = torch.nan_to_num((gv - rv).abs(), nan=float("inf"))
        ratio = float((err / bound_of(rv, S, pb.dt, K, ex)).max()) if n else 0.0
        ok, msg = v.ok, v.msg
        # the exact fraction is a statement about many elements: a case of PER_CASE elements or more must reach it on its own, and
        # all cases of a kernel, type and K together must reach it (Pool)
        f_need = 0.0 if o.square or not fraction else need_f(pb.dt, K)
        fm = o.frac[mask] if o.frac is not None else torch.ones_like(rv, dtype=torch.bool)
        n_frac, n_exact = int(fm.sum()), int((gv == rv)[fm].sum())
        if ok and n_frac >= PER_CASE and n_exact < f_need * n_frac:
            ok, msg = False, f"{what}: exact fraction {n_exact / n_frac:.5f} of {n_frac} elements (need {f_need:.4f})"
        if o.pre_clamp is not None:
            pc = o.pre_clamp[mask]
            sure = pc.abs() > 1.0 + bound_of(pc, S, pb.dt, K, ex)
            if bool((gv.abs() > 1.0).any()):
                ok, msg = False, f"{what}: a sample beyond [-1, 1]"
            elif not torch.equal(gv[sure], torch.sign(pc[sure])):
                ok, msg = False, f"{what}: a clamped sample is not exactly +/-1.0"
        res.append(Result(name, ok, msg, ratio, n_exact / n_frac if n_frac else 1.0, n, n_exact=n_exact, n_frac=n_frac, f=f_need,
                          key=(pb.kind, pb.dt, name, K)))
    return res


def as_got(pb: Problem) -> dict:
    """The reference's own outputs as device bits (mutants of the reference are judged through this)."""
    if pb.enc is not None:
        return {"codes": pb.enc["codes_out"]}
    out = {}
    for name, o in pb.outs.items():
        f = pb.storage_fmt(name)
        init = pb.initial_bits(name)
        mask = o.mask if o.mask is not None else ~torch.isnan(o.ref)
        val = o.bits if o.mode == "bits" else encode(torch.sqrt(o.ref) if o.square else o.ref, f)
        out[name] = torch.where(mask, val, init)
    return out


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()) & 0x7FFFFFFF)        # (hash() of a str changes per process)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def wide(g, dt, *shape, lo=-6, hi=6):
    """random values over a wide range of binades, T-representable"""
    e = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    return rnd(randn(g, *shape) * torch.pow(2.0, e), dt)


def guarded(x, before=GUARD, after=GUARD):
    """x [rows][...] between NaN guard rows; returns the buffer and the element offset of x's first row"""
    gb = torch.full((before,) + tuple(x.shape[1:]), NAN, dtype=F64)
    ga = torch.full((after,) + tuple(x.shape[1:]), NAN, dtype=F64)
    ld = int(torch.tensor(x.shape[1:]).prod()) if x.dim() > 1 else 1
    return torch.cat([gb, x, ga]), before * ld


def blank(rows, *rest):
    return torch.full((rows + 2 * GUARD,) + rest, NAN, dtype=F64)


def R_of(dt, mutant):
    if mutant == "trunc" and dt != "f32":
        return lambda x: rnd_trunc(x, dt)
    return lambda x: rnd(x, dt)


def uniq(xs):
    out = []
    for x in xs:
        if x not in out:
            out.append(x)
    return out


# ---- RVQ gather ---------------------------------------------------------------------------------------------------------------------
BOOK_ROWS = 7


def rvq_gather_cases():
    cs = []
    i = 0
    for nq in (1, 2, 16):
        for n_first in uniq((0, 1, nq)):
            for dim in (8, 256, 300):
                for Tn in (1, 5):
                    for row_lo in uniq((0, 2, Tn - 1)):
                        if row_lo >= Tn:
                            continue
                        cs.append(dict(nq=nq, n_first=n_first, dim=dim, Tn=Tn, row_lo=row_lo, NS=(1, 3)[i % 2], seed=i))
                        i += 1
    return cs


def seq_sum(rows, R, pairwise=False):
    """rows: list of [.., dim] float64 terms -> the sequential rounded sum (the first term unrounded); none: 0"""
    if not rows:
        return None
    if pairwise:
        while len(rows) > 1:
            rows = [R(rows[i] + rows[i + 1]) if i + 1 < len(rows) else rows[i] for i in range(0, len(rows), 2)]
        return rows[0]
    acc = rows[0]
    for e in rows[1:]:
        acc = R(acc + e)
    return acc


def rvq_gather(c, dt, new=False, mutant=""):
    nq, n_first, dim, Tn, row_lo, NS = c["nq"], c["n_first"], c["dim"], c["Tn"], c["row_lo"], c["NS"]
    g = gen("rvq", c["seed"])
    R = R_of(dt, mutant)
    pb = Problem("rvq_gather_new" if new else "rvq_gather", dt, K=nq, note=str(c))
    books = []
    for j in range(nq):         # big, -big, small (16 : 1, so that bf16 still sees the small term behind the big ones): any order of
        # summation other than the sequential one rounds differently
        mag, sign = (16.0, 16.0, 1.0)[j % 3], (1.0, -1.0, 1.0)[j % 3]
        b = rnd(sign * mag * (1.0 + 0.25 * torch.rand(BOOK_ROWS, dim, generator=g, dtype=F64)), dt)
        books.append(b)
        pb.bufs[f"book{j}"], off = guarded(b)
        pb.tab[j] = (f"book{j}", off)
    codes = torch.randint(0, BOOK_ROWS, (NS, Tn, nq), generator=g)
    codes[0, Tn - 1, 0], codes[NS - 1, Tn - 1, nq - 1] = 0, BOOK_ROWS - 1
    if nq == 1:
        codes[0, Tn - 1, 0] = 0 if NS > 1 else BOOK_ROWS - 1
    dev_codes = codes[:, row_lo:].contiguous() if new else codes
    pb.bufs["codes"], pb.fmt["codes"] = dev_codes.reshape(-1), "i64"
    pb.hc = "codes"
    nf = n_first + 1 if mutant == "n_first_off" else n_first
    first, rest = blank(NS * Tn, dim), blank(NS * Tn, dim)
    for u in range(NS):
        for t in range(row_lo, Tn):
            terms = [books[j][codes[u, t, j]] for j in range(nq)]
            if mutant == "drop_level" and nq > 1:
                terms = terms[:-1]
                fa, ra = terms[:min(nf, nq - 1)], terms[min(nf, nq - 1):]
            else:
                fa, ra = terms[:nf], terms[nf:]
            for buf, part in ((first, fa), (rest, ra)):
                s = seq_sum(list(part), R, pairwise=(mutant == "pairwise"))
                buf[GUARD + u * Tn + t] = torch.zeros(dim, dtype=F64) if s is None else s
    pb.p = [("codes", 0), ("first", GUARD * dim), ("rest", GUARD * dim)]
    pb.n = [nq, n_first, dim, Tn, row_lo, NS, BOOK_ROWS]
    pb.outs = {"first": Out(first, mode="exact"), "rest": Out(rest, mode="exact")}
    return pb


# ---- row copies --------------------------------------------------------------------------------------------------------------------
def copy_cases():
    cs = []
    i = 0
    for n_rows in (1, 3, 70):
        for nbytes in (16, 48, 512):
            for NS in (1, 3, 128):
                cs.append(dict(n_rows=n_rows, nbytes=nbytes, NS=NS, seed=i))
                i += 1
    return cs


def rand_bits(g, dt, *shape):
    """random bit patterns, NaN payloads included"""
    hi = 1 << (16 if dt == "bf16" else 32)
    return torch.randint(0, hi, shape, generator=g, dtype=torch.int64)


def copy_rows(c, dt, keep=False, mutant=""):
    n_rows, NS = c["n_rows"], c["NS"]
    epc = 16 // esz(dt)
    n_cols = c["nbytes"] // esz(dt)
    g = gen("copy", c["seed"], keep)
    sent = G.SENTINEL[dt]
    pb = Problem("keep_rows" if keep else "prefix_rows", dt, note=str(c))
    # the table side: one buffer, a segment per utterance; the tensor side: [NS][rows_per_utt][ld] between guard rows
    t_ld, t_off, t_rows = n_cols + 2 * epc, n_cols + 3 * epc, n_rows + 2            # t_off: row 1, column epc of the segment
    t_seg = t_rows * t_ld
    w_ld, w_col0, w_row0, w_rows = n_cols + 3 * epc, epc, 2, n_rows + 3
    w_seg = w_rows * w_ld
    table = rand_bits(g, dt, NS, t_rows, t_ld)
    work = rand_bits(g, dt, NS, w_rows, w_ld)
    guard = torch.full((GUARD, w_ld), sent, dtype=torch.int64)
    if keep:      # workspace rows -> the table's destinations
        exp = torch.full((NS, t_rows, t_ld), sent, dtype=torch.int64)
        mask = torch.zeros(NS, t_rows, t_ld, dtype=torch.bool)
        for u in range(NS):
            flat, mflat = exp[u].view(-1), mask[u].view(-1)
            for r in range(n_rows):
                src = work[u, w_row0 + r, w_col0:w_col0 + n_cols]
                if mutant == "row_off":
                    src = work[u, w_row0 + r - 1, w_col0:w_col0 + n_cols]
                flat[t_off + r * t_ld: t_off + r * t_ld + n_cols] = src
                mflat[t_off + r * t_ld: t_off + r * t_ld + n_cols] = True
        pb.bufs["src"], pb.fmt["src"] = torch.cat([guard, work.view(-1, w_ld), guard]), "bits"
        pb.p = [("src", GUARD * w_ld)]
        pb.tab = {u: ("dst", u * t_seg) for u in range(NS)}
        pb.n = [w_seg, w_ld, w_row0, w_col0, t_off, t_ld, n_rows, n_cols, NS, w_rows, t_seg]
        pb.outs = {"dst": Out(mode="bits", bits=exp, mask=mask)}
    else:         # the table's sources -> workspace rows
        exp = torch.full((NS, w_rows, w_ld), sent, dtype=torch.int64)
        mask = torch.zeros(NS, w_rows, w_ld, dtype=torch.bool)
        for u in range(NS):
            flat = table[u].view(-1)
            for r in range(n_rows):
                o = t_off + (r + (1 if mutant == "row_off" else 0)) * t_ld
                exp[u, w_row0 + r, w_col0:w_col0 + n_cols] = flat[o:o + n_cols] if o + n_cols <= flat.numel() else 0
                mask[u, w_row0 + r, w_col0:w_col0 + n_cols] = True
        gm = torch.zeros(GUARD, w_ld, dtype=torch.bool)
        pb.bufs["src"], pb.fmt["src"] = table.view(-1), "bits"
        pb.p = [("dst", GUARD * w_ld)]
        pb.tab = {u: ("src", u * t_seg) for u in range(NS)}
        pb.n = [t_off, t_ld, w_seg, w_ld, w_row0, w_col0, n_rows, n_cols, NS, w_rows, t_seg]
        pb.outs = {"dst": Out(mode="bits", bits=torch.cat([guard, exp.view(-1, w_ld), guard]), mask=torch.cat([gm, mask.view(-1, w_ld), gm]))}
    return pb


# ---- norms --------------------------------------------------------------------------------------------------------------------------
EPS = 1e-6
ROW_SETS = ("random", "equal", "offset", "zero")


def norm_cases(vec=0):
    cs = []
    i = 0
    if vec:
        for rows in (1, 3, 4, 5, 9):
            cs.append(dict(C=512 * vec, rows=rows, row_lo=0, NS=1, seed=i))
            i += 1
        return cs
    for C in (32, 64, 96, 1000):
        for rows in (1, 3, 4, 5, 9):
            for row_lo in uniq((0, 1, rows - 1)):
                if row_lo >= rows:
                    continue
                for NS in (1, 3):
                    cs.append(dict(C=C, rows=rows, row_lo=row_lo, NS=NS, seed=i))
                    i += 1
    return cs


def norm_rows_input(c, dt):
    """[NS * rows][C]: per row one of the operand sets (random wide-range, all equal, mean = 100 std, zero), rotating with the row,
    the utterance and the case; rows below row_lo hold NaN (not read)"""
    C, rows, NS = c["C"], c["rows"], c["NS"]
    g = gen("norm", c["seed"], C)
    x = torch.zeros(NS * rows, C, dtype=F64)
    for u in range(NS):
        for r in range(rows):
            kind = ROW_SETS[(r + u + c["seed"]) % 4]
            if kind == "random":
                v = wide(g, dt, C, lo=-4, hi=4)
            elif kind == "equal":       # moderate magnitude: at |x| = 2^12 the fp32 mean's own rounding would exceed eps in the variance
                v = rnd(torch.full((C,), 1.0 + 0.37 * (r + u), dtype=F64), dt)
            elif kind == "offset":
                v = rnd(100.0 + randn(g, C), dt)
            else:
                v = torch.zeros(C, dtype=F64)
            x[u * rows + r] = v if r >= c["row_lo"] else NAN
    w = rnd(1.0 + 0.5 * randn(g, C), dt)
    b = rnd(0.5 * randn(g, C), dt)
    return x, w, b


def rmsnorm(c, dt, kind="rmsnorm_rows", mutant=""):
    C, rows, row_lo, NS = c["C"], c["rows"], c["row_lo"], c["NS"]
    x, w, _ = norm_rows_input(c, dt)
    R = R_of(dt, mutant)
    pb = Problem(kind, dt, K=C, note=str(c))
    eps = 0.0 if mutant == "no_eps" else EPS
    ms = (x * x).sum(dim=1, keepdim=True) / C
    rs = rnd(1.0 / torch.sqrt(ms + eps), "f32")
    xs = R(x * rs)
    y = R(w * x * rs) if mutant == "gain_first" else R(w * xs)
    S = x.abs() * rs * w.abs()
    extra = ulp(xs, dt) * w.abs() if dt != "f32" else None
    pb.bufs["x"], off = guarded(x)
    pb.bufs["w"] = torch.cat([w, torch.full((8,), NAN, dtype=F64)])
    yb, _ = guarded(y)
    Sb, _ = guarded(torch.nan_to_num(S))
    pb.p = [("x", off), ("w", 0), ("y", off)]
    pb.n = [row_lo, rows, C, NS] if kind == "rmsnorm_rows" else [rows, C]
    pb.f = [EPS]
    pb.outs = {"y": Out(yb, Sb, None if extra is None else guarded(torch.nan_to_num(extra))[0])}
    return pb


def layernorm(c, dt, mutant=""):
    C, rows, row_lo, NS = c["C"], c["rows"], c["row_lo"], c["NS"]
    x, w, b = norm_rows_input(c, dt)
    R = R_of(dt, mutant)
    pb = Problem("layernorm_rows", dt, K=C, note=str(c))
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).sum(dim=1, keepdim=True) / (C - 1 if mutant == "c_minus_1" else C)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = R((x - mean) * rstd * w + b)
    S = (x.abs() + mean.abs()) * rstd * w.abs() + b.abs()
    pb.bufs["x"], off = guarded(x)
    pb.bufs["w"] = torch.cat([w, torch.full((8,), NAN, dtype=F64)])
    pb.bufs["b"] = torch.cat([b, torch.full((8,), NAN, dtype=F64)])
    pb.p = [("x", off), ("w", 0), ("b", 0), ("y", off)]
    pb.n = [row_lo, rows, C, NS]
    pb.f = [EPS]
    # The exact fraction counts the elements whose sum does not cancel by more than two bits (S <= 4 |y|): where x ~ mean (the
    # all-equal and the mean = 100 std rows) or (x - mean) rstd w ~ -b, the fp32 mean's own rounding, times S / |y|, exceeds an ulp of
    # T and no fp32 evaluation reproduces the rounding of the exact value.  Those elements are held to the bound, which carries S.
    # The factor 4: the kernel's value passes about four fp32 roundings (mean, difference, two products and the sum: ~4 * 2^-24 S),
    # a bf16 x 2 ulp is 2^-15 |y|, so a rounding flips with probability ~4 * 2^-24 S / (2^-15 |y|) = 2^-7 S / |y|; the floor
    # 0.9 - 0.004 sqrt(K) leaves 10 % to 23 % of flips, reached at S / |y| ~ 13 to 30, and 4 keeps a factor of three below that for
    # the fp32 mean's sqrt(C) term.  Derived from the formats, not from results; not to be tuned.
    frac = torch.nan_to_num(S) <= 4.0 * torch.nan_to_num(y).abs()
    pb.outs = {"y": Out(guarded(y)[0], guarded(torch.nan_to_num(S))[0], frac=guarded(frac.to(F64))[0] == 1.0)}
    return pb


# ---- dwconv7 ------------------------------------------------------------------------------------------------------------------------
def dwconv_cases():
    cs = []
    i = 0
    for C in (1, 24, 130):
        for rows in (1, 6, 7, 8, 40):
            for row_lo in uniq((0, 1, 6, 7, rows - 1)):
                if row_lo >= rows:
                    continue
                for NS in (1, 3):
                    cs.append(dict(C=C, rows=rows, row_lo=row_lo, NS=NS, set=("random", "tap")[i % 2], seed=i))
                    cs.append(dict(C=C, rows=rows, row_lo=row_lo, NS=NS, set=("tap", "random")[i % 2], seed=i + 1))
                    i += 2
    return cs


def dwconv7(c, dt, mutant=""):
    C, rows, row_lo, NS = c["C"], c["rows"], c["row_lo"], c["NS"]
    g = gen("dw", c["seed"])
    R = R_of(dt, mutant)
    pb = Problem("dwconv7", dt, K=7, note=str(c))
    if c["set"] == "tap":       # an impulse per channel at a known row, w[c][k] = 2^k: the output names the tap and the shift
        x = torch.zeros(NS, rows, C, dtype=F64)
        ch = torch.arange(C)
        for u in range(NS):
            x[u, (ch * 3 + u) % rows, ch] = 1.0 + u
        w = torch.pow(2.0, torch.arange(7, dtype=F64)).repeat(C, 1)
        b = torch.zeros(C, dtype=F64)
    else:
        x = wide(g, dt, NS, rows, C, lo=-3, hi=3)
        w = rnd(randn(g, C, 7), dt)
        b = rnd(randn(g, C), dt)
    wk = w.flip(1) if mutant == "taps_reversed" else w
    acc = torch.zeros(NS, rows, C, dtype=F64)
    S = b.abs().expand(NS, rows, C).clone()
    flat = x.view(NS * rows, C)
    for k in range(7):
        sh = 6 - k + (1 if mutant == "shift_row" else 0)          # y[t] += w[k] x[t - sh]
        xs = torch.zeros_like(x)
        if sh < rows:
            xs[:, sh:] = x[:, :rows - sh]
        if mutant == "prev_utt":
            for u in range(1, NS):
                for t in range(min(sh, rows)):
                    if u * rows + t - sh >= 0:
                        xs[u, t] = flat[u * rows + t - sh]
        acc += wk[:, k] * xs
        S += (wk[:, k] * xs).abs()
    y = R(acc + b)
    y[:, :row_lo] = NAN
    pb.bufs["x"], off = guarded(x.view(NS * rows, C))
    pb.bufs["w"], pb.bufs["b"] = w.reshape(-1), b
    pb.p = [("x", off), ("w", 0), ("b", 0), ("y", off)]
    pb.n = [row_lo, rows, C, NS]
    pb.outs = {"y": Out(guarded(y.view(NS * rows, C))[0], guarded(S.view(NS * rows, C))[0])}
    return pb


# ---- silu_mul ---------------------------------------------------------------------------------------------------------------------
def silu_cases():
    return [dict(rows=r, I=I, seed=i) for i, (r, I) in enumerate((r, I) for r in (1, 5) for I in (1, 24, 257))]


def silu_mul(c, dt, mutant=""):
    rows, I = c["rows"], c["I"]
    g = gen("silu", c["seed"])
    R = R_of(dt, mutant)
    pb = Problem("silu_mul", dt, K=1, note=str(c))
    gate = rnd((torch.rand(rows, I, generator=g, dtype=F64) * 200.0 - 100.0) * torch.pow(2.0, -torch.randint(0, 8, (rows, I), generator=g).to(F64)), dt)
    special = torch.tensor([0.0, -90.0, 90.0, -100.0, 100.0], dtype=F64)
    idx = torch.randperm(rows * I, generator=g)[:5]
    gate.view(-1)[idx] = special[:len(idx)]
    up = rnd(randn(g, rows, I) * 2.0, dt)
    sg = G.silu(gate)
    sq = sg if mutant == "no_inner_round" else R(sg)
    y = R(sq * up)
    S = (sq * up).abs()
    extra = ulp(sq, dt) * up.abs() + torch.where(-gate > math.log(FLT_MAX), gate.abs() / FLT_MAX * up.abs() * 2.0, torch.zeros_like(gate))
    # the bottom of the fp32 range: below 2^-110 the low half of a bf16 x 2 value, and below 2^-126 the value itself, is a denormal
    # (kept or flushed to zero, 2^-133 apart at best): one FLT_MIN per factor, absolute; such elements leave the exact fraction
    extra = extra + 2.0 ** -126 * (1.0 + up.abs())
    tiny = (sq * up).abs() < 2.0 ** -100
    gu = torch.cat([gate, up], dim=1)
    pb.bufs["gu"], off = guarded(gu)
    pb.p = [("gu", off), ("y", GUARD * I)]
    pb.n = [rows, I]
    # where 1 + exp(-g) leaves the fp32 range the result is an underflow, not a rounding: no part of the exact fraction
    pb.outs = {"y": Out(guarded(y)[0], guarded(S)[0], guarded(extra)[0], frac=guarded(((-gate <= math.log(FLT_MAX)) & ~tiny).to(F64))[0] == 1.0)}
    return pb


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------------
def rope_cases():
    cs = []
    i = 0
    for hd in (32, 64, 128):
        for NH in (1, 3):
            for rows in (1, 5, 9):
                for row_lo in uniq((0, 2, rows - 1)):
                    if row_lo >= rows:
                        continue
                    NS = (1, 3)[i % 2]
                    base = [0, 5, 1000] if NS == 3 else [(0, 5, 1000)[(i // 2) % 3]]
                    cs.append(dict(hd=hd, NH=NH, rows=rows, row_lo=row_lo, NS=NS, base=base, seed=i))
                    i += 1
    return cs


def rope_table(n_rows, half):
    """cos / sin of position * theta_j as fp32 values, NaN rows behind the last position"""
    pos = torch.arange(n_rows, dtype=F64)[:, None]
    theta = torch.pow(10000.0, -torch.arange(half, dtype=F64) / half)[None, :]
    pad = torch.full((GUARD, half), NAN, dtype=F64)
    return torch.cat([rnd(torch.cos(pos * theta), "f32"), pad]), torch.cat([rnd(torch.sin(pos * theta), "f32"), pad])


def rope(c, dt, plain=False, mutant=""):
    """plain: rope_rows_kernel (position = row) on the same data with base = row_lo for every utterance"""
    hd, NH, rows, row_lo, NS = c["hd"], c["NH"], c["rows"], c["row_lo"], c["NS"]
    base = [row_lo] * NS if plain or c.get("base_is_row_lo") else c["base"]
    QD, half = NH * hd, hd // 2
    g = gen("rope", c["seed"])
    R = R_of(dt, mutant)
    pb = Problem("rope_rows" if plain else "rope_rows_pos", dt, K=1, note=str(c))
    n_tab = max(base) + rows - row_lo           # the table ends exactly at the last position used
    ct, st = rope_table(n_tab, half)
    qkv = wide(g, dt, NS, rows, 3, NH, hd, lo=-3, hi=3)
    y = torch.full_like(qkv, NAN)
    S = torch.zeros_like(qkv)
    extra = torch.zeros_like(qkv)
    for u in range(NS):
        for t in range(row_lo, rows):
            pos = base[u] + t - row_lo
            if mutant == "pos_off":
                pos = min(pos + 1, n_tab - 1) if pos + 1 < n_tab else pos - 1
            if mutant == "base_ignored":
                pos = t - row_lo if max(base) > 0 else t + 1 if t + 1 < n_tab else 0
            cs, sn = ct[pos], st[pos]
            if mutant == "sign":
                sn = -sn
            thirds = (0,) if mutant == "k_alone" else (0, 1)
            for th in thirds:
                x0, x1 = qkv[u, t, th, :, :half], qkv[u, t, th, :, half:]
                a, b, cc, d = R(x0 * cs), R(-x1 * sn), R(x1 * cs), R(x0 * sn)
                y[u, t, th, :, :half], y[u, t, th, :, half:] = R(a + b), R(cc + d)
                S[u, t, th, :, :half], S[u, t, th, :, half:] = (x0 * cs).abs() + (x1 * sn).abs(), (x1 * cs).abs() + (x0 * sn).abs()
                if dt != "f32":
                    extra[u, t, th, :, :half], extra[u, t, th, :, half:] = ulp(a, dt) + ulp(b, dt), ulp(cc, dt) + ulp(d, dt)
            if mutant == "k_alone":
                y[u, t, 1] = NAN
    flat = lambda z: z.reshape(NS * rows, 3 * QD)
    pb.bufs["qkv"], off = guarded(flat(qkv))
    pb.bufs["cos"], pb.bufs["sin"] = ct, st
    pb.fmt["cos"] = pb.fmt["sin"] = "f32"
    pb.p = [("qkv", off), ("cos", 0), ("sin", 0)]
    pb.n = [rows, QD, hd, row_lo, NS, n_tab]
    pb.pos = list(base)
    pb.outs = {"qkv": Out(guarded(flat(y))[0], guarded(flat(S))[0], guarded(flat(extra))[0], init="qkv")}
    return pb


# ---- final_conv ----------------------------------------------------------------------------------------------------------------------
def final_conv_channels(dt):
    """8, 96, and the smallest C (a multiple of 8) at which final_conv_spw returns 192, 128, 64 and 64 above 64 KB of LDS"""
    cs = [8, 96]
    want = [(192, False), (128, False), (64, False), (64, True)]
    for spw_w, big in want:
        for C in range(8, 1025, 8):
            spw, b = final_spw(C, dt)
            if spw == spw_w and (b > 64 * 1024) == big:
                cs.append(C)
                break
        else:
            raise AssertionError((dt, spw_w, big))
    assert final_spw(8, dt)[0] == 256
    return cs


def final_conv_cases(dt):
    """Every chosen channel count with its own spw: rows in {1, 63, 64, 65, spw + 1, 2 spw + 5} x t_lo in {0, 1, 5, 6, 7, spw - 1, spw,
    rows - 1} (those below rows), each in all three operand sets and with 1 and 3 utterances."""
    cs = []
    i = 0
    for C in final_conv_channels(dt):
        spw = final_spw(C, dt)[0]
        for rows in uniq((1, 63, 64, 65, spw + 1, 2 * spw + 5)):
            for t_lo in uniq((0, 1, 5, 6, 7, spw - 1, spw, rows - 1)):
                if t_lo >= rows:
                    continue
                for s in ("random", "tap", "clamp"):
                    for NS in (1, 3):
                        cs.append(dict(C=C, rows=rows, t_lo=t_lo, NS=NS, set=s, seed=i))
                        i += 1
    return cs


def final_conv_operands(c, dt):
    C, rows, NS = c["C"], c["rows"], c["NS"]
    g = gen("fc", c["seed"])
    if c["set"] == "tap":       # one channel per row carries an impulse; w[k][c] = 2^(k - 8) (1 + (c % 3) / 4): the sum spells the taps
        x = torch.zeros(NS, rows, C, dtype=F64)
        t = torch.arange(rows)
        for u in range(NS):
            x[u, t, (t * 5 + u) % C] = 1.0
        w = torch.pow(2.0, torch.arange(7, dtype=F64) - 8.0)[:, None] * (1.0 + (torch.arange(C) % 3).to(F64) / 4.0)[None, :]
        b = torch.zeros(1, dtype=F64)
    else:
        sigma = 0.87 if c["set"] == "clamp" else 0.25           # P(|N(0, 0.87)| > 1) = 0.25
        x = rnd(randn(g, NS, rows, C), dt)
        w = rnd(randn(g, 7, C) * sigma / math.sqrt(7 * C), dt)
        b = rnd(randn(g, 1) * 0.05, dt)
    return x, w, b


def final_conv(c, dt, mutant=""):
    C, rows, t_lo, NS = c["C"], c["rows"], c["t_lo"], c["NS"]
    R = R_of(dt, mutant)
    x, w, b = final_conv_operands(c, dt)
    pb = Problem("final_conv", dt, K=7 * C, note=str(c))
    acc = torch.zeros(NS, rows, dtype=F64)
    S = torch.zeros(NS, rows, dtype=F64)
    for k in range(7):
        sh = 6 - k + (1 if mutant == "window_shift" else 0)
        xs = torch.zeros_like(x)
        if sh < rows:
            xs[:, sh:] = x[:, :rows - sh]
        acc += (xs * w[k]).sum(dim=2)
        S += (xs * w[k]).abs().sum(dim=2)
    bb = 0.0 if mutant == "no_bias" else b
    pre = R(acc + bb)
    y = pre if mutant == "no_clamp" else pre.clamp(-1.0, 1.0)
    S = S + b.abs()
    n_out = rows - t_lo
    pb.bufs["x"], off = guarded(x.view(NS * rows, C))
    pb.bufs["w"], pb.bufs["b"] = w.reshape(-1), torch.cat([b, torch.full((7,), NAN, dtype=F64)])
    g1 = lambda z: guarded(z[:, t_lo:].reshape(-1), 4, 4)[0]
    pb.p = [("x", off), ("w", 0), ("b", 0), ("pcm", 4)]
    pb.n = [t_lo, rows, C, NS]
    pb.outs = {"pcm": Out(g1(y), g1(S), store="f32", pre_clamp=g1(acc + bb))}
    return pb


def final_conv_f32_chain(c, dt):
    """float32 model of the stated chain: one fma chain in (tap, channel) order, bias, rounding, clamp.  (Each fma is emulated as the
    fp32 rounding of the float64 w * x + acc: a double rounding, exact except on rare ties.)  A record, not a reference."""
    C, rows, t_lo, NS = c["C"], c["rows"], c["t_lo"], c["NS"]
    x, w, b = final_conv_operands(c, dt)
    acc = torch.zeros(NS, rows, dtype=F64)
    for k in range(7):
        sh = 6 - k
        xs = torch.zeros_like(x)
        if sh < rows:
            xs[:, sh:] = x[:, :rows - sh]
        for ch in range(C):
            acc = (w[k, ch] * xs[:, :, ch] + acc).to(torch.float32).to(F64)
    v = rnd((acc + b).to(torch.float32).to(F64), dt).clamp(-1.0, 1.0)
    return v[:, t_lo:].reshape(-1)


# ---- snake_consts --------------------------------------------------------------------------------------------------------------------
def snake_cases():
    return [dict(C=1, seed=0), dict(C=300, seed=1)]


def snake_consts(c, dt, mutant=""):
    C = c["C"]
    g = gen("snake", c["seed"])
    R = R_of(dt, mutant)
    pb = Problem("snake_consts", dt, K=1, note=str(c))
    alpha = rnd(torch.rand(C, generator=g, dtype=F64) * 8.0 - 4.0, dt)
    beta = rnd(torch.rand(C, generator=g, dtype=F64) * 8.0 - 4.0, dt)
    beta[0] = -30.0             # exp(-30) = 9.4e-14: the 1e-9 decides the result
    a = R(torch.exp(alpha))
    bq = R(torch.exp(beta))
    bb = R(bq + (0.0 if mutant == "no_1e9" else F32_1E9))
    ib = R(1.0 / bb)
    extra = ib * (ulp(bq, dt) + ulp(bb, dt)) / bb if dt != "f32" else torch.zeros_like(ib)
    pad = lambda z: torch.cat([z, torch.full((8,), NAN, dtype=F64)])
    pb.bufs["alpha"], pb.bufs["beta"] = pad(alpha), pad(beta)
    pb.p = [("alpha", 0), ("beta", 0), ("a", 0), ("ib", 0)]
    pb.n = [C]
    pb.outs = {"a": Out(pad(a), pad(a.abs())), "ib": Out(pad(ib), pad(ib.abs()), pad(extra))}
    return pb


# ---- analysers (fp32) ----------------------------------------------------------------------------------------------------------------
def conv_in_cases():
    cs = []
    i = 0
    for K in (1, 7):
        for n in uniq((1, K - 1, K, 300)):
            if n < 1:
                continue
            for C in (1, 24):
                cs.append(dict(n=n, C=C, K=K, seed=i))
                i += 1
    return cs


def conv_in(c, dt="f32", mutant=""):
    n, C, K = c["n"], c["C"], c["K"]
    g = gen("cin", c["seed"])
    pb = Problem("conv_in", "f32", K=K, note=str(c))
    x = rnd(randn(g, n), "f32")
    w = rnd(randn(g, C, K), "f32")
    b = rnd(randn(g, C), "f32")
    acc = b.expand(n, C).clone()
    S = b.abs().expand(n, C).clone()
    for k in range(K):
        sh = K - 1 - k + (1 if mutant == "shift_row" else 0)
        xs = torch.zeros(n, dtype=F64)
        if sh < n:
            xs[sh:] = x[:n - sh]
        acc += xs[:, None] * w[None, :, k]
        S += (xs[:, None] * w[None, :, k]).abs()
    pb.bufs["x"], off = guarded(x)
    pb.bufs["w"], pb.bufs["b"] = w.reshape(-1), b
    pb.p = [("x", off), ("w", 0), ("b", 0), ("y", GUARD * C), ("e", GUARD * C)]
    pb.n = [n, C, K]
    pb.outs = {"y": Out(guarded(rnd(acc, "f32"))[0], guarded(S)[0]), "e": Out(guarded(rnd(G.elu(acc), "f32"))[0], guarded(S)[0])}
    return pb


def pad_cases():
    cs = []
    i = 0
    for mode in (0, 1):
        for pad in (0, 1, 3):
            for T in uniq((1, 2, pad, pad + 1, 50)):
                if T < 1:
                    continue
                for two in (False, True):
                    cs.append(dict(mode=mode, pad_l=pad, T=T, rows_out=T + 2 * pad, two=two, seed=i))
                    i += 1
    for T in (1, 2, 3, 50):            # the replicate form of the downsample
        cs.append(dict(mode=1, pad_l=2, T=T, rows_out=2 + 2 * ((T + 1) // 2), two=False, seed=i))
        i += 1
    return cs


def pad_index(r, pad_l, T, mode, edge_repeat=False):
    t = r - pad_l
    if mode == 0:
        if edge_repeat:                 # "symmetric": the mutant
            t = -t - 1 if t < 0 else t
            t = 2 * T - 1 - t if t >= T else t
        else:
            t = -t if t < 0 else t
            t = 2 * (T - 1) - t if t >= T else t
    return min(max(t, 0), T - 1)


def pad_rows(c, dt="f32", mutant=""):
    T, pad_l, rows_out, mode = c["T"], c["pad_l"], c["rows_out"], c["mode"]
    C, ld1, ld2, ldd = 5, 7, 6, 9
    g = gen("pad", c["seed"])
    pb = Problem("pad_rows", "f32", note=str(c))
    s1 = torch.full((T, ld1), NAN, dtype=F64)
    s2 = torch.full((T, ld2), NAN, dtype=F64)
    s1[:, :C], s2[:, :C] = wide(g, "f32", T, C), wide(g, "f32", T, C)
    idx = [pad_index(r, pad_l, T, mode, mutant == "edge_repeat") for r in range(rows_out)]
    dst = torch.full((rows_out, ldd), NAN, dtype=F64)
    dst[:, :C] = rnd(s1[idx, :C] + s2[idx, :C], "f32") if c["two"] else s1[idx, :C]
    pb.bufs["src1"], o1 = guarded(s1)
    pb.bufs["src2"], o2 = guarded(s2)
    pb.p = [("src1", o1), ("src2", o2) if c["two"] else None, ("dst", GUARD * ldd)]
    pb.n = [ld1, ld2, ldd, T, C, pad_l, rows_out, mode]
    pb.outs = {"dst": Out(guarded(dst)[0], mode="exact")}
    return pb


def codebook_cases():
    return [dict(K=3, D=5, seed=0), dict(K=256, D=8, seed=1)]


CB_EPS = 1e-5


def codebook_prepare(c, dt="f32", mutant=""):
    K, D = c["K"], c["D"]
    g = gen("cb", c["seed"])
    pb = Problem("codebook_prepare", "f32", K=1, note=str(c))
    es = rnd(randn(g, K, D) * 10.0, "f32")
    usage = rnd(torch.rand(K, generator=g, dtype=F64) * 20.0, "f32")
    usage[0], usage[K - 1] = 0.0, float(torch.tensor(1e-7, dtype=torch.float32))
    eps = float(torch.tensor(CB_EPS, dtype=torch.float32))
    emb = rnd(es / usage.clamp_min(0.0 if mutant == "no_clamp" else eps)[:, None], "f32")
    pb.bufs["es"], oe = guarded(es)
    pb.bufs["usage"] = torch.cat([usage, torch.full((4,), NAN, dtype=F64)])
    pb.p = [("es", oe), ("usage", 0), ("emb", GUARD * D), ("embT", GUARD * K)]
    pb.n = [K, D]
    pb.f = [CB_EPS]
    pb.outs = {"emb": Out(guarded(emb)[0], guarded(emb.abs())[0]), "embT": Out(guarded(emb.t().contiguous())[0], guarded(emb.t().abs().contiguous())[0])}
    return pb


def dft_cases():
    return [dict(F=F, NB=NB, seed=i) for i, (F, NB) in enumerate((F, NB) for F in (1, 5) for NB in (1, 33))]


def dft_mag(c, dt="f32", mutant=""):
    F, NB = c["F"], c["NB"]
    g = gen("dft", c["seed"])
    pb = Problem("dft_mag", "f32", K=1, note=str(c))
    spec = wide(g, "f32", F, 2 * NB, lo=-10, hi=4)
    spec[0, 0] = spec[0, NB] = 0.0
    spec[F - 1, NB - 1] = 0.0
    re, im = spec[:, :NB], spec[:, NB:]
    mag = torch.sqrt(re * re + im * im + (0.0 if mutant == "no_1e9" else F32_1E9))
    pb.bufs["spec"], off = guarded(spec)
    pb.p = [("spec", off), ("mag", GUARD * NB)]
    pb.n = [F, NB]
    pb.outs = {"mag": Out(guarded(rnd(mag, "f32"))[0], guarded(mag)[0])}
    return pb


def col_stats_cases():
    cs = []
    i = 0
    for T in (1, 15, 16, 17, 100):
        for C in (1, 64, 65, 130):
            for logits in (False, True):
                for eps in (0.0, 1e-12):
                    cs.append(dict(T=T, C=C, logits=logits, outs=("both", "mean", "std")[i % 3], eps=eps, seed=i))
                    i += 1
    # exp(80) = 5.5e34 still fits fp32, so within [-80, 80] the subtraction of the maximum cannot be seen: two cases with a logit of 100
    # (exp(100) does not fit) on top of that range
    cs.append(dict(T=17, C=65, logits=True, outs="both", eps=1e-12, seed=i, top=100.0))
    cs.append(dict(T=100, C=1, logits=True, outs="both", eps=0.0, seed=i + 1, top=100.0))
    return cs


def col_stats(c, dt="f32", mutant=""):
    T, C = c["T"], c["C"]
    ldx, ldl = C + 3, C + 1
    g = gen("cs", c["seed"])
    pb = Problem("col_stats", "f32", K=T, note=str(c))
    x = torch.full((T, ldx), NAN, dtype=F64)
    x[:, :C] = rnd(randn(g, T, C) * 3.0 + 1.0, "f32")
    x[:, 0] = 2.5                       # a constant column
    lg = torch.full((T, ldl), NAN, dtype=F64)
    lg[:, :C] = rnd(torch.rand(T, C, generator=g, dtype=F64) * 160.0 - 80.0, "f32")
    lg[0, :C] = c.get("top", 80.0)
    xv = x[:, :C]
    if c["logits"]:
        if mutant == "no_max":          # exp(80) overflows fp32
            e = torch.exp(lg[:, :C]).to(torch.float32)
            wgt = (e / e.sum(dim=0, keepdim=True)).to(F64)
        else:
            wgt = torch.softmax(lg[:, :C], dim=0)
    else:
        wgt = torch.full((T, C), 1.0 / T, dtype=F64)
    mu = (wgt * xv).sum(dim=0)
    var = (wgt * (xv - mu) ** 2).sum(dim=0)
    if mutant == "unbiased" and T > 1 and not c["logits"]:
        var = var * T / (T - 1)
    eps = float(torch.tensor(c["eps"], dtype=torch.float32))
    pad = lambda z: torch.cat([z, torch.full((4,), NAN, dtype=F64)])
    pb.bufs["x"], ox = guarded(x)
    pb.bufs["lg"], ol = guarded(lg)
    want_m, want_s = c["outs"] in ("both", "mean"), c["outs"] in ("both", "std")
    pb.p = [("x", ox), ("lg", ol) if c["logits"] else None, ("mean", 0) if want_m else None, ("std", 0) if want_s else None]
    pb.n = [ldx, ldl, T, C]
    pb.f = [c["eps"]]
    if want_m:
        pb.outs["mean"] = Out(pad(rnd(mu, "f32")), pad((wgt * xv.abs()).sum(dim=0)))
    if want_s:      # judged on the variance: a constant column must not go through a square root at 0
        pb.outs["std"] = Out(pad(var.clamp_min(eps)), pad((wgt * (xv.abs() + mu.abs()) ** 2).sum(dim=0)), square=True)
    return pb


def se_cases():
    return [dict(T=T, C=C, seed=i) for i, (T, C) in enumerate((T, C) for T in (1, 5) for C in (1, 70))]


def se_scale(c, dt="f32", mutant=""):
    T, C = c["T"], c["C"]
    ldx, ldr, ldy = C + 2, C + 5, C + 1
    g = gen("se", c["seed"])
    pb = Problem("se_scale", "f32", K=1, note=str(c))
    x, r, y, S = (torch.full((T, ld), NAN, dtype=F64) for ld in (ldx, ldr, ldy, ldy))
    x[:, :C], r[:, :C] = wide(g, "f32", T, C), wide(g, "f32", T, C)
    gate = rnd(torch.rand(C, generator=g, dtype=F64), "f32")
    res = 0.0 if mutant == "no_res" else r[:, :C]
    y[:, :C] = rnd(x[:, :C] * gate + res, "f32")
    S[:, :C] = (x[:, :C] * gate).abs() + r[:, :C].abs()
    pb.bufs["x"], ox = guarded(x)
    pb.bufs["r"], orr = guarded(r)
    pb.bufs["gate"] = torch.cat([gate, torch.full((4,), NAN, dtype=F64)])
    pb.p = [("x", ox), ("gate", 0), ("r", orr), ("y", GUARD * ldy)]
    pb.n = [ldx, ldr, ldy, T, C]
    pb.outs = {"y": Out(guarded(y)[0], guarded(torch.nan_to_num(S))[0])}
    return pb


# ---- rvq_encode ----------------------------------------------------------------------------------------------------------------------
def encode_cases():
    cs = []
    i = 0
    for D in (8, 32):
        for K in (256, 512, 1024, 2048, 4096):
            for nq in (1, 4, 16):
                j = i // 2              # one n_sem and T per (D, K, nq), the same for both operand sets
                for s in ("separated", "random"):
                    cs.append(dict(D=D, K=K, nq=nq, n_sem=(1, 2)[j % 2] if nq > 1 else 1, T=(1, 3)[(j // 2) % 2], set=s, seed=i))
                    i += 1
    for K in (256, 512, 1024, 2048, 4096):           # exact ties: the winning row of frame 0 twice
        for tie in ("next", "next_group", "waves", "waves_group"):
            if tie in ("next_group", "waves_group") and ENC_PER[K] == 1:
                continue
            cs.append(dict(D=8, K=K, nq=4, n_sem=2, T=3, set="tie", tie=tie, seed=i))
            i += 1
    return cs


def tie_pair(K, tie):
    """(i, duplicate) with i the lower index.  A code's owner: group i // (256 VEC), thread (i % (256 VEC)) // VEC"""
    vec = ENC_VEC[K]
    if tie == "next":
        return 5 * vec + vec - 1, 5 * vec + vec                     # neighbours in two threads (VEC = 1: adjacent threads)
    if tie == "next_group":
        return 5 * vec + 1, 5 * vec + 1 + 256 * vec                 # one thread, consecutive groups
    if tie == "waves":
        return 5 * vec, (5 + 128) * vec                             # waves 0 and 2
    return 200 * vec, 5 * vec + 256 * vec                           # wave 3 in group 0 holds the lower index, wave 0 in group 1 the other


def encode_operands(c):
    D, K, nq, T = c["D"], c["K"], c["nq"], c["T"]
    g = gen("enc", c["seed"])
    if c["set"] == "separated":
        # Level m of a quantizer group: the lattice {-1, 0, 1}^D (distinct rows: the base-3 digits of a permuted index, repeated along
        # D) scaled by 4^-m; the input is the exact sum of one row per level (two bits a level: exact in fp32 for DEPTH levels).  The
        # tail behind a level is below a third of its spacing, so the chosen row wins by a third of the spacing squared; behind the
        # last summed level the residual is exactly 0 and the all-zero row wins at distance 0.
        DEPTH = 10
        emb = []
        pw = 3 ** torch.arange(8)
        z = torch.zeros(T, 2 * D, dtype=F64)
        for lv in range(nq):
            part = 0 if lv < c["n_sem"] else 1
            m = lv - (0 if part == 0 else c["n_sem"])
            idx = (3280 + (torch.arange(K) - (K // 3 + lv)) * 7) % 6561          # row K / 3 + lv: digits 1 1 1 ..., the all-zero row
            e = ((idx[:, None] // pw[None, :]) % 3 - 1).to(F64).repeat(1, D // 8) * (4.0 ** -m if m < DEPTH else 1.0)
            emb.append(e)
            if m < DEPTH:
                for t in range(T):
                    z[t, part * D:(part + 1) * D] += e[int(torch.randint(0, K, (1,), generator=g))]
        proj = rnd(z, "f32")
        assert torch.equal(proj, z)
    else:
        emb = [rnd(randn(g, K, D), "f32") for _ in range(nq)]
        proj = rnd(randn(g, T, 2 * D) * 1.5, "f32")
        if c["set"] == "tie":
            i0, i1 = tie_pair(K, c["tie"])
            for part, lv in ((0, 0), (1, c["n_sem"])):
                emb[lv][i0] = emb[lv][i1] = proj[0, part * D:(part + 1) * D]
    return proj, emb


def encode_walk(c, proj, emb, codes=None, mutant=""):
    """Walks the levels in float64 distances on the fp32 residual.  codes given: follows them (the kernel's ids) and returns, per
    decision, (d64 of the id, d64 of the argmin, argmin); else follows the argmin (lowest index) and returns the codes."""
    D, K, nq, n_sem, T = c["D"], c["K"], c["nq"], c["n_sem"], c["T"]
    out = torch.zeros(T, nq, dtype=torch.int64)
    rows = []
    for t in range(T):
        for part in (0, 1):
            cols = slice((1 - part) * D, (2 - part) * D) if mutant == "halves_swapped" else slice(part * D, (part + 1) * D)
            res = proj[t, cols].clone()
            for lv in (range(0, n_sem) if part == 0 else range(n_sem, nq)):
                d = ((res[None, :] - emb[lv]) ** 2).sum(dim=1)
                best = int(torch.argmin(d))                       # torch.argmin: the first index of the minimum
                if mutant == "last_index":
                    best = int(torch.nonzero(d == d.min()).flatten()[-1])
                j = best if codes is None else int(codes[t, lv])
                ok_id = 0 <= j < K
                rows.append((t, lv, j, float(d[j]) if ok_id else float("inf"), float(d[best]), best))
                out[t, lv] = j
                if not ok_id:
                    break
                if mutant != "no_residual":
                    res = rnd(res - emb[lv][j], "f32")
    return out, rows


def encode_min_margin(c, proj, emb):
    """the smallest (d(runner-up) - d(winner)) / (c (d(runner-up) + d(winner))) over the decisions of a case (float64)"""
    D, nq, n_sem, T = c["D"], c["nq"], c["n_sem"], c["T"]
    cc = 8.0 * math.sqrt(D) * 2.0 ** -24
    worst = float("inf")
    for t in range(T):
        for part in (0, 1):
            res = proj[t, part * D:(part + 1) * D].clone()
            for lv in (range(0, n_sem) if part == 0 else range(n_sem, nq)):
                d = ((res[None, :] - emb[lv]) ** 2).sum(dim=1)
                two = torch.topk(d, 2, largest=False).values
                worst = min(worst, float((two[1] - two[0]) / (cc * (two[1] + two[0]))))
                res = rnd(res - emb[lv][int(torch.argmin(d))], "f32")
    return worst


def rvq_encode(c, dt="f32", mutant=""):
    D, K, nq, T = c["D"], c["K"], c["nq"], c["T"]
    proj, emb = encode_operands(c)
    pb = Problem(ENC_KIND[K], "f32", K=D, note=str(c))
    for lv in range(nq):
        pb.bufs[f"emb{lv}"], oe = guarded(emb[lv])
        pb.bufs[f"embT{lv}"], ot = guarded(emb[lv].t().contiguous())
        pb.tab[lv], pb.tab[32 + lv] = (f"emb{lv}", oe), (f"embT{lv}", ot)
    pb.bufs["proj"], op = guarded(proj)
    pb.p = [("proj", op), ("codes", GUARD * nq)]
    pb.n = [nq, c["n_sem"], K, D, T]
    codes, _ = encode_walk(c, proj, emb, mutant=mutant)
    full = torch.full(((T + 2 * GUARD) * nq,), -7, dtype=torch.int64)
    full[GUARD * nq:(GUARD + T) * nq] = codes.view(-1)
    pb.enc = dict(case=c, proj=proj, emb=emb, codes_out=full)
    pb.outs = {"codes": Out(ref=torch.zeros((T + 2 * GUARD) * nq, dtype=F64), store="i64")}
    return pb


def initial_codes(pb):
    c = pb.enc["case"]
    return torch.full(((c["T"] + 2 * GUARD) * c["nq"],), -7, dtype=torch.int64)


def judge_encode(pb, got):
    c = pb.enc["case"]
    nq, T = c["nq"], c["T"]
    what = f"{pb.kind} {pb.note}"
    init = initial_codes(pb)
    lo, hi = GUARD * nq, (GUARD + T) * nq
    if not (torch.equal(got[:lo], init[:lo]) and torch.equal(got[hi:], init[hi:])):
        return Result("codes", False, f"{what}: the guard rows of the codes changed")
    codes = got[lo:hi].view(T, nq)
    _, rows = encode_walk(c, pb.enc["proj"], pb.enc["emb"], codes=codes)
    cc = 8.0 * math.sqrt(c["D"]) * 2.0 ** -24
    near, bad = 0, []
    for t, lv, j, dj, db, best in rows:
        if j == best:
            continue
        if dj - db <= cc * (dj + db) and dj != db:      # an equal distance at another index is the tie rule broken, not a near tie
            near += 1
        else:
            bad.append((t, lv, j, best, dj, db))
    n = T * nq
    cap = 0 if c["set"] == "separated" else 0.02 * n
    ok = not bad and near <= cap and len(rows) == n
    return Result("codes", ok, f"{what}: wrong ids (frame, level, got, want, d(got), d(want)) {bad[:4]}, near ties {near} of {n} (cap {cap})",
                  near=near, decisions=n, n=n)


def encode_f32_model(c):
    """A float32 model of the scan (squared differences accumulated in ascending d, fp32): its ids, for the self-test's conditions."""
    proj, emb = encode_operands(c)
    D, K, nq, n_sem, T = c["D"], c["K"], c["nq"], c["n_sem"], c["T"]
    out = torch.zeros(T, nq, dtype=torch.int64)
    for t in range(T):
        for part in (0, 1):
            res = proj[t, part * D:(part + 1) * D].to(torch.float32)
            for lv in (range(0, n_sem) if part == 0 else range(n_sem, nq)):
                e = emb[lv].to(torch.float32)
                acc = torch.zeros(K, dtype=torch.float32)
                for d in range(D):
                    df = res[d] - e[:, d]
                    acc = (df.to(F64) * df.to(F64) + acc.to(F64)).to(torch.float32)
                j = int(torch.argmin(acc))
                out[t, lv] = j
                res = res - e[j]
    full = initial_codes(Problem("", "f32", enc=dict(case=c)))
    full[GUARD * nq:(GUARD + T) * nq] = out.view(-1)
    return full


# ---- the case list of the GPU test -------------------------------------------------------------------------------------------------
def _vec2(c, dt, mutant=""):
    return rmsnorm(c, dt, kind="rmsnorm_vec2", mutant=mutant)


def _vec4(c, dt, mutant=""):
    return rmsnorm(c, dt, kind="rmsnorm_vec4", mutant=mutant)


def _gather_new(c, dt, mutant=""):
    return rvq_gather(c, dt, new=True, mutant=mutant)


def _keep(c, dt, mutant=""):
    return copy_rows(c, dt, keep=True, mutant=mutant)


def _rope_plain(c, dt, mutant=""):
    return rope(c, dt, plain=True, mutant=mutant)


# test name -> (builder, cases(dt), storage types)
SUITE = {
    "rvq_gather": (rvq_gather, lambda dt: rvq_gather_cases(), DTS),
    "rvq_gather_new": (_gather_new, lambda dt: rvq_gather_cases(), DTS),
    "prefix_rows": (copy_rows, lambda dt: copy_cases(), DTS),
    "keep_rows": (_keep, lambda dt: copy_cases(), DTS),
    "rmsnorm_rows": (rmsnorm, lambda dt: norm_cases(), DTS),
    "rmsnorm_vec2": (_vec2, lambda dt: norm_cases(2), DTS),
    "rmsnorm_vec4": (_vec4, lambda dt: norm_cases(4), DTS),
    "layernorm_rows": (layernorm, lambda dt: norm_cases(), DTS),
    "dwconv7": (dwconv7, lambda dt: dwconv_cases(), DTS),
    "silu_mul": (silu_mul, lambda dt: silu_cases(), DTS),
    "rope_rows_pos": (rope, lambda dt: rope_cases(), DTS),
    "rope_rows": (_rope_plain, lambda dt: rope_cases(), DTS),
    "final_conv": (final_conv, final_conv_cases, DTS),
    "snake_consts": (snake_consts, lambda dt: snake_cases(), DTS),
    "conv_in": (conv_in, lambda dt: conv_in_cases(), ("f32",)),
    "pad_rows": (pad_rows, lambda dt: pad_cases(), ("f32",)),
    "codebook_prepare": (codebook_prepare, lambda dt: codebook_cases(), ("f32",)),
    "rvq_encode": (rvq_encode, lambda dt: encode_cases(), ("f32",)),
    "dft_mag": (dft_mag, lambda dt: dft_cases(), ("f32",)),
    "col_stats": (col_stats, lambda dt: col_stats_cases(), ("f32",)),
    "se_scale": (se_scale, lambda dt: se_cases(), ("f32",)),
}

# mutants that change a rounding to T only: they do not exist in fp32
ROUNDING_MUTANTS = ("trunc", "gain_first", "no_inner_round")
# the mutants of the reference the judge must reject on at least one case of SUITE (tests/test_rows_reference_cpu.py)
MUTANTS = {
    "rvq_gather": ("trunc", "pairwise", "n_first_off", "drop_level"),
    "prefix_rows": ("row_off",),
    "keep_rows": ("row_off",),
    "rmsnorm_rows": ("trunc", "no_eps", "gain_first"),
    "rmsnorm_vec2": ("trunc", "gain_first"),
    "layernorm_rows": ("trunc", "c_minus_1"),
    "dwconv7": ("trunc", "taps_reversed", "shift_row", "prev_utt"),
    "silu_mul": ("trunc", "no_inner_round"),
    "rope_rows_pos": ("trunc", "sign", "pos_off", "base_ignored", "k_alone"),
    "final_conv": ("trunc", "no_clamp", "no_bias", "window_shift"),
    "snake_consts": ("trunc", "no_1e9"),
    "conv_in": ("shift_row",),
    "pad_rows": ("edge_repeat",),
    "codebook_prepare": ("no_clamp",),
    "rvq_encode": ("last_index", "no_residual", "halves_swapped"),
    "dft_mag": ("no_1e9",),
    "col_stats": ("no_max", "unbiased"),
    "se_scale": ("no_res",),
}
