"""Voice library search: what one ``fq3_voices_search`` costs beside what a user would write today.

    python tools/voices_probe.py [--out profiles/voice_library.json]

Seeded random embeddings, D = 1024, N = 10 000 / 100 000 / 1 000 000, 1 / 8 / 32 queries, k = 1 / 16.  In the same process, alternated:
the search (three launches) against ``torch.topk(qn @ libn.T, k)`` on pre-normalised device tensors, and at the smallest N against
rows x N pair cosines through ``fq3_refenc_similarity``.  A sample is a window of several calls between two HIP events (20 calls, 5 at
a million rows), per call; 9 samples after a warm-up; the median with the smallest and largest sample beside it.  The library's bytes
over the search's time are compared with the 8 TB/s HBM peak this project measures against (that time includes the query pack and the
merge: it is a call's rate, not the scan kernel's; libraries of 10 000 and 100 000 rows -- 41 and 410 MB -- stay wholly or partly
in the 256 MB last-level cache between calls, so their rate is not an HBM figure).  Also: the scan variants -- slab sizes, and the
queries staged in LDS, which only tools/microbench/libvoices_variant.so builds -- at N = 100 000 and 1 000 000, D = 2048 with 1 / 16 /
32 queries, and the largest error against float64 for D = 16 / 64 / 1024.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")]

from fq3hip import _lib as L                                                # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def sampled(fns, reps, calls):
    """per form (median, min, max) of `reps` windows of `calls` calls each, the forms alternated window by window"""
    for _ in range(2):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(timed(f, calls))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def spread(t):
    return [round(t[1], 4), round(t[2], 4)]


class Lib:
    def __init__(self, raw):
        self.lib, self.h = L.load(), L.vp()
        L.check(self.lib.fq3_voices_create(raw.shape[1], raw.shape[0], C.byref(self.h)))
        assert self.lib.fq3_voices_add(self.h, raw.data_ptr(), raw.shape[0], torch.cuda.current_stream().cuda_stream) == 0
        self.idx = torch.empty(32, 16, dtype=torch.int32, device="cuda")
        self.cos = torch.empty(32, 16, dtype=torch.float32, device="cuda")

    def search(self, q, k):
        L.check(self.lib.fq3_voices_search(self.h, q.data_ptr(), q.shape[0], k, self.idx.data_ptr(), self.cos.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))

    def close(self):
        self.lib.fq3_voices_destroy(self.h)


def library(n, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    raw = torch.randn(n, dim, generator=g, device="cuda")
    q = raw[torch.arange(32, device="cuda") * (n // 32)] + 0.3 * torch.randn(32, dim, generator=g, device="cuda")
    return raw, q.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_library.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    lib_so = L.load()
    rows_out, variants, errors = [], [], []
    variant = C.CDLL(os.path.join(ROOT, "tools", "microbench", "libvoices_variant.so")).voices_variant_time
    variant.argtypes = [L.vp, C.c_long, C.c_int, L.vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, L.vp, L.vp, C.POINTER(C.c_float)]
    for n in (10000, 100000, 1000000):
        calls = 5 if n >= 1000000 else 20
        raw, q = library(n, 1024, n)
        vl = Lib(raw)
        libn = torch.nn.functional.normalize(raw, dim=1)
        for rows in (1, 8, 32):
            qr = q[:rows].contiguous()
            qn = torch.nn.functional.normalize(qr, dim=1)
            for k in (1, 16):
                fns = [lambda: vl.search(qr, k), lambda: torch.topk(qn @ libn.T, k)]
                if n == 10000:                                               # the pair cosines: rows x N of them, one launch per query
                    out = torch.empty(n, device="cuda")
                    pair = [qr[i: i + 1].expand(n, -1).contiguous() for i in range(rows)]
                    st = torch.cuda.current_stream().cuda_stream
                    fns.append(lambda: [L.check(lib_so.fq3_refenc_similarity(p.data_ptr(), raw.data_ptr(), n, 1024, out.data_ptr(), st)) for p in pair])
                t = sampled(fns, args.reps, calls)
                ms = [x[0] for x in t]
                want = torch.topk(qn.double() @ libn.double().T, k)
                vl.search(qr, k)
                torch.cuda.synchronize()
                row = dict(N=n, D=1024, queries=rows, k=k, search_ms=round(ms[0], 4), search_min_max_ms=spread(t[0]), matmul_topk_ms=round(ms[1], 4),
                           matmul_topk_min_max_ms=spread(t[1]),
                           matmul_topk_over_search=round(ms[1] / ms[0], 3), library_TBps_of_the_call=round(n * 4096 / (ms[0] * 1e-3) / 1e12, 3),
                           share_of_8TBps=round(n * 4096 / (ms[0] * 1e-3) / HBM_PEAK, 3),
                           same_indices_as_float64=bool(torch.equal(vl.idx.view(-1)[:rows * k].view(rows, k).long(), want.indices)))
                if n == 10000:
                    row["pair_cosines_ms"] = round(ms[2], 4)
                rows_out.append(row)
                print(row, flush=True)
        if n >= 100000:                                                      # the scan variants, built by the tool from the same kernels
            idx, cos, ms = torch.empty_like(vl.idx), torch.empty_like(vl.cos), (C.c_float * args.reps)()
            for rows, k in ((1, 1), (32, 16)):
                part = q[:rows].contiguous()
                vl.search(part, k)
                for slab, qlds in ((128, 0), (256, 0), (512, 0), (256, 1), (512, 1)):
                    rc = variant(raw.data_ptr(), n, 1024, part.data_ptr(), rows, k, slab // 128, qlds, args.reps, calls, idx.data_ptr(), cos.data_ptr(), ms)
                    assert rc == 0, rc
                    same = bool(torch.equal(idx.view(-1)[:rows * k], vl.idx.view(-1)[:rows * k]) and torch.equal(cos.view(-1)[:rows * k], vl.cos.view(-1)[:rows * k]))
                    variants.append(dict(N=n, D=1024, queries=rows, k=k, slab_rows=slab, query_lds=qlds, search_ms=round(statistics.median(ms), 4),
                                         search_min_max_ms=[round(min(ms), 4), round(max(ms), 4)], bit_identical_to_the_library=same))
                    print(variants[-1], flush=True)
        vl.close()
        del raw, libn, vl
        torch.cuda.empty_cache()
    raw, q = library(400000, 2048, 5)                                        # fp32 matrix rate or HBM?  32 queries against 16
    vl = Lib(raw)
    wide = []
    for rows in (1, 16, 32):
        part = q[:rows].contiguous()
        t = sampled([lambda: vl.search(part, 16)], args.reps, 5)[0]
        ms = t[0]
        wide.append(dict(N=400000, D=2048, queries=rows, k=16, search_ms=round(ms, 4), search_min_max_ms=spread(t), library_TBps_of_the_call=round(400000 * 8192 / (ms * 1e-3) / 1e12, 3),
                         mfma_TFLOPs_issued=round(2 * 400000 * 2048 * (32 if rows > 16 else 16) / (ms * 1e-3) / 1e12, 2)))
        print(wide[-1], flush=True)
    vl.close()
    del raw, vl
    torch.cuda.empty_cache()
    for dim in (16, 64, 1024):
        raw, q = library(10000, dim, 77 + dim)
        vl = Lib(raw)
        vl.search(q, 16)
        torch.cuda.synchronize()
        c64 = torch.nn.functional.normalize(q.double(), dim=1) @ torch.nn.functional.normalize(raw.double(), dim=1).T
        err = float((vl.cos.double() - torch.gather(c64, 1, vl.idx.long())).abs().max())
        errors.append(dict(D=dim, N=10000, queries=32, k=16, max_abs_error=err, bound=(dim + dim / 256 + 16) * 2.0 ** -24))
        print(errors[-1], flush=True)
        vl.close()
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               timing="a sample is a window of 20 calls (5 at N >= 400 000) between two HIP events, per call; median of the samples with [min, max] beside it; "
                      "the forms alternated window by window (the variants run one after the other inside the tool); the search's time is all three launches",
               cache_note="libraries of 41 MB (N = 10 000) and 410 MB (N = 100 000) stay wholly or partly in the 256 MB last-level cache between calls: "
                          "their bytes per second are not an HBM figure",
               fp32_matrix_peak_TFLOPs=157.3,
               hbm_peak_assumed_TBps=HBM_PEAK / 1e12, rows=rows_out, variants=variants, dim_2048=wide, error_against_float64=errors,
               not_measured=["kernel-only times", "real voices", "libraries above one device's memory"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
