// Conformance probe of the prefill and windowed attention kernels (csrc/prefill_kernels.cuh, csrc/codec_kernels.cuh,
// csrc/refenc_kernels.cuh): a shared library with a C ABI that launches exactly ONE named kernel on caller-owned device buffers, so that
// tests/test_gpu_prefill_attn_reference.py can compare each of them, key by key, with the float64 reference of
// tests/_prefill_attn_ref.py.  It includes the product headers (no attention code of its own; the one kernel below evaluates exp2f /
// expf on a grid for the reference's exponential constants) and never links into libfq3hip.so.
//
// Block tables and the per-sequence rows of a pack arrive in HOST memory, so that they can be validated; the probe copies the tables to
// the device and builds the by-value PackSeq from them.  Anything that would make a kernel read or write outside the buffers the
// arguments describe is refused with kRefused and nothing is launched.
#include "../../faster-qwen3-tts_amd/csrc/prefill_kernels.cuh"
#include "../../faster-qwen3-tts_amd/csrc/refenc_kernels.cuh"
#include <cstddef>
#include <cstring>
#include <vector>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;
constexpr int kLdsRefused = 100001;      // the device refused the 158 KB of dynamic LDS flash_prefill_small_kernel needs

enum Kind {
    K_NORM_KV = 0,      // qk_norm_rope_kv_kernel<T>, one sequence
    K_NORM_KV_PACK,     // qk_norm_rope_kv_pack_kernel<T>, n_seq sequences
    K_WAVE,             // prefill_attn_kernel<T>
    K_FLASH,            // flash_prefill_kernel<nw, paired>: <4,false>, <4,true>, <8,true> (bf16)
    K_FLASH_SMALL,      // flash_prefill_small_kernel, n_seq packed sequences (bf16)
    K_SWA,              // swa_attn_kernel<T, hd>, grid.z = n_batch
    K_WIN,              // win_attn_kernel<hd, np> (fp32)
    K_ROPE_ROWS,        // rope_rows_kernel<T>, grid.y = n_batch
    K_COUNT
};
enum Te { TE_BF16 = 0, TE_F32 = 2 };          // the storage-type codes of the GEMM probe

__global__ void exp_grid_kernel(const float* x, float* y, int n, int which) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = which == 0 ? exp2f(x[i]) : expf(x[i]);
}

}  // namespace

extern "C" {

// Everything one probe launch needs.  Device pointers unless marked HOST.
// Paged kinds: qkv [qkv_rows][NH + 2 NKV][128], out [qkv_rows][NH][128], pools [n_blocks][NKV][64][128]; sequence q of a pack owns
// packed rows [sum of the lengths before it, + seq_len[q]) and the table row table + q * n_table.  The single-sequence kinds read entry 0
// of seq_len / seq_n_pad / seq_rope_delta and table row 0.
// Windowed kinds: qkv [n_batch][Tn][3 * NH * hd], out [n_batch][Tn][NH * hd], cos_tab / sin_tab [Tn][hd / 2].
struct PrefillProbeArgs {
    int NH, NKV;
    int n_seq;                      // 1 for the single-sequence kinds
    int qkv_rows;                   // rows the qkv and out buffers hold
    int rope_len;                   // rows of cos_tab / sin_tab (64 floats each)
    int n_blocks, n_table;          // blocks in the pool, entries in every sequence's table
    int nw, paired;                 // K_FLASH
    int hd, np;                     // windowed kinds: head dim; K_WIN: passes of 64 keys
    int Tn, window, row_lo, n_batch;
    float eps, scale;
    void* qkv; const void* q_norm_w; const void* k_norm_w;
    const float* cos_tab; const float* sin_tab;
    void* kpool; void* vpool;
    void* out;
    const int* table;               // HOST [n_seq][n_table]
    const int* seq_len; const int* seq_n_pad; const int* seq_rope_delta;      // HOST [n_seq]
};

int prefill_probe_version() { return kProbeVersion; }
int prefill_probe_kinds() { return K_COUNT; }
int prefill_probe_refused_code() { return kRefused; }

// struct layout for the ctypes mirror: [sizeof PrefillProbeArgs, offsets of its fields in declaration order, sizeof PackSeq, kMaxPack,
// kFsMaxRows, kFsLdsBytes]; returns the number of values written
int prefill_probe_layout(long* out, int cap) {
#define P(f) (long)offsetof(PrefillProbeArgs, f)
    const long v[] = {(long)sizeof(PrefillProbeArgs),
                      P(NH), P(NKV), P(n_seq), P(qkv_rows), P(rope_len), P(n_blocks), P(n_table), P(nw), P(paired), P(hd), P(np), P(Tn),
                      P(window), P(row_lo), P(n_batch), P(eps), P(scale), P(qkv), P(q_norm_w), P(k_norm_w), P(cos_tab), P(sin_tab),
                      P(kpool), P(vpool), P(out), P(table), P(seq_len), P(seq_n_pad), P(seq_rope_delta),
                      (long)sizeof(PackSeq), (long)kMaxPack, (long)kFsMaxRows, (long)kFsLdsBytes};
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

bool is_windowed(int k) { return k == K_SWA || k == K_WIN || k == K_ROPE_ROWS; }
bool is_pack(int k) { return k == K_NORM_KV_PACK || k == K_FLASH_SMALL; }
bool is_norm(int k) { return k == K_NORM_KV || k == K_NORM_KV_PACK; }

bool admits(int kind, int te, const PrefillProbeArgs& p) {
    if ((te != TE_BF16 && te != TE_F32) || kind < 0 || kind >= K_COUNT) return false;
    if (p.NH < 1 || p.NH > 64) return false;
    if (is_windowed(kind)) {
        if (!p.qkv || !one_of<32, 64, 128>(p.hd) || p.Tn < 1 || p.Tn > (1 << 20) || p.n_batch < 1 || p.n_batch > 64) return false;
        if (p.row_lo < 0 || p.row_lo >= p.Tn) return false;
        if (kind == K_ROPE_ROWS) return p.cos_tab && p.sin_tab;
        if (!p.out || p.window < 1) return false;
        if (kind == K_SWA) return p.window <= 128;
        // K_WIN: fp32, one utterance, from row 0, every key of the window inside the np passes
        if (te != TE_F32 || p.n_batch != 1 || p.row_lo != 0 || !one_of<1, 2, 3, 4>(p.np)) return false;
        return (p.window < p.Tn ? p.window : p.Tn) <= 64 * p.np;
    }
    // the paged kinds
    if (p.NKV < 1 || p.NH % p.NKV || !p.qkv || !p.kpool || !p.vpool || !p.table || !p.seq_len || !p.seq_n_pad || !p.seq_rope_delta) return false;
    if ((kind == K_FLASH || kind == K_FLASH_SMALL) && te != TE_BF16) return false;
    if (kind == K_FLASH && !((p.nw == 4 && (p.paired == 0 || p.paired == 1)) || (p.nw == 8 && p.paired == 1))) return false;
    if (is_norm(kind) && (!p.q_norm_w || !p.k_norm_w || !p.cos_tab || !p.sin_tab || p.rope_len < 1)) return false;
    if (!is_norm(kind) && !p.out) return false;
    if (p.n_seq < 1 || p.n_seq > kMaxPack || (!is_pack(kind) && p.n_seq != 1)) return false;
    if (p.n_blocks < 1 || p.n_table < 1 || p.qkv_rows < 1) return false;
    long rows = 0;
    for (int q = 0; q < p.n_seq; ++q) {
        const int L = p.seq_len[q], n_pad = p.seq_n_pad[q];
        if (L < 1 || L > (1 << 20) || n_pad < 0 || n_pad >= L) return false;
        if (kind == K_FLASH_SMALL && L > kFsMaxRows) return false;
        if ((L + kKeysPerTile - 1) / kKeysPerTile > p.n_table) return false;
        if (p.seq_rope_delta[q] < -(1 << 24) || p.seq_rope_delta[q] > (1 << 24)) return false;
        rows += L;
    }
    if (rows > p.qkv_rows) return false;
    for (long i = 0; i < (long)p.n_seq * p.n_table; ++i)
        if (p.table[i] < 0 || p.table[i] >= p.n_blocks) return false;
    return true;
}

template <typename T>
int run_paged(int kind, const PrefillProbeArgs& p, hipStream_t s) {
    const int NH = p.NH, NKV = p.NKV, per = NH + 2 * NKV;
    int* dtab = nullptr;
    const size_t tbytes = sizeof(int) * (size_t)p.n_seq * p.n_table;
    if (hipMalloc(&dtab, tbytes) != hipSuccess) return (int)hipGetLastError();
    if (hipMemcpy(dtab, p.table, tbytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dtab); return (int)hipGetLastError(); }
    PagedKV<T> kv{(T*)p.kpool, (T*)p.vpool, dtab, NKV * kKeysPerTile * kHeadDim};
    PackSeq sq{};
    int Lmax = 0;
    sq.n = p.n_seq;
    for (int q = 0; q < p.n_seq; ++q) {
        sq.table[q] = dtab + (size_t)q * p.n_table; sq.off[q + 1] = sq.off[q] + p.seq_len[q];
        sq.n_pad[q] = p.seq_n_pad[q]; sq.rope_delta[q] = p.seq_rope_delta[q];
        Lmax = p.seq_len[q] > Lmax ? p.seq_len[q] : Lmax;
    }
    const int L = p.seq_len[0], n_pad = p.seq_n_pad[0], Lt = sq.off[sq.n];
    int rc = 0;
    switch (kind) {
        case K_NORM_KV:
            hipLaunchKernelGGL((qk_norm_rope_kv_kernel<T>), dim3((L * per + 3) / 4), dim3(256), 0, s, (T*)p.qkv, (const T*)p.q_norm_w,
                               (const T*)p.k_norm_w, p.eps, p.cos_tab, p.sin_tab, p.rope_len, p.seq_rope_delta[0], kv, L, n_pad, NH, NKV);
            break;
        case K_NORM_KV_PACK:
            hipLaunchKernelGGL((qk_norm_rope_kv_pack_kernel<T>), dim3((Lt * per + 3) / 4), dim3(256), 0, s, (T*)p.qkv, (const T*)p.q_norm_w,
                               (const T*)p.k_norm_w, p.eps, p.cos_tab, p.sin_tab, p.rope_len, kv, sq, NH, NKV);
            break;
        case K_WAVE:
            hipLaunchKernelGGL((prefill_attn_kernel<T>), dim3((L * NH + 3) / 4), dim3(256), 0, s, (const T*)p.qkv, kv, (T*)p.out, L, n_pad, NH,
                               NKV, p.scale);
            break;
        default:
            if constexpr (sizeof(T) == 2) {
                if (kind == K_FLASH && p.nw == 8) {
                    const int nqb = (L + 127) / 128;
                    hipLaunchKernelGGL((flash_prefill_kernel<8, true>), dim3((nqb + 1) / 2, NH), dim3(512), 0, s, (const bf16_t*)p.qkv, kv,
                                       (bf16_t*)p.out, L, n_pad, NH, NKV, p.scale, nqb);
                } else if (kind == K_FLASH) {
                    const int nqb = (L + 63) / 64;
                    if (p.paired) hipLaunchKernelGGL((flash_prefill_kernel<4, true>), dim3((nqb + 1) / 2, NH), dim3(256), 0, s, (const bf16_t*)p.qkv,
                                                     kv, (bf16_t*)p.out, L, n_pad, NH, NKV, p.scale, nqb);
                    else hipLaunchKernelGGL((flash_prefill_kernel<4, false>), dim3(nqb, NH), dim3(256), 0, s, (const bf16_t*)p.qkv, kv,
                                            (bf16_t*)p.out, L, n_pad, NH, NKV, p.scale, nqb);
                } else if (kind == K_FLASH_SMALL) {
                    if (!lds_limit_at_least<flash_prefill_small_kernel>(kFsLdsBytes)) rc = kLdsRefused;
                    else hipLaunchKernelGGL(flash_prefill_small_kernel, dim3((Lmax + kFaQ - 1) / kFaQ, NH, sq.n), dim3(256), kFsLdsBytes, s,
                                            (const bf16_t*)p.qkv, kv, (bf16_t*)p.out, sq, NH, NKV, p.scale);
                }
            }
            break;
    }
    if (rc == 0) rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);            // the tables are freed below: the launch must have finished with them
    if (rc == 0) rc = rs;
    (void)hipFree(dtab);
    return rc;
}

template <typename T>
int run_windowed(int kind, const PrefillProbeArgs& p, hipStream_t s) {
    const int QD = p.NH * p.hd;
    if (kind == K_ROPE_ROWS) {
        const size_t n = (size_t)(p.Tn - p.row_lo) * 2 * p.NH * (p.hd / 2);
        hipLaunchKernelGGL((rope_rows_kernel<T>), dim3((unsigned)((n + 255) / 256), p.n_batch), dim3(256), 0, s, (T*)p.qkv, p.cos_tab, p.sin_tab,
                           p.Tn, QD, p.hd, p.row_lo);
    } else if (kind == K_SWA) {
        const dim3 ag((p.Tn - p.row_lo + 3) / 4, p.NH, p.n_batch);
        with_value<32, 64, 128>(p.hd, [&](auto h) {
            hipLaunchKernelGGL((swa_attn_kernel<T, decltype(h)::value>), ag, dim3(256), 0, s, (const T*)p.qkv, (T*)p.out, p.Tn, p.NH, p.window,
                               p.scale, p.row_lo);
        });
    } else if constexpr (sizeof(T) == 4) {
        const dim3 ag((p.Tn + 3) / 4, p.NH);
        with_value<32, 64, 128>(p.hd, [&](auto h) {
            with_value<1, 2, 3, 4>(p.np, [&](auto n) {
                hipLaunchKernelGGL((win_attn_kernel<decltype(h)::value, decltype(n)::value>), ag, dim3(256), 0, s, (const float*)p.qkv,
                                   (float*)p.out, p.Tn, p.NH, p.window, p.scale);
            });
        });
    }
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);
    return rc ? rc : rs;
}

}  // namespace

extern "C" {

// 1 = these arguments stay inside the buffers they describe for kernel `kind` in storage type te (0 bf16, 2 fp32)
int prefill_probe_admits(int kind, int te, const PrefillProbeArgs* p) { return p && admits(kind, te, *p) ? 1 : 0; }

// launch exactly kernel `kind` and wait for it; returns the HIP error of the launch or the wait, or kRefused (nothing launched)
int prefill_probe_run(int kind, int te, const PrefillProbeArgs* p, hipStream_t s) {
    if (!p || !admits(kind, te, *p)) return kRefused;
    if (is_windowed(kind)) return te == TE_F32 ? run_windowed<float>(kind, *p, s) : run_windowed<bf16_t>(kind, *p, s);
    return te == TE_F32 ? run_paged<float>(kind, *p, s) : run_paged<bf16_t>(kind, *p, s);
}

// y[i] = exp2f(x[i]) (which 0: the flash kernels' exponential) or expf(x[i]) (which 1: win_attn_kernel's) for n device floats, for the
// reference's exponential constants (tests/_prefill_attn_ref.py)
int prefill_probe_exp(int which, const float* x, float* y, int n, hipStream_t s) {
    if (!x || !y || n <= 0 || (which != 0 && which != 1)) return kRefused;
    hipLaunchKernelGGL(exp_grid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n, which);
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);
    return rc ? rc : rs;
}

}  // extern "C"
