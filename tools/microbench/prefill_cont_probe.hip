// Conformance probe of the continuation prefill kernels (csrc/prefill_kernels.cuh: qk_norm_rope_kv_cont_kernel, prefill_attn_cont_kernel,
// flash_prefill_cont_kernel, flash_cont_merge_kernel): a shared library with a C ABI that launches exactly ONE named kernel on caller-owned
// device buffers, so that tests/test_gpu_prefill_cont_reference.py can compare each of them with the float64 reference of
// tests/_prefill_cont_ref.py.  It includes the product header (no attention code of its own) and never links into libfq3hip.so.
//
// The block table arrives in HOST memory, so that it can be validated; the probe copies it to the device.  Anything that would make a
// kernel read or write outside the buffers the arguments describe is refused with kRefused and nothing is launched.
#include "../../faster-qwen3-tts_amd/csrc/prefill_kernels.cuh"
#include <cstddef>
using namespace fq3;

namespace {
constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;
enum Kind { K_NORM_CONT = 0, K_WAVE_CONT, K_FLASH_CONT, K_MERGE, K_COUNT };
enum Te { TE_BF16 = 0, TE_F32 = 2 };          // the storage-type codes of the other probes
}  // namespace

extern "C" {

// qkv [qkv_rows][NH + 2 NKV][128] and out [qkv_rows][NH][128] hold the n NEW rows (local row t = position start + t); pools
// [n_blocks][NKV][64][128]; ws [ws_floats] the key-split records of K_FLASH_CONT with S > 1 and of K_MERGE.
struct ContProbeArgs {
    int NH, NKV;
    int start, n;
    int qkv_rows;
    int rope_len, rope_delta;
    int n_blocks, n_table;
    int S;
    long ws_floats;
    float eps, scale;
    void* qkv; const void* q_norm_w; const void* k_norm_w;
    const float* cos_tab; const float* sin_tab;
    void* kpool; void* vpool;
    void* out;
    float* ws;
    const int* table;               // HOST [n_table]
};

int cont_probe_version() { return kProbeVersion; }
int cont_probe_kinds() { return K_COUNT; }
int cont_probe_refused_code() { return kRefused; }
int cont_probe_record_floats() { return kFcRec; }
// the launcher's key-split rule (flash_cont_splits) for a device of n_cu CUs
int cont_probe_splits(int start, int n, int NH, int n_cu, long ws_floats) {
    if (start < 0 || n < 1 || NH < 1 || n_cu < 1) return 0;
    return flash_cont_splits(start, n, NH, n_cu, ws_floats);
}

int cont_probe_layout(long* out, int cap) {
#define P(f) (long)offsetof(ContProbeArgs, f)
    const long v[] = {(long)sizeof(ContProbeArgs), P(NH), P(NKV), P(start), P(n), P(qkv_rows), P(rope_len), P(rope_delta), P(n_blocks), P(n_table),
                      P(S), P(ws_floats), P(eps), P(scale), P(qkv), P(q_norm_w), P(k_norm_w), P(cos_tab), P(sin_tab), P(kpool), P(vpool), P(out),
                      P(ws), P(table)};
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

bool admits(int kind, int te, const ContProbeArgs& p) {
    if ((te != TE_BF16 && te != TE_F32) || kind < 0 || kind >= K_COUNT) return false;
    if ((kind == K_FLASH_CONT || kind == K_MERGE) && te != TE_BF16) return false;
    if (p.NH < 1 || p.NH > 64 || p.NKV < 1 || p.NH % p.NKV) return false;
    if (p.start < 0 || p.n < 1 || p.start > (1 << 20) || p.n > (1 << 20) || p.qkv_rows < p.n) return false;
    if (kind == K_MERGE) return p.out && p.ws && p.S >= 2 && p.S <= kFcMaxSplit && (long)p.S * p.n * p.NH * kFcRec <= p.ws_floats;
    if (!p.qkv || !p.kpool || !p.vpool || !p.table || p.n_blocks < 1 || p.n_table < 1) return false;
    if ((p.start + p.n + kKeysPerTile - 1) / kKeysPerTile > p.n_table) return false;
    for (int i = 0; i < p.n_table; ++i)
        if (p.table[i] < 0 || p.table[i] >= p.n_blocks) return false;
    if (kind == K_NORM_CONT)
        return p.q_norm_w && p.k_norm_w && p.cos_tab && p.sin_tab && p.rope_len >= 1 && p.rope_delta >= -(1 << 24) && p.rope_delta <= (1 << 24);
    if (!p.out) return false;
    if (kind == K_FLASH_CONT) {
        if (p.S < 1 || p.S > kFcMaxSplit) return false;
        if (p.S > 1 && (!p.ws || (long)p.S * p.n * p.NH * kFcRec > p.ws_floats)) return false;
    }
    return true;
}

template <typename T>
int run(int kind, const ContProbeArgs& p, hipStream_t s) {
    const int NH = p.NH, NKV = p.NKV, per = NH + 2 * NKV, n = p.n;
    if (kind == K_MERGE) {
        hipLaunchKernelGGL(flash_cont_merge_kernel, dim3((n * NH + 1) / 2), dim3(256), 0, s, (const float*)p.ws, (bf16_t*)p.out, n, NH, p.S);
        const int rc = (int)hipGetLastError(), rs = (int)hipStreamSynchronize(s);
        return rc ? rc : rs;
    }
    int* dtab = nullptr;
    const size_t tbytes = sizeof(int) * (size_t)p.n_table;
    if (hipMalloc(&dtab, tbytes) != hipSuccess) return (int)hipGetLastError();
    if (hipMemcpy(dtab, p.table, tbytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dtab); return (int)hipGetLastError(); }
    PagedKV<T> kv{(T*)p.kpool, (T*)p.vpool, dtab, NKV * kKeysPerTile * kHeadDim};
    if (kind == K_NORM_CONT)
        hipLaunchKernelGGL((qk_norm_rope_kv_cont_kernel<T>), dim3((n * per + 3) / 4), dim3(256), 0, s, (T*)p.qkv, (const T*)p.q_norm_w,
                           (const T*)p.k_norm_w, p.eps, p.cos_tab, p.sin_tab, p.rope_len, p.rope_delta, kv, p.start, n, NH, NKV);
    else if (kind == K_WAVE_CONT)
        hipLaunchKernelGGL((prefill_attn_cont_kernel<T>), dim3((n * NH + 3) / 4), dim3(256), 0, s, (const T*)p.qkv, kv, (T*)p.out, p.start, n, NH,
                           NKV, p.scale);
    else if constexpr (sizeof(T) == 2)
        hipLaunchKernelGGL(flash_prefill_cont_kernel, dim3((n + kFaQ - 1) / kFaQ, NH, p.S), dim3(256), 0, s, (const bf16_t*)p.qkv, kv, (bf16_t*)p.out,
                           p.ws, p.start, n, NH, NKV, p.scale, p.S);
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);            // the table is freed below: the launch must have finished with it
    (void)hipFree(dtab);
    return rc ? rc : rs;
}

}  // namespace

extern "C" {

int cont_probe_admits(int kind, int te, const ContProbeArgs* p) { return p && admits(kind, te, *p) ? 1 : 0; }

// launch exactly kernel `kind` and wait for it; returns the HIP error of the launch or the wait, or kRefused (nothing launched)
int cont_probe_run(int kind, int te, const ContProbeArgs* p, hipStream_t s) {
    if (!p || !admits(kind, te, *p)) return kRefused;
    return te == TE_F32 ? run<float>(kind, *p, s) : run<bf16_t>(kind, *p, s);
}

}  // extern "C"
