// Conformance probe of the PACKED continuation prefill kernels (csrc/prefill_kernels.cuh: qk_norm_rope_kv_cont_pack_kernel,
// flash_prefill_cont_pack_kernel, flash_cont_pack_merge_kernel): a shared library with a C ABI that launches exactly ONE named kernel on
// caller-owned device buffers, so that tests/test_gpu_prefill_pack_cont_reference.py can compare each of them with the float64 reference
// of tests/_prefill_cont_ref.py and, bit for bit, with the single-sequence kernels of prefill_cont_probe.hip.  It includes the product
// header (no attention code of its own) and never links into libfq3hip.so.
//
// Everything that describes the pack (start, cnt, rope deltas, forced splits, the block tables) arrives in HOST memory, so that it can
// be validated; the probe copies the tables to the device.  Anything that would make a kernel read or write outside the buffers the
// arguments describe is refused with kRefused and nothing is launched.
#include "../../faster-qwen3-tts_amd/csrc/prefill_kernels.cuh"
#include <cstddef>
using namespace fq3;

namespace {
constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;
enum Kind { K_NORM_PACK = 0, K_FLASH_PACK, K_MERGE_PACK, K_COUNT };
enum Te { TE_BF16 = 0, TE_F32 = 2 };          // the storage-type codes of the other probes
}  // namespace

extern "C" {

// qkv [qkv_rows][NH + 2 NKV][128] and out [qkv_rows][NH][128] hold the packed NEW rows (sequence q: rows off[q] .. off[q] + cnt[q], off the
// prefix sum of cnt); pools [n_blocks][NKV][64][128]; ws [ws_floats] the key-split records.  table holds the sequences' block tables
// back to back: sequence q's is table[toff[q] .. toff[q + 1]).  S == null: the launcher's rule (flash_cont_pack_splits) for n_cu CUs.
struct PackContProbeArgs {
    int NH, NKV;
    int n_seq;
    int qkv_rows;
    int rope_len;
    int n_blocks, n_table;
    int n_cu;
    long ws_floats;
    float eps, scale;
    void* qkv; const void* q_norm_w; const void* k_norm_w;
    const float* cos_tab; const float* sin_tab;
    void* kpool; void* vpool;
    void* out;
    float* ws;
    const int* start;               // HOST [n_seq]
    const int* cnt;                 // HOST [n_seq]
    const int* rope_delta;          // HOST [n_seq]
    const int* S;                   // HOST [n_seq] or null
    const int* toff;                // HOST [n_seq + 1]
    const int* table;               // HOST [n_table]
};

int pack_cont_probe_version() { return kProbeVersion; }
int pack_cont_probe_kinds() { return K_COUNT; }
int pack_cont_probe_refused_code() { return kRefused; }
int pack_cont_probe_record_floats() { return kFcRec; }
int pack_cont_probe_max_pack() { return kMaxPack; }
// the launcher's key-split rule (flash_cont_pack_splits) for a device of n_cu CUs; returns the floats of records, -1 when refused
long pack_cont_probe_splits(const int* start, const int* cnt, int n, int NH, int n_cu, long ws_floats, int* S) {
    if (!start || !cnt || !S || n < 1 || n > kMaxPack || NH < 1 || n_cu < 1 || ws_floats < 0) return -1;
    for (int q = 0; q < n; ++q)
        if (start[q] < 0 || cnt[q] < 1 || start[q] > (1 << 20) || cnt[q] > (1 << 20)) return -1;
    flash_cont_pack_splits(start, cnt, n, NH, n_cu, ws_floats, S);
    return flash_cont_pack_ws_floats(cnt, n, NH, S);
}

int pack_cont_probe_layout(long* out, int cap) {
#define P(f) (long)offsetof(PackContProbeArgs, f)
    const long v[] = {(long)sizeof(PackContProbeArgs), P(NH), P(NKV), P(n_seq), P(qkv_rows), P(rope_len), P(n_blocks), P(n_table), P(n_cu),
                      P(ws_floats), P(eps), P(scale), P(qkv), P(q_norm_w), P(k_norm_w), P(cos_tab), P(sin_tab), P(kpool), P(vpool), P(out),
                      P(ws), P(start), P(cnt), P(rope_delta), P(S), P(toff), P(table), (long)sizeof(PackCont)};
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

// the splits of this call: the forced ones, or the launcher's rule
void splits_of(const PackContProbeArgs& p, int* S) {
    if (p.S) for (int q = 0; q < p.n_seq; ++q) S[q] = p.S[q];
    else flash_cont_pack_splits(p.start, p.cnt, p.n_seq, p.NH, p.n_cu, p.ws_floats, S);
}

bool admits(int kind, int te, const PackContProbeArgs& p) {
    if ((te != TE_BF16 && te != TE_F32) || kind < 0 || kind >= K_COUNT) return false;
    if (kind != K_NORM_PACK && te != TE_BF16) return false;
    if (p.NH < 1 || p.NH > 64 || p.NKV < 1 || p.NH % p.NKV) return false;
    if (p.n_seq < 1 || p.n_seq > kMaxPack || !p.start || !p.cnt) return false;
    long rows = 0;
    for (int q = 0; q < p.n_seq; ++q) {
        if (p.start[q] < 0 || p.cnt[q] < 1 || p.start[q] > (1 << 20) || p.cnt[q] > (1 << 20)) return false;
        rows += p.cnt[q];
    }
    if (rows > p.qkv_rows) return false;
    if (kind != K_NORM_PACK) {
        if (!p.out || p.ws_floats < 0 || (!p.S && p.n_cu < 1)) return false;
        int S[kMaxPack];
        if (p.S) for (int q = 0; q < p.n_seq; ++q) if (p.S[q] < 1 || p.S[q] > kFcMaxSplit) return false;
        splits_of(p, S);
        const long rec = flash_cont_pack_ws_floats(p.cnt, p.n_seq, p.NH, S);
        if (rec > p.ws_floats || rec > 0x7fffffffL || (rec > 0 && !p.ws)) return false;
        if (kind == K_MERGE_PACK) return true;              // reads the records and writes out only
    }
    if (!p.qkv || !p.kpool || !p.vpool || !p.table || !p.toff || p.n_blocks < 1 || p.n_table < 1) return false;
    if (p.toff[0] != 0 || p.toff[p.n_seq] > p.n_table) return false;
    for (int q = 0; q < p.n_seq; ++q) {
        const int len = p.toff[q + 1] - p.toff[q];
        if (len < 0 || (p.start[q] + p.cnt[q] + kKeysPerTile - 1) / kKeysPerTile > len) return false;
    }
    for (int i = 0; i < p.n_table; ++i)
        if (p.table[i] < 0 || p.table[i] >= p.n_blocks) return false;
    if (kind == K_NORM_PACK) {
        if (!p.rope_delta) return false;
        for (int q = 0; q < p.n_seq; ++q)
            if (p.rope_delta[q] < -(1 << 24) || p.rope_delta[q] > (1 << 24)) return false;
        return p.q_norm_w && p.k_norm_w && p.cos_tab && p.sin_tab && p.rope_len >= 1;
    }
    return true;
}

template <typename T>
int run(int kind, const PackContProbeArgs& p, hipStream_t s) {
    const int NH = p.NH, NKV = p.NKV, per = NH + 2 * NKV, n = p.n_seq;
    int S[kMaxPack];
    if (kind == K_NORM_PACK) for (int q = 0; q < n; ++q) S[q] = 1;
    else splits_of(p, S);
    int* dtab = nullptr;
    if (kind != K_MERGE_PACK) {
        const size_t tbytes = sizeof(int) * (size_t)p.n_table;
        if (hipMalloc(&dtab, tbytes) != hipSuccess) return (int)hipGetLastError();
        if (hipMemcpy(dtab, p.table, tbytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dtab); return (int)hipGetLastError(); }
    }
    PackCont sq{};
    sq.n = n;
    int nqb_max = 0;
    for (int q = 0; q < n; ++q) {
        sq.table[q] = dtab ? dtab + p.toff[q] : nullptr; sq.off[q + 1] = sq.off[q] + p.cnt[q]; sq.start[q] = p.start[q];
        sq.rope_delta[q] = p.rope_delta ? p.rope_delta[q] : 0;
        sq.zoff[q + 1] = sq.zoff[q] + S[q];
        sq.wsoff[q] = q == 0 ? 0 : sq.wsoff[q - 1] + (S[q - 1] > 1 ? S[q - 1] * p.cnt[q - 1] * NH * kFcRec : 0);
        nqb_max = nqb_max > (p.cnt[q] + kFaQ - 1) / kFaQ ? nqb_max : (p.cnt[q] + kFaQ - 1) / kFaQ;
    }
    const int Lt = sq.off[n];
    PagedKV<T> kv{(T*)p.kpool, (T*)p.vpool, dtab, NKV * kKeysPerTile * kHeadDim};
    if (kind == K_NORM_PACK)
        hipLaunchKernelGGL((qk_norm_rope_kv_cont_pack_kernel<T>), dim3((Lt * per + 3) / 4), dim3(256), 0, s, (T*)p.qkv, (const T*)p.q_norm_w,
                           (const T*)p.k_norm_w, p.eps, p.cos_tab, p.sin_tab, p.rope_len, kv, sq, NH, NKV);
    else if constexpr (sizeof(T) == 2) {
        if (kind == K_FLASH_PACK)
            hipLaunchKernelGGL(flash_prefill_cont_pack_kernel, dim3(nqb_max, NH, sq.zoff[n]), dim3(256), 0, s, (const bf16_t*)p.qkv, kv, (bf16_t*)p.out,
                               p.ws, sq, NH, NKV, p.scale);
        else
            hipLaunchKernelGGL(flash_cont_pack_merge_kernel, dim3((Lt * NH + 1) / 2), dim3(256), 0, s, (const float*)p.ws, (bf16_t*)p.out, sq, NH);
    }
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);            // the tables are freed below: the launch must have finished with them
    if (dtab) (void)hipFree(dtab);
    return rc ? rc : rs;
}

}  // namespace

extern "C" {

int pack_cont_probe_admits(int kind, int te, const PackContProbeArgs* p) { return p && admits(kind, te, *p) ? 1 : 0; }

// launch exactly kernel `kind` and wait for it; returns the HIP error of the launch or the wait, or kRefused (nothing launched)
int pack_cont_probe_run(int kind, int te, const PackContProbeArgs* p, hipStream_t s) {
    if (!p || !admits(kind, te, *p)) return kRefused;
    return te == TE_F32 ? run<float>(kind, *p, s) : run<bf16_t>(kind, *p, s);
}

}  // extern "C"
