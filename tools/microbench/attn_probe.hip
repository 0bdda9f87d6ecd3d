// Conformance probe of the decode-time attention kernels (csrc/decode_kernels.cuh, csrc/batch_kernels.cuh): a shared library with a
// C ABI that launches exactly ONE named kernel (or kernel pair) on caller-owned device buffers, so that tests/test_gpu_attn_reference.py
// can compare each of them, key by key, with the float64 reference of tests/_attn_ref.py.  It includes the product headers (no attention
// code of its own; the one kernel below evaluates __expf on a grid for the reference's exp constant) and never links into libfq3hip.so.
//
// The probe, not the caller, builds what the batch kernels read from device memory: one zero-initialised DecodeState per lane with
// pos / done / n_pad set, the LaneTab / LaneKV / LaneTabs pointer tables, the block tables (passed in HOST memory, so that they can be
// validated), and the single-stream kernel's position / done words.  Anything that would make a kernel read or write outside the
// buffers the arguments describe is refused with kRefused and nothing is launched.
#include "../../faster-qwen3-tts_amd/csrc/batch_kernels.cuh"
#include <cstddef>
#include <cstring>
#include <vector>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;

enum Kind {
    K_SPLIT = 0,        // attn_decode_kernel<T, REP, PAGED>, grid (n_kv, workers) -> partial slots
    K_MERGE,            // combine_batch_kernel<T> on given partials -> out
    K_MERGE_GEMV,       // gemv_kernel<T, NCH, PRO_COMBINE, EPI_STORE> through the identity weight `ident` -> out
    K_PRED,             // attn_pred_kernel<T>, grid (n_kv * rep)
    K_PRED_BATCH,       // attn_pred_batch_kernel<T>, grid (n_kv * rep, lanes)
    K_PRED_GROUP,       // attn_pred_group_batch_kernel<T, REP>, grid (n_kv, lanes)
    K_BATCH_SPLIT,      // attn_decode_batch_kernel<T, REP>, grid (n_kv, workers, lanes), then combine_batch_kernel<T>
    K_LANE,             // attn_decode_lane_kernel<T, REP, NI>, grid (n_kv, lanes)
    K_COUNT
};
enum Te { TE_BF16 = 0, TE_F32 = 2 };          // the storage-type codes of the GEMM probe
enum Flags { FL_POS_PTR = 1, FL_DONE_PTR = 2 };

__global__ void expf_grid_kernel(const float* x, float* y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __expf(x[i]);
}

}  // namespace

extern "C" {

// Everything one probe launch needs.  Device pointers unless marked HOST.  Lane l of a batch kind reads qkv + l * qkv_stride, the RoPE
// row rope + l * 128 (cos[64] | sin[64]), its own cache (contiguous [n_kv][max_seq][128]) or block pool ([n_blocks][n_kv][64][128]) at
// kcache / vcache + l * kv_lane_stride, partial slots at part + l * part_stride, and writes out + l * out_stride.
struct AttnProbeArgs {
    int n_kv, rep, max_seq;
    int workers;                    // split: grid.y; merge kinds: n_part
    int paged;                      // K_SPLIT only (the batch split and the lane kernel are always paged, the predictor never)
    int ni;                         // K_LANE: 2 or 4
    int n_lanes;                    // 1 for the single-stream kinds
    int n_blocks, n_table;          // paged: blocks in every lane's pool, entries in every lane's table
    int qkv_stride, out_stride;     // elements
    int flags;                      // K_SPLIT: FL_POS_PTR (position through pos_ptr), FL_DONE_PTR (done through done_ptr; else it must be 0)
    float eps, scale;
    long kv_lane_stride;            // elements
    long part_stride;               // floats
    const void* qkv; const void* q_norm_w; const void* k_norm_w;
    const float* rope;
    void* kcache; void* vcache;
    float* part; void* out;
    const void* ident;              // K_MERGE_GEMV: T[q_dim][q_dim]
    const int* table;               // HOST [n_lanes][n_table]
    const int* pos; const int* done; const int* n_pad;      // HOST [n_lanes]
};

int attn_probe_version() { return kProbeVersion; }
int attn_probe_kinds() { return K_COUNT; }
int attn_probe_refused_code() { return kRefused; }

// struct layout for the ctypes mirror: [sizeof AttnProbeArgs, offsets of its fields in declaration order, sizeof AttnArgs,
// sizeof DecodeState, kMaxLanes, kMaxWorkers, kPartStride]; returns the number of values written
int attn_probe_layout(long* out, int cap) {
#define P(f) (long)offsetof(AttnProbeArgs, f)
    const long v[] = {(long)sizeof(AttnProbeArgs),
                      P(n_kv), P(rep), P(max_seq), P(workers), P(paged), P(ni), P(n_lanes), P(n_blocks), P(n_table), P(qkv_stride),
                      P(out_stride), P(flags), P(eps), P(scale), P(kv_lane_stride), P(part_stride), P(qkv), P(q_norm_w), P(k_norm_w),
                      P(rope), P(kcache), P(vcache), P(part), P(out), P(ident), P(table), P(pos), P(done), P(n_pad),
                      (long)sizeof(AttnArgs), (long)sizeof(DecodeState), (long)kMaxLanes, (long)kMaxWorkers, (long)kPartStride};
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

bool is_pred(int k) { return k == K_PRED || k == K_PRED_BATCH || k == K_PRED_GROUP; }
bool is_merge(int k) { return k == K_MERGE || k == K_MERGE_GEMV; }
bool is_batch(int k) { return k == K_MERGE || k == K_PRED_BATCH || k == K_PRED_GROUP || k == K_BATCH_SPLIT || k == K_LANE; }
bool is_paged(int k, const AttnProbeArgs& p) { return k == K_BATCH_SPLIT || k == K_LANE || (k == K_SPLIT && p.paged); }

bool admits(int kind, int te, const AttnProbeArgs& p) {
    if ((te != TE_BF16 && te != TE_F32) || kind < 0 || kind >= K_COUNT) return false;
    if (p.n_kv < 1 || p.n_kv > 64 || !one_of<1, 2, 4>(p.rep)) return false;
    if (p.n_lanes < 1 || p.n_lanes > kMaxLanes || (!is_batch(kind) && p.n_lanes != 1)) return false;
    const long q_dim = (long)p.n_kv * p.rep * kHeadDim;
    if (!p.out && kind != K_SPLIT) return false;
    if (kind != K_SPLIT && (p.out_stride % 8 || p.out_stride < q_dim)) return false;
    const bool parts = kind == K_SPLIT || kind == K_BATCH_SPLIT || is_merge(kind);
    if (parts) {
        if (p.workers < 1 || p.workers > kMaxWorkers || !p.part) return false;
        if (p.part_stride % 4 || p.part_stride < (long)p.n_kv * kMaxWorkers * p.rep * kPartStride) return false;
    }
    if (is_merge(kind)) {
        if (kind == K_MERGE_GEMV && (!p.ident || q_dim > 2048 || gemv_chunks((int)q_dim, 4) == 0)) return false;
        return true;
    }
    // the attention kinds: token, gains, RoPE rows, cache, positions
    if (!p.qkv || !p.q_norm_w || !p.k_norm_w || !p.rope || !p.kcache || !p.vcache || !p.pos || !p.done || !p.n_pad) return false;
    if (p.qkv_stride % 8 || p.qkv_stride < q_dim + 2L * p.n_kv * kHeadDim) return false;
    if (p.max_seq < 1) return false;
    const int n_tiles = (p.max_seq + kKeysPerTile - 1) / kKeysPerTile;
    const bool paged = is_paged(kind, p);
    const long lane_elems = paged ? (long)p.n_blocks * p.n_kv * kKeysPerTile * kHeadDim : (long)p.n_kv * p.max_seq * kHeadDim;
    if (p.n_lanes > 1 && (p.kv_lane_stride % 8 || p.kv_lane_stride < lane_elems)) return false;
    if (kind == K_LANE && !one_of<2, 4>(p.ni)) return false;
    if (paged) {
        if (!p.table || p.n_blocks < 1 || p.n_table < n_tiles) return false;
        for (long i = 0; i < (long)p.n_lanes * p.n_table; ++i)
            if (p.table[i] < 0 || p.table[i] >= p.n_blocks) return false;
    }
    for (int l = 0; l < p.n_lanes; ++l) {
        if (p.pos[l] < 0 || p.pos[l] >= p.max_seq || p.n_pad[l] < 0 || p.done[l] < 0 || p.done[l] > 2) return false;
        if (is_pred(kind) && (p.pos[l] > 16 || p.pos[l] != p.pos[0] || p.done[l] != 0 || p.n_pad[l] != 0)) return false;   // one position per launch
    }
    if (kind == K_SPLIT && !(p.flags & FL_DONE_PTR) && p.done[0] != 0) return false;
    return true;
}

template <typename T>
int run_t(int kind, const AttnProbeArgs& p, hipStream_t s) {
    const int B = p.n_lanes, q_dim = p.n_kv * p.rep * kHeadDim;
    // ---- the device image of everything the kernels chase pointers through ----
    struct Blob { LaneTab tab; LaneKV kv; LaneTabs tabs; int pos0, done0; };
    const size_t off_st = sizeof(Blob), off_tb = off_st + sizeof(DecodeState) * (size_t)B;
    const size_t n_tab = is_paged(kind, p) ? (size_t)B * p.n_table : 0;
    const size_t bytes = off_tb + sizeof(int) * (n_tab ? n_tab : 1);
    char* dev = nullptr;
    AttnArgs a{};
    if (!is_merge(kind)) {
        if (hipMalloc(&dev, bytes) != hipSuccess) return (int)hipGetLastError();
        std::vector<char> host(bytes, 0);
        Blob* b = reinterpret_cast<Blob*>(host.data());
        DecodeState* st = reinterpret_cast<DecodeState*>(host.data() + off_st);
        int* tb = reinterpret_cast<int*>(host.data() + off_tb);
        for (int l = 0; l < B; ++l) {
            st[l].pos = p.pos[l]; st[l].done = p.done[l]; st[l].n_pad = p.n_pad[l]; st[l].max_seq = p.max_seq;
            b->tab.st[l] = reinterpret_cast<DecodeState*>(dev + off_st) + l;
            b->kv.k[l] = reinterpret_cast<T*>(p.kcache) + (size_t)l * p.kv_lane_stride;
            b->kv.v[l] = reinterpret_cast<T*>(p.vcache) + (size_t)l * p.kv_lane_stride;
            b->tabs.t[l] = reinterpret_cast<const int*>(dev + off_tb) + (size_t)l * p.n_table;
        }
        b->tabs.blk_stride = p.n_kv * kKeysPerTile * kHeadDim;
        b->pos0 = p.pos[0]; b->done0 = p.done[0];
        if (n_tab) memcpy(tb, p.table, n_tab * sizeof(int));
        if (hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dev); return (int)hipGetLastError(); }
        a.qkv = p.qkv; a.q_norm_w = p.q_norm_w; a.k_norm_w = p.k_norm_w; a.eps = p.eps;
        a.cos_row = p.rope; a.sin_row = p.rope + 64;
        a.kcache = p.kcache; a.vcache = p.vcache; a.max_seq = p.max_seq;
        a.table = n_tab ? reinterpret_cast<const int*>(dev + off_tb) : nullptr;
        a.blk_stride = p.n_kv * kKeysPerTile * kHeadDim;
        a.pos_ptr = nullptr; a.pos_imm = p.pos[0]; a.n_pad = p.n_pad[0]; a.done_ptr = nullptr;
        a.n_kv = p.n_kv; a.part = p.part; a.scale = p.scale; a.rep = p.rep; a.out = p.out;
    }
    const Blob* db = reinterpret_cast<const Blob*>(dev);
    const dim3 mgrid((q_dim / 8 + 255) / 256, B);
    switch (kind) {
        case K_SPLIT:
            if (p.flags & FL_POS_PTR) { a.pos_ptr = &db->pos0; a.pos_imm = -1; }
            if (p.flags & FL_DONE_PTR) a.done_ptr = &db->done0;
            with_value<1, 2, 4>(p.rep, [&](auto r) {
                constexpr int REP = decltype(r)::value;
                if (p.paged) attn_decode_launch<T, REP, true>(a, p.workers, s);
                else attn_decode_launch<T, REP, false>(a, p.workers, s);
            });
            break;
        case K_MERGE:
            hipLaunchKernelGGL((combine_batch_kernel<T>), mgrid, dim3(256), 0, s, (const float*)p.part, (size_t)p.part_stride, p.workers, p.rep,
                               q_dim, reinterpret_cast<T*>(p.out), p.out_stride);
            break;
        case K_MERGE_GEMV: {
            GemvArgs g{};
            g.W = p.ident; g.N = q_dim; g.K = q_dim; g.y = p.out; g.part = p.part; g.n_part = p.workers; g.rep = p.rep;
            const int grid = (g.N + 3) / 4;
            const size_t shm = (size_t)g.K * sizeof(float);
            with_value<1, 2, 4>(gemv_chunks(q_dim, 4), [&](auto n) {
                gemv_launch<T, decltype(n)::value, PRO_COMBINE, EPI_STORE, false, 1, 1>(g, grid, shm, s);
            });
            break;
        }
        case K_PRED:
            attn_pred_launch<T>(a, p.n_kv * p.rep, s);
            break;
        case K_PRED_BATCH:
            hipLaunchKernelGGL((attn_pred_batch_kernel<T>), dim3(p.n_kv * p.rep, B), dim3(64), 0, s, a, &db->kv, p.qkv_stride, p.out_stride);
            break;
        case K_PRED_GROUP:
            with_value<1, 2, 4>(p.rep, [&](auto r) {
                hipLaunchKernelGGL((attn_pred_group_batch_kernel<T, decltype(r)::value>), dim3(p.n_kv, B), dim3(64), 0, s, a, &db->kv,
                                   p.qkv_stride, p.out_stride);
            });
            break;
        case K_BATCH_SPLIT:
            with_value<1, 2, 4>(p.rep, [&](auto r) {
                hipLaunchKernelGGL((attn_decode_batch_kernel<T, decltype(r)::value>), dim3(p.n_kv, p.workers, B), dim3(256), 0, s, a, &db->kv,
                                   &db->tabs, &db->tab, p.qkv_stride, p.rope, (size_t)p.part_stride);
            });
            hipLaunchKernelGGL((combine_batch_kernel<T>), mgrid, dim3(256), 0, s, (const float*)p.part, (size_t)p.part_stride, p.workers, p.rep,
                               q_dim, reinterpret_cast<T*>(p.out), p.out_stride);
            break;
        case K_LANE:
            with_value<1, 2, 4>(p.rep, [&](auto r) {
                constexpr int REP = decltype(r)::value;
                if (p.ni == 2) hipLaunchKernelGGL((attn_decode_lane_kernel<T, REP, 2>), dim3(p.n_kv, B), dim3(256), 0, s, a, &db->kv, &db->tabs,
                                                  &db->tab, p.qkv_stride, p.rope, p.out_stride);
                else hipLaunchKernelGGL((attn_decode_lane_kernel<T, REP, 4>), dim3(p.n_kv, B), dim3(256), 0, s, a, &db->kv, &db->tabs,
                                        &db->tab, p.qkv_stride, p.rope, p.out_stride);
            });
            break;
        default: break;
    }
    int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);            // the blob is freed below: the launch must have finished with it
    if (rc == 0) rc = rs;
    if (dev) (void)hipFree(dev);
    return rc;
}

}  // namespace

extern "C" {

// 1 = these arguments stay inside the buffers they describe for kernel `kind` in storage type te (0 bf16, 2 fp32)
int attn_probe_admits(int kind, int te, const AttnProbeArgs* p) { return p && admits(kind, te, *p) ? 1 : 0; }

// launch exactly kernel `kind` and wait for it; returns the HIP error of the launch or the wait, or kRefused (nothing launched)
int attn_probe_run(int kind, int te, const AttnProbeArgs* p, hipStream_t s) {
    if (!p || !admits(kind, te, *p)) return kRefused;
    return te == TE_F32 ? run_t<float>(kind, *p, s) : run_t<bf16_t>(kind, *p, s);
}

// y[i] = __expf(x[i]) for n device floats: the softmax's exponential, for the reference's exp constant (tests/_attn_ref.py)
int attn_probe_expf(const float* x, float* y, int n, hipStream_t s) {
    if (!x || !y || n <= 0) return kRefused;
    hipLaunchKernelGGL(expf_grid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n);
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);
    return rc ? rc : rs;
}

}  // extern "C"
