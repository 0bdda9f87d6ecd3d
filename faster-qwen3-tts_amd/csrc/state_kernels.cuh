// The small kernels that move loop state, text rows and KV blocks between the arithmetic launches: the batch poll and the batch text
// append (launched by fq3_batch.hip), the block-table write, the paged KV copies, fq3_kv_adopt's block copy, and the arming, forcing,
// cancelling and reading-out of the decode loop (launched by fq3_api.hip).  tools/microbench/state_probe.hip launches each of them
// alone for tests/test_gpu_state_reference.py.
#pragma once
#include "batch_kernels.cuh"

namespace fq3 {

// ---- batch poll: out[2 l] = frame of lane l, out[2 l + 1] = fq3_decode_poll's `done` (2 held, 1 finished or EOS sampled, 0 running);
// slots from 2 B on are not written
static __global__ void poll_gather_kernel(LaneSt t, int B, int* out) {
    const int l = threadIdx.x;
    if (l < B) {
        const DecodeState* st = t.st[l];
        out[2 * l] = st->frame;
        out[2 * l + 1] = st->done == 2 ? 2 : ((st->done || st->token == st->eos_id) ? 1 : 0);      // fq3_decode_poll's `done`
    }
}

// ---- incremental text for all lanes at once (fq3hip.h: fq3_batch_text_append) ------------------------------------------------------
struct AppendDst { void* dst[kMaxLanes]; int first[kMaxLanes + 1]; };        // item i: packed rows [first[i], first[i + 1]) -> dst[i]
struct AppendPub { DecodeState* st[kMaxLanes]; int rows[kMaxLanes]; int closes[kMaxLanes]; };
// one workgroup per packed row, 16-byte pieces (a row is H elements, H a multiple of 32: fq3_bind_prompt_weights)
static __global__ __launch_bounds__(256) void text_scatter_kernel(AppendDst a, int n_items, const u32x4* y, int row_vec) {
    const int r = blockIdx.x;
    int lo = 0, hi = n_items - 1;                          // the last item whose first row is <= r (items without rows never match)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.first[mid] <= r) lo = mid; else hi = mid - 1;
    }
    u32x4* d = gptr(reinterpret_cast<u32x4*>(a.dst[lo])) + (size_t)(r - a.first[lo]) * row_vec;
    const u32x4* src = y + (size_t)r * row_vec;
    for (int e = threadIdx.x; e < row_vec; e += 256) d[e] = src[e];
}
// the named items' states: trailing_len = rows[i]; text_open = 0 where closes[i]
static __global__ __launch_bounds__(kMaxLanes) void text_publish_lanes_kernel(AppendPub p, int n_items) {
    const int i = threadIdx.x;
    if (i < n_items) {
        DecodeState* st = gptr(p.st[i]);
        st->trailing_len = p.rows[i];
        if (p.closes[i]) st->text_open = 0;
    }
}

// ---- talker KV: block table and paged copies ---------------------------------------------------------------------------------------
// entries [first, first + count) of the device block table <- vals (by value in the launch), count <= 128
struct KvTableVals { int v[128]; };
static __global__ void kv_table_write_kernel(int* table, KvTableVals vals, int first, int count) {
    const int i = threadIdx.x;
    if (i < count) table[first + i] = vals.v[i];
}

// rows [0, L) of one layer between the paged cache and a dense [n_kv][L][128] tensor (the HF layout), 16 bytes per thread
template <typename T, bool TO_CACHE>
__global__ __launch_bounds__(256) void kv_paged_copy_kernel(T* cache, const int* table, int blk_stride, T* dense, int n_kv, int L) {
    constexpr int EPC = 16 / (int)sizeof(T), CPR = kHeadDim / EPC;          // 16-byte chunks per row
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_kv * L * CPR) return;
    const int ch = i % CPR, row = i / CPR, key = row % L, h = row / L;
    T* cp = cache + (size_t)table[key / kKeysPerTile] * blk_stride + ((size_t)h * kKeysPerTile + key % kKeysPerTile) * kHeadDim + ch * EPC;
    T* dp = dense + ((size_t)h * L + key) * kHeadDim + ch * EPC;
    if (TO_CACHE) *reinterpret_cast<u32x4*>(cp) = *reinterpret_cast<const u32x4*>(dp);
    else *reinterpret_cast<u32x4*>(dp) = *reinterpret_cast<const u32x4*>(cp);
}

// fq3_kv_adopt between contexts of DIFFERENT pools: whole blocks [0, ceil(L / 64)) of every talker layer, block to block, in one
// launch: grid (2 * layers, blocks)
struct KvAdoptTab { void* dst[128]; const void* src[128]; };
template <typename T>
__global__ __launch_bounds__(256) void kv_adopt_kernel(KvAdoptTab t, const int* dst_table, const int* src_table, int blk_elems) {
    const int which = blockIdx.x, b = blockIdx.y;
    const u32x4* s = reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(t.src[which]) + (size_t)src_table[b] * blk_elems);
    u32x4* d = reinterpret_cast<u32x4*>(reinterpret_cast<T*>(t.dst[which]) + (size_t)dst_table[b] * blk_elems);
    const int n16 = blk_elems * (int)sizeof(T) / 16;
    for (int i = threadIdx.x; i < n16; i += 256) d[i] = s[i];
}

// ---- the decode loop's state from the host's side ----------------------------------------------------------------------------------
// fq3_decode_begin: the history bitmap cleared over seen_bytes bytes (a multiple of 4), past_hidden <- ph_src (ph_words 32-bit words),
// *st = init (the state travels by value in the launch)
static __global__ __launch_bounds__(256) void decode_arm_kernel(DecodeState* st, DecodeState init, unsigned char* seen, int seen_bytes,
                                                                uint32_t* past_hidden, const uint32_t* ph_src, int ph_words) {
    for (int i = threadIdx.x; i < seen_bytes / 4; i += 256) reinterpret_cast<uint32_t*>(seen)[i] = 0u;
    for (int i = threadIdx.x; i < ph_words; i += 256) past_hidden[i] = ph_src[i];
    if (threadIdx.x == 0) *st = init;
}
static __global__ void decode_set_forced_kernel(TeacherForcing* tf, const int* forced, int* decisions) {
    tf->forced = forced; tf->decisions = decisions;
}
static __global__ void decode_cancel_kernel(DecodeState* st) { st->done = 1; }
static __global__ void codes_to_i64_kernel(const int* src, int64_t* dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

}  // namespace fq3
