// Segment join (fq3_join.hip): leading / trailing silence of every segment removed and a pause of zeros put behind it, on the device,
// one launch per push, ONE workgroup per stream (the hops of a stream form a chain: what a hop's fate is depends on the hops before it;
// the streams of a group do not depend on each other: join_group_kernel walks up to 32 of them side by side, a workgroup each).
//
// The stream is cut into hops of H = in_rate / 100 samples, counted from the start of each segment.  A hop is ACTIVE when some sample
// has |x| >= threshold.  Between pushes the object keeps, on the device, the samples whose fate is still open -- they are always the
// contiguous END of what was pushed so far, and they start on a hop boundary:
//     phase 0 (no active hop yet in this segment)   the last q <= lead_hops whole hops (the pre-roll) + the partial hop
//     phase 1 (an active hop was seen)              the q <= hold_hops inactive hops since the last active one (the hold queue) + the partial hop
// so a push works on V = pending ++ chunk, whose first q hops are already counted, and decides the hops behind them:
//     active                 emit hops [i - q, i], q = 0, released = 0, phase = 1
//     inactive, phase 0      q = min(q + 1, lead_hops)                         (the oldest pre-roll hop is forgotten)
//     inactive, phase 1      q += 1; above hold_hops the oldest queued hop is emitted (released += 1)
//     segment end, phase 1   the first min(q, max(0, tail_hops - released)) queued hops are emitted, then the pause
// Everything emitted is a range of V, in ascending order, so the output is a compaction of V plus zero fill.
//
// Per round of kJoinSlice hops: (1) the round's samples are read once, flat and coalesced (16 bytes per lane where the chunk is
// aligned), and every thread that meets a sample at or above the threshold stores 1 to its hop's flag in LDS -- plain stores of the
// same value, so the order does not matter; (2) thread 0 walks the flags and writes (source, length, destination) ranges to LDS,
// merging neighbours -- this walk, one lane's dependent instructions at about 0.2 us per hop, is what a push's time is made of
// (measured: 96 hops 0.025 ms, 1 600 hops 0.36 ms; a wave per hop with a ballot in (1), or eight 16-byte loads in flight per lane in
// (1) and (3), changed nothing; keeping the open range in registers took 15 % off);
// (3) all waves copy the ranges, 16 bytes per lane where source and destination agree modulo 16 bytes, element-wise otherwise.
// No atomics, no cross-workgroup traffic, no private arrays.  The state words and the pending samples are written with plain stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fq3 {

constexpr int kJoinThreads = 1024;
constexpr int kJoinSlice = 256;                     // hops per round
constexpr int kJoinReleasedCap = 1 << 20;           // `released` only matters below tail_hops <= 400

struct JoinArgs {
    const float* pcm;          // the new chunk, n_in floats
    const float* pend;         // pending samples as of before this push: q H + part floats
    float* pend_next;          // receives the pending samples as of after this push (the other of the object's two buffers)
    float* out;                // room for n_in + pending + pause floats (the host checked the bound)
    int64_t* n_out;            // device: samples written by this push
    int* state;                // device: phase, q, released
    int64_t n_in, pause;       // pause: zeros behind the segment (end == 1 only)
    float threshold;
    int H, lead, tail, hold;
    int part;                  // samples of the partial hop at the end of pend (the host knows it: segment length so far mod H)
    int end;                   // 0 the segment goes on, 1 it ends, 2 it and the stream end
    int fresh;                 // the stream starts here: the state words are not read
};

__device__ __forceinline__ float join_fetch(const JoinArgs& a, int64_t n_pend, int64_t c) {
    return c < n_pend ? a.pend[c] : a.pcm[c - n_pend];
}

// n floats from src to dst by the whole workgroup: 16-byte accesses when both pointers have the same offset inside 16 bytes
__device__ __forceinline__ void join_copy(const float* __restrict__ src, float* __restrict__ dst, int64_t n, int tid) {
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) != 0) {
#pragma unroll 4
        for (int64_t j = tid; j < n; j += kJoinThreads) dst[j] = src[j];
        return;
    }
    int64_t head = (int64_t)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const int64_t nv = (n - head) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
#pragma unroll 4
    for (int64_t j = tid; j < nv; j += kJoinThreads) d4[j] = s4[j];
    const int64_t done = head + 4 * nv;
    if (done + tid < n) dst[done + tid] = src[done + tid];
}

__device__ __forceinline__ void join_zero(float* __restrict__ dst, int64_t n, int tid) {
    int64_t head = (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (tid < head) dst[tid] = 0.0f;
    const int64_t nv = (n - head) >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int64_t j = tid; j < nv; j += kJoinThreads) d4[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int64_t done = head + 4 * nv;
    if (done + tid < n) dst[done + tid] = 0.0f;
}

// One push of one stream by one workgroup: the body of the single and of the group kernel, so that a row of a group is the single
// push instruction for instruction.
__device__ __forceinline__ void join_push_body(const JoinArgs& a) {
    __shared__ __align__(16) int act[kJoinSlice];
    __shared__ int64_t e_src[kJoinSlice + 2], e_len[kJoinSlice + 2], e_dst[kJoinSlice + 2];      // e_src < 0: zeros
    __shared__ int s_ne, s_phase, s_q, s_rel;
    __shared__ int64_t s_dst;
    const int tid = threadIdx.x;
    const int H = a.H;
    const int q0 = a.fresh ? 0 : a.state[1];
    const int64_t n_pend = (int64_t)q0 * H + a.part;
    const int64_t m = n_pend + a.n_in;                             // V = pend ++ pcm
    const int64_t n_full = m / H, rem = m - n_full * H;
    const int64_t n_hops = n_full + ((a.end && rem > 0) ? 1 : 0);  // a segment's last hop may be short
    if (tid == 0) {
        s_phase = a.fresh ? 0 : a.state[0];
        s_q = q0;
        s_rel = a.fresh ? 0 : a.state[2];
        s_dst = 0;
    }
    // the first q0 hops of V are the queue: counted already
    for (int64_t h0 = q0;; h0 += kJoinSlice) {
        const int64_t left = n_hops - h0;
        const int ns = (int)(left < kJoinSlice ? (left > 0 ? left : 0) : kJoinSlice);
        const bool last = left <= kJoinSlice;
        // (1) the round's samples as one flat, coalesced pass: the loads of a thread do not depend on each other, and whoever finds a
        // sample at or above the threshold stores 1 to its hop's flag -- plain stores of one value, whatever the order
        for (int j = tid; j < ns; j += kJoinThreads) act[j] = 0;
        __syncthreads();
        {
            const int64_t base = h0 * H;
            const int64_t avail = m - base;
            const int span = (int)(avail < (int64_t)ns * H ? (avail > 0 ? avail : 0) : (int64_t)ns * H);
            const int in_pend = (int)(n_pend > base ? (n_pend - base < span ? n_pend - base : span) : 0);
            for (int i = tid; i < in_pend; i += kJoinThreads)
                if (fabsf(a.pend[base + i]) >= a.threshold) act[i / H] = 1;                  // a NaN compares false
            const float* __restrict__ src = a.pcm + (base - n_pend);                             // src[i] is valid for i in [in_pend, span)
            if (span > in_pend && ((uintptr_t)(src + in_pend) & 15) == 0) {
                const float4* s4 = reinterpret_cast<const float4*>(src + in_pend);
                const int nv = (span - in_pend) >> 2;
#pragma unroll 4
                for (int v = tid; v < nv; v += kJoinThreads) {
                    const float4 x = s4[v];
                    const int i = in_pend + 4 * v;
                    if (fabsf(x.x) >= a.threshold) act[i / H] = 1;
                    if (fabsf(x.y) >= a.threshold) act[(i + 1) / H] = 1;
                    if (fabsf(x.z) >= a.threshold) act[(i + 2) / H] = 1;
                    if (fabsf(x.w) >= a.threshold) act[(i + 3) / H] = 1;
                }
                for (int i = in_pend + 4 * nv + tid; i < span; i += kJoinThreads)
                    if (fabsf(src[i]) >= a.threshold) act[i / H] = 1;
            } else {
#pragma unroll 4
                for (int i = in_pend + tid; i < span; i += kJoinThreads)
                    if (fabsf(src[i]) >= a.threshold) act[i / H] = 1;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int phase = s_phase, q = s_q, rel = s_rel, ne = 0;
            int64_t dst = s_dst;
            // the newest range stays open in registers while its neighbours extend it; LDS sees it once, when it closes (a
            // read-modify-write of LDS per hop measured 0.43 ms against 0.36 ms for a 200-frame segment)
            int64_t cur_b = -1, cur_e = -1, cur_d = 0;
            auto close = [&]() {
                if (cur_e > cur_b) { e_src[ne] = cur_b; e_len[ne] = cur_e - cur_b; e_dst[ne] = cur_d; ++ne; }
            };
            auto emit = [&](int64_t b, int64_t e) {
                if (e > m) e = m;
                if (cur_e == b) cur_e = e;
                else { close(); cur_b = b; cur_e = e; cur_d = dst; }
                dst += e - b;
            };
            int4 f4 = make_int4(0, 0, 0, 0);
            for (int j = 0; j < ns; ++j) {
                const int64_t i = h0 + j;
                if ((j & 3) == 0) f4 = *reinterpret_cast<const int4*>(&act[j]);      // (flags behind ns are stale and not looked at)
                const int f = (j & 3) == 0 ? f4.x : (j & 3) == 1 ? f4.y : (j & 3) == 2 ? f4.z : f4.w;
                if (f) {
                    emit((i - q) * H, (i + 1) * H);
                    phase = 1; q = 0; rel = 0;
                } else if (phase == 0) {
                    q = q < a.lead ? q + 1 : a.lead;
                } else {
                    ++q;
                    if (q > a.hold) {
                        emit((i - q + 1) * H, (i - q + 2) * H);
                        --q;
                        if (rel < kJoinReleasedCap) ++rel;
                    }
                }
            }
            if (last && a.end) {
                if (phase == 1) {
                    int k = a.tail - rel;
                    k = k < 0 ? 0 : (k > q ? q : k);
                    if (k > 0) emit((n_hops - q) * H, (n_hops - q + k) * H);
                    close();
                    cur_b = cur_e = -1;
                    if (a.end == 1 && a.pause > 0) { e_src[ne] = -1; e_len[ne] = a.pause; e_dst[ne] = dst; ++ne; dst += a.pause; }
                }
                phase = 0; q = 0; rel = 0;
            }
            close();
            s_phase = phase; s_q = q; s_rel = rel; s_dst = dst; s_ne = ne;
        }
        __syncthreads();
        const int ne = s_ne;
        for (int e = 0; e < ne; ++e) {
            const int64_t src = e_src[e], len = e_len[e];
            float* d = a.out + e_dst[e];
            if (src < 0) { join_zero(d, len, tid); continue; }
            const int64_t in_pend = src < n_pend ? (src + len < n_pend ? len : n_pend - src) : 0;
            for (int64_t j = tid; j < in_pend; j += kJoinThreads) d[j] = a.pend[src + j];
            if (len > in_pend) join_copy(a.pcm + (src + in_pend - n_pend), d + in_pend, len - in_pend, tid);
        }
        __syncthreads();                                           // the next round rewrites act / e_*
        if (last) break;
    }
    // what stays open: the queue and the partial hop (nothing after a segment's end)
    const int64_t keep = a.end ? 0 : (int64_t)s_q * H + rem;
    for (int64_t j = tid; j < keep; j += kJoinThreads) a.pend_next[j] = join_fetch(a, n_pend, m - keep + j);
    if (tid == 0) {
        a.state[0] = s_phase; a.state[1] = s_q; a.state[2] = s_rel;
        *a.n_out = s_dst;
    }
}

__global__ void __launch_bounds__(kJoinThreads) join_kernel(const JoinArgs a) { join_push_body(a); }

// The pushes of up to kJoinGroupMax streams in ONE launch (fq3_join_push_group): workgroup b runs row b through the body above.  The
// rows' descriptors travel in the argument block (32 x 96 bytes, inside the 4 KB that fq3_batch.hip notes as the limit), so there is
// no table to copy; rows share nothing, each writes its own out / n_out / state / pend_next.
constexpr int kJoinGroupMax = 32;
struct JoinGroupArgs {
    JoinArgs row[kJoinGroupMax];
    int B;
};
static_assert(sizeof(JoinGroupArgs) <= 3200, "the group's descriptors travel as launch arguments: keep them well inside 4 KB");

__global__ void __launch_bounds__(kJoinThreads) join_group_kernel(const JoinGroupArgs g) {
    const int b = blockIdx.x;
    if (b >= g.B) return;                                          // (uniform over the workgroup: no barrier is skipped by a part of it)
    join_push_body(g.row[b]);
}

}  // namespace fq3
