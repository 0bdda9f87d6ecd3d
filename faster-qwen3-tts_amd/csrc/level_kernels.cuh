// Leveller (fq3_level.hip): a causal BS.1770 gain for a stream that has not ended (include/fq3hip.h, "Leveller", states the arithmetic).
// The hop energies, peaks and non-finite counts are the loudness meter's own (loud_push_kernel through fq3_loud_push on a meter the
// object owns); the two kernels here turn them into a gain and apply it.
//
// target  ONE workgroup per hop h the push newly enters: the loud_finish computation over the PREFIX E[0 .. h) -- peak and non-finite
//         count of the hops below h, the two gates as exact integer sums and on thread 0 the mean power and the gain in IEEE double,
//         all by the ONE body loud_finish_kernel runs (loud_gate, loud_mean_power, loud_gain in loud_kernels.cuh).  T[h] = that gain when the prefix is valid
//         and at least min_blocks blocks passed the absolute gate, else g0.  The hops are independent: no chain runs over them.  The
//         workgroup of the LAST hop also writes the object's stats slot, so the slot always describes the newest T.  Workgroup h
//         walks its prefix twice: a push that enters N hops behind h0 costs about N (h0 + N / 2) block sums -- nothing for a stream
//         fed chunk by chunk, 44 000 for a 370-frame utterance in one push, and about 5 * 10^11 for ONE push of 2^20 hops (29 hours
//         of audio), which is what the capacity allows and what nobody should do: feed long audio in pieces.
// apply   one workgroup per tile of 4096 samples.  A tile touches at most 7 hops (H >= 800), so it needs S of at most 8 hops and for
//         those at most 64 + 7 values of T: they are staged in the LDS, at most 8 threads form the S values (k doubles each, ascending)
//         and every lane then computes its samples' ramp from the LDS.  16 bytes per lane where source and destination agree modulo
//         16 bytes, element-wise otherwise.  A sample's gain depends on its absolute position alone.
// stats   one thread: the slot plus S of the newest hop into the caller's device memory.
// No atomics, no private arrays in memory; everything is written by ordinary vector stores.  The __device__ bodies take their row's
// arguments and LDS, the __global__ shells only hand them over: level_target_group_kernel and level_apply_group_kernel (the launches of
// fq3_leveller_push_group, at the end of this file) call the same bodies for the row blockIdx.y picks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fq3hip.h"
#include "loud_kernels.cuh"               // loud_gate and its constants (fq3_level.hip leaves the meter's kernels to fq3_loud.hip)

#pragma clang fp contract(off)

namespace fq3 {

constexpr int kLevelTargetThreads = kLoudFinishThreads;   // loud_gate is written for this many
constexpr int kLevelApplyThreads = 256;
constexpr int kLevelTile = 4096;                           // samples per workgroup of the apply kernel
constexpr int kLevelMaxSmooth = 64;
constexpr int kLevelTileHops = 8;                          // S values a tile can need: hops hb - 1 .. hb + 6 (H >= 800)
constexpr int kLevelTileT = kLevelMaxSmooth + kLevelTileHops - 1;

struct LevelTargetArgs {
    const uint64_t* energy;    // the meter's per-hop values
    const float* peak;
    const int* bad;
    float* T;                  // T[h], h <= capacity
    fq3_level_report* slot;     // the object's stats slot
    int h_first, h_last;       // workgroup b computes T[h_first + b]; h_last = h_first + gridDim.x - 1
    int min_blocks;
    float g0;
    uint64_t abs_gate;
    double four_h, target_power, ceiling, max_gain;
};

// T[h] from the prefix E[0 .. h): the meter's own gating (loud_gate, the body loud_finish_kernel runs) with n_hops = h and no partial
// hop behind the prefix
__device__ __forceinline__ void level_target_body(const LevelTargetArgs& a, int h, LoudGateLds& s) {
    const LoudGate g = loud_gate(a.energy, a.peak, a.bad, h, h, a.abs_gate, s);
    if (threadIdx.x != 0) return;
    double mean_power = 0.0;
    float gain = a.g0;
    int valid = 0;
    if (g.n2 > 0) {
        mean_power = loud_mean_power(g, a.four_h);
        if (g.nb == 0 && g.n1 >= a.min_blocks) {
            gain = loud_gain(mean_power, g.pk, a.target_power, a.ceiling, a.max_gain);
            valid = 1;
        }
    }
    a.T[h] = gain;
    if (h == a.h_last) {
        fq3_level_report st;
        st.mean_power = mean_power; st.target_gain = gain; st.smooth_gain = 0.0f;      // (S is formed by the stats kernel)
        st.n_hops = h; st.n_abs = g.n1; st.n_rel = g.n2; st.n_bad = g.nb; st.valid = valid; st.reserved = 0;
        *a.slot = st;
    }
}

__global__ void __launch_bounds__(kLevelTargetThreads) level_target_kernel(const LevelTargetArgs a) {
    __shared__ LoudGateLds s;
    level_target_body(a, a.h_first + (int)blockIdx.x, s);
}

// S(h) = (float) ((sum of (double) T(i), i = h - k + 1 .. h ascending) / (double) k) with T(i) = g0 for i < 0; `at(i)` reads T(i), i >= 0
template <typename F>
__device__ __forceinline__ float level_smooth(int h, int k, float g0, F at) {
    double acc = 0.0;
    for (int i = h - k + 1; i <= h; ++i) acc += (double)(i < 0 ? g0 : at(i));
    return (float)(acc / (double)k);
}

struct LevelApplyArgs {
    const float* pcm;
    float* out;
    const float* T;
    int64_t n0;                // the stream position of pcm[0]
    int64_t n_in;
    int H, k;
    float g0;
};

struct LevelApplyLds {
    float T[kLevelTileT];
    float S[kLevelTileHops];
};

// the gain of the sample r samples behind the start of hop hb (r < 7 H): S index 0 is hop hb - 1
__device__ __forceinline__ float level_gain(const LevelApplyLds& s, uint32_t r, uint32_t H, float fH) {
    const uint32_t q = r / H, j = r - q * H;
    const float prev = s.S[q], cur = s.S[q + 1];
    return fmaf(cur - prev, __fdiv_rn((float)j, fH), prev);
}

// tile `tile` of a push: samples [tile * kLevelTile, min(n_in, (tile + 1) * kLevelTile)) of pcm
__device__ __forceinline__ void level_apply_body(const LevelApplyArgs& a, int64_t tile, LevelApplyLds& s) {
    const int tid = threadIdx.x;
    const int64_t i0 = tile * kLevelTile;
    const int n = (int)(a.n_in - i0 < kLevelTile ? a.n_in - i0 : kLevelTile);
    const int64_t p0 = a.n0 + i0;                                   // stream position of the tile's first sample
    const int64_t hb64 = p0 / a.H;
    const int hb = (int)hb64;                                       // its hop (below 2^20 + 1)
    const uint32_t r0 = (uint32_t)(p0 - hb64 * a.H);
    const int n_s = (int)((r0 + (uint32_t)(n - 1)) / (uint32_t)a.H) + 2;      // S of hops hb - 1 .. the last sample's hop: at most 8
    // T(hb - k .. hb - 2 + n_s): entry t is T(hb - k + t); S index q needs entries q .. q + k - 1
    for (int t = tid; t < a.k + n_s - 1; t += kLevelApplyThreads) {
        const int i = hb - a.k + t;
        s.T[t] = i < 0 ? a.g0 : a.T[i];
    }
    __syncthreads();
    if (tid < n_s) {
        const float* row = &s.T[tid];
        double acc = 0.0;
        for (int q = 0; q < a.k; ++q) acc += (double)row[q];
        s.S[tid] = (float)(acc / (double)a.k);
    }
    __syncthreads();
    const float* src = a.pcm + i0;
    float* dst = a.out + i0;
    const uint32_t H = (uint32_t)a.H;
    const float fH = (float)a.H;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) != 0) {
        for (int e = tid; e < n; e += kLevelApplyThreads) dst[e] = src[e] * level_gain(s, r0 + (uint32_t)e, H, fH);
        return;
    }
    int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid] * level_gain(s, r0 + (uint32_t)tid, H, fH);
    const int nv = (n - head) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int v = tid; v < nv; v += kLevelApplyThreads) {
        const float4 x = s4[v];
        const uint32_t r = r0 + (uint32_t)(head + 4 * v);
        d4[v] = make_float4(x.x * level_gain(s, r, H, fH), x.y * level_gain(s, r + 1, H, fH), x.z * level_gain(s, r + 2, H, fH),
                            x.w * level_gain(s, r + 3, H, fH));
    }
    const int done = head + 4 * nv;
    if (done + tid < n) dst[done + tid] = src[done + tid] * level_gain(s, r0 + (uint32_t)(done + tid), H, fH);
}

__global__ void __launch_bounds__(kLevelApplyThreads) level_apply_kernel(const LevelApplyArgs a) {
    __shared__ LevelApplyLds s;
    level_apply_body(a, (int64_t)blockIdx.x, s);
}

// ---- a group of pushes in one launch each (fq3_leveller_push_group) ----
// target: grid (most newly entered hops over the rows, B); apply: grid (most tiles, B).  blockIdx.y picks the row.  The rows share the
// design but for the initial gain (H, k, min_blocks, the gate and gain constants); the pointers, the stream positions, the counts and
// g0 travel per row, BY VALUE in the kernel's argument block as in audio_kernels.cuh and tsm_kernels.cuh.  A workgroup behind its row's
// last hop or tile leaves before any barrier; a row that enters no hop (h_last < h_first) or has no samples costs workgroups that leave.
constexpr int kLevelGroupMax = 32;                         // FQ3_STAGE_GROUP_MAX

struct LevelTargetRow {
    const uint64_t* energy;
    const float* peak;
    const int* bad;
    float* T;
    fq3_level_report* slot;
    int h_first, h_last;
    float g0;
    int reserved;
};

struct LevelTargetGroupArgs {
    int min_blocks;
    uint64_t abs_gate;
    double four_h, target_power, ceiling, max_gain;
    LevelTargetRow rows[kLevelGroupMax];
};

struct LevelApplyRow {
    const float* pcm;
    float* out;
    const float* T;
    int64_t n0, n_in;
    float g0;
    int reserved;
};

struct LevelApplyGroupArgs {
    int H, k;
    LevelApplyRow rows[kLevelGroupMax];
};
static_assert(sizeof(LevelTargetRow) == 56 && sizeof(LevelTargetGroupArgs) <= 4096 && sizeof(LevelApplyRow) == 48 &&
              sizeof(LevelApplyGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

__global__ void __launch_bounds__(kLevelTargetThreads) level_target_group_kernel(const LevelTargetGroupArgs g) {
    __shared__ LoudGateLds s;
    const LevelTargetRow& r = g.rows[blockIdx.y];
    if ((int)blockIdx.x > r.h_last - r.h_first) return;
    LevelTargetArgs a;
    a.energy = r.energy; a.peak = r.peak; a.bad = r.bad; a.T = r.T; a.slot = r.slot;
    a.h_first = r.h_first; a.h_last = r.h_last; a.min_blocks = g.min_blocks; a.g0 = r.g0;
    a.abs_gate = g.abs_gate; a.four_h = g.four_h; a.target_power = g.target_power; a.ceiling = g.ceiling; a.max_gain = g.max_gain;
    level_target_body(a, a.h_first + (int)blockIdx.x, s);
}

__global__ void __launch_bounds__(kLevelApplyThreads) level_apply_group_kernel(const LevelApplyGroupArgs g) {
    __shared__ LevelApplyLds s;
    const LevelApplyRow& r = g.rows[blockIdx.y];
    if ((int64_t)blockIdx.x * kLevelTile >= r.n_in) return;
    LevelApplyArgs a;
    a.pcm = r.pcm; a.out = r.out; a.T = r.T; a.n0 = r.n0; a.n_in = r.n_in; a.H = g.H; a.k = g.k; a.g0 = r.g0;
    level_apply_body(a, (int64_t)blockIdx.x, s);
}

// the slot and S of its hop into the caller's memory; have == 0: nothing was measured yet (T = S = g0)
__global__ void level_stats_kernel(const fq3_level_report* slot, const float* T, fq3_level_report* out, int have, int k, float g0) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    fq3_level_report st;
    if (have) {
        st = *slot;
        st.smooth_gain = level_smooth(st.n_hops, k, g0, [&](int i) { return T[i]; });
    } else {
        st.mean_power = 0.0; st.target_gain = g0; st.smooth_gain = g0;
        st.n_hops = 0; st.n_abs = 0; st.n_rel = 0; st.n_bad = 0; st.valid = 0; st.reserved = 0;
    }
    *out = st;
}

}  // namespace fq3
