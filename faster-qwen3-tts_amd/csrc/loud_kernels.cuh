// Loudness stage (fq3_loud.hip): the BS.1770 K-weighted hop energies of a stream, the gated mean power and the gain that brings it to a
// target, and the multiply that applies a gain -- all on the device (include/fq3hip.h states the arithmetic).
//
// push    one lane per hop of H = in_rate / 10 samples, 64-lane workgroups.  A lane runs both biquads from zero state over the hop in
//         front of its own (the warm-up, outputs discarded) and then its own, 2 H serial steps of about two dependent fmaf each; hop 0
//         warms up on zeros, which leave the state at zero.  The lanes' samples lie H floats apart, so the workgroup stages tiles of 64
//         rows x 32 samples through the LDS: 32 consecutive lanes read one row's 128 bytes (two rows per load instruction), the rows
//         are padded by one word, and every lane then reads its own row without a bank conflict.  The next tile's loads are in flight
//         while the current one is filtered.  Every sample is read by two lanes (its own hop's and the next one's).  A lane also takes
//         the peak and the count of non-finite samples of its own hop.  One more workgroup copies the samples the next push still
//         needs (at most 2 H - 1) into the other history buffer and, on the final push, takes the peak of the partial hop at the end.
//         A workgroup is ONE wave, so a push takes what one lane's 2 H steps take, whatever its length (measured: 0.32 ms at 24 kHz,
//         about 160 clocks per step): the walk is kept lean -- the warm-up half runs the biquads alone, the
//         quantum is formed in 32-bit parts without a double, and no load is guarded by a branch.
// finish  ONE workgroup: blocks of four hops, the two gates as exact integer sums (32-bit halves in two uint64, reduced through the
//         LDS), and on thread 0 the mean power and the gain in IEEE double (multiply, divide, sqrt, compare, convert -- nothing else).
// apply   out[i] = pcm[i] * *gain: 16 bytes per lane where source and destination agree modulo 16 bytes, element-wise otherwise.
// No atomics, no private arrays in memory; everything is written by ordinary vector stores.  The push is ONE __device__ body
// (loud_push_body) behind two __global__ shells: loud_push_kernel for one stream and loud_push_group_kernel for the meters of a group
// of levellers (fq3_leveller_push_group), whose blockIdx.y picks the row -- the rows' serial walks then run side by side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fq3hip.h"

#pragma clang fp contract(off)

namespace fq3 {

constexpr int kLoudLanes = 64;                      // hops per workgroup of the push kernel: one wave
constexpr int kLoudTile = 32;                       // samples per row and tile: one 128-byte line
constexpr int kLoudPitch = kLoudTile + 1;           // LDS row pitch in words
constexpr int kLoudFinishThreads = 256;
constexpr int kLoudApplyThreads = 256;
constexpr float kLoudClip = 64.0f;                  // y * y is clipped here, so that a hop's energy stays below 2^59
constexpr double kLoudScale = 1099511627776.0;      // 2^40

struct LoudCoef { float b0, b1, b2, a1, a2; };

struct LoudPushArgs {
    const float* pcm;          // the new samples, n_in floats
    const float* hist;         // the last n_hist samples pushed before them
    float* hist_next;          // receives the samples the next push needs (the other of the object's two buffers)
    uint64_t* energy;          // E[h]
    float* peak;               // per hop; entry n_hops of a finished stream: the partial hop at the end
    int* bad;                  // per hop likewise: non-finite samples
    int64_t n_hist, n_in;
    int64_t v0;                // V = hist ++ pcm; V[0] is sample v0 of the stream
    int64_t h0;                // first hop this push completes
    int n_new;                 // hops it completes
    int H;
    int final;
    int keep;                  // not final: the samples to keep, V[m - keep, m)
    LoudCoef shelf, hp;
};

__device__ __forceinline__ float loud_fetch(const LoudPushArgs& a, int64_t c) {
    return c < a.n_hist ? a.hist[c] : a.pcm[c - a.n_hist];
}

__device__ __forceinline__ float loud_biquad(const LoudCoef& c, float x, float& s1, float& s2) {
    const float u = fmaf(c.b0, x, s1);
    s1 = fmaf(-c.a1, u, fmaf(c.b1, x, s2));
    s2 = fmaf(-c.a2, u, c.b2 * x);
    return u;
}

// q(y) = rint(min(y * y, 64) * 2^40) in two 32-bit parts, q = (hi << 23) + lo, without a double: with p = min(y * y, 64.0f) and
// x = p * 2^17 (exact), hi = trunc(x) <= 2^23 and lo = rint((x - hi) * 2^23) <= 2^23 -- the fraction of a float is a float and the
// scalings are by powers of two, so every step but the one rint is exact, and hi * 2^23 is even, so ties fall as in the contract.
// 32 samples of either part sum to at most 2^28: a tile is accumulated in 32 bits.
__device__ __forceinline__ void loud_quant(float y, uint32_t& hi, uint32_t& lo) {
    const float p = fminf(y * y, kLoudClip);
    const float x = p * 131072.0f;
    const float a = truncf(x);
    hi += (uint32_t)a;
    lo += (uint32_t)rintf((x - a) * 8388608.0f);
}

__device__ __forceinline__ void loud_note(float x, float& pk, int& nb) {
    const float ax = fabsf(x);
    const bool ok = ax <= 3.402823466e+38f;                        // a NaN compares false
    pk = fmaxf(pk, ok ? ax : 0.0f);
    nb += ok ? 0 : 1;
}

struct LoudLane { float s1, s2, t1, t2, pk; int nb; uint64_t e; };

// nj <= kLoudTile steps of one lane from its LDS row; kMeasure: the lane's own hop (energy, peak, non-finite count)
template <bool kMeasure, bool kFull>
__device__ __forceinline__ void loud_steps(const LoudPushArgs& a, const float* row, int nj, LoudLane& z) {
    uint32_t hi = 0, lo = 0;
    if (kFull) {
        float x[kLoudTile];
#pragma unroll
        for (int j = 0; j < kLoudTile; ++j) x[j] = row[j];
#pragma unroll
        for (int j = 0; j < kLoudTile; ++j) {
            const float y = loud_biquad(a.hp, loud_biquad(a.shelf, x[j], z.s1, z.s2), z.t1, z.t2);
            if (kMeasure) { loud_quant(y, hi, lo); loud_note(x[j], z.pk, z.nb); }
        }
    } else {
        for (int j = 0; j < nj; ++j) {
            const float x = row[j];
            const float y = loud_biquad(a.hp, loud_biquad(a.shelf, x, z.s1, z.s2), z.t1, z.t2);
            if (kMeasure) { loud_quant(y, hi, lo); loud_note(x, z.pk, z.nb); }
        }
    }
    if (kMeasure) z.e += ((uint64_t)hi << 23) + lo;
}

struct LoudPushLds {
    float tile[kLoudLanes * kLoudPitch];
    float r_pk[kLoudLanes];
    int r_nb[kLoudLanes];
};

// workgroup `wg` of a push, wg <= (n_new + 63) / 64: the ONE body of the single and the group launch (all kLoudLanes threads call it)
__device__ __forceinline__ void loud_push_body(const LoudPushArgs& a, int wg, LoudPushLds& s) {
    float* const tile = s.tile;
    float* const r_pk = s.r_pk;
    int* const r_nb = s.r_nb;
    const int lane = threadIdx.x;
    const int64_t m = a.n_hist + a.n_in;
    const int n_wg = (a.n_new + kLoudLanes - 1) / kLoudLanes;
    if (wg == n_wg) {
        // the workgroup behind the hops: the history of the next push, or the partial hop that ends the stream
        if (!a.final) {
            for (int j = lane; j < a.keep; j += kLoudLanes) a.hist_next[j] = loud_fetch(a, m - a.keep + j);
            return;
        }
        const int64_t hops = a.h0 + a.n_new;
        float pk = 0.0f;
        int nb = 0;
        for (int64_t c = hops * a.H - a.v0 + lane; c < m; c += kLoudLanes) loud_note(loud_fetch(a, c), pk, nb);
        r_pk[lane] = pk; r_nb[lane] = nb;
        __syncthreads();
        for (int s = kLoudLanes / 2; s > 0; s >>= 1) {
            if (lane < s) { r_pk[lane] = fmaxf(r_pk[lane], r_pk[lane + s]); r_nb[lane] += r_nb[lane + s]; }
            __syncthreads();
        }
        if (lane == 0) { a.peak[hops] = r_pk[0]; a.bad[hops] = r_nb[0]; }
        return;
    }
    const int H = a.H;
    const int row0 = wg * kLoudLanes;                 // first hop of this workgroup, counted from h0
    const int rows = a.n_new - row0 < kLoudLanes ? a.n_new - row0 : kLoudLanes;
    // row r starts at V index (h0 + row0 + r - 1) H - v0: below zero only for hop 0, whose warm-up lies in front of the stream
    const int64_t base = (a.h0 + row0 - 1) * H - a.v0;
    const int sub = lane & (kLoudTile - 1), half = lane >> 5;
    // Nothing a load brings in has to be a zero, so no load needs a branch: rows behind the last one repeat it (their lanes store
    // nothing), a short tile's spare steps are not walked, and hop 0 -- whose warm-up lies in front of the stream -- gets its state
    // set back to zero behind the warm-up, which is what a warm-up on zeros leaves.  A workgroup whose rows all lie inside the new
    // samples adds a per-lane offset to a uniform pointer; the first workgroup of a push, which may begin in the history or in front
    // of the stream, and short tiles clamp the index into V and pick the source.
    const bool inside = base >= a.n_hist;
    const int last = rows - 1;
    // the walk is two phases of H steps (warm-up, own hop), each cut into tiles of 32 steps; only a phase's last tile may be short
    const int per_phase = (H + kLoudTile - 1) / kLoudTile;
    const int64_t span = m - base;                                 // offsets from `base` stay far below 2^31: 66 H at most are used
    const int lo = base < 0 ? (int)-base : 0, hi = (int)(span < 0x7fffffff ? span : 0x7fffffff) - 1;
    const int64_t split64 = a.n_hist - base;
    const int split = (int)(split64 < 0 ? 0 : split64);            // offsets below it are history (n_hist < 2 H)
    // V[base] seen from either source (typed pointers, so the loads stay global loads; only offsets inside the source are read)
    const float* const hist_at = a.hist + base;
    const float* const pcm_at = a.pcm + (base - a.n_hist);
    float pre[kLoudTile];
    auto load = [&](int T) {
        const int phase = T >= per_phase ? 1 : 0, tt = T - phase * per_phase;
        const int s0 = phase * H + tt * kLoudTile;                 // first step of the tile
        const int nj = H - tt * kLoudTile < kLoudTile ? H - tt * kLoudTile : kLoudTile;
        if (inside && nj == kLoudTile) {
            const float* p0 = a.pcm + (base - a.n_hist + s0);       // uniform
#pragma unroll
            for (int k = 0; k < kLoudTile; ++k) {
                const int r = 2 * k + half < last ? 2 * k + half : last;
                pre[k] = p0[r * H + sub];
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < kLoudTile; ++k) {
            const int r = 2 * k + half < last ? 2 * k + half : last;
            int off = r * H + s0 + sub;
            off = off < lo ? lo : (off > hi ? hi : off);
            pre[k] = (off < split ? hist_at : pcm_at)[off];
        }
    };
    LoudLane z{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0};
    load(0);
    for (int T = 0; T < 2 * per_phase; ++T) {
#pragma unroll
        for (int k = 0; k < kLoudTile; ++k) tile[(2 * k + half) * kLoudPitch + sub] = pre[k];
        __syncthreads();
        if (T + 1 < 2 * per_phase) load(T + 1);
        const int tt = T >= per_phase ? T - per_phase : T;
        const int nj = H - tt * kLoudTile < kLoudTile ? H - tt * kLoudTile : kLoudTile;
        const float* row = &tile[lane * kLoudPitch];
        if (T < per_phase) {
            if (nj == kLoudTile) loud_steps<false, true>(a, row, nj, z);
            else loud_steps<false, false>(a, row, nj, z);
        } else {
            if (nj == kLoudTile) loud_steps<true, true>(a, row, nj, z);
            else loud_steps<true, false>(a, row, nj, z);
        }
        if (T == per_phase - 1 && a.h0 + row0 + lane == 0) z.s1 = z.s2 = z.t1 = z.t2 = 0.0f;      // hop 0: the warm-up was zeros
        __syncthreads();                                           // the next round rewrites the tile
    }
    if (lane < rows) {
        const int64_t h = a.h0 + row0 + lane;
        a.energy[h] = z.e; a.peak[h] = z.pk; a.bad[h] = z.nb;
    }
}

// ---- a group of pushes in one launch (fq3_loud_push_group_, for fq3_leveller_push_group) ----
// Grid (largest n_wg + 1 over the rows, B): blockIdx.y picks the row, blockIdx.x its workgroup.  The rows share the rate (H and the
// K-weighting coefficients); everything else travels per row, BY VALUE in the kernel's argument block as in audio_kernels.cuh and
// tsm_kernels.cuh: blockIdx.y is uniform, so a row's fields are scalar loads from the argument segment.  A workgroup behind its row's
// last one (the history workgroup) leaves before any barrier; a row with nothing to do (active == 0) costs workgroups that leave.
constexpr int kLoudGroupMax = 32;                   // FQ3_STAGE_GROUP_MAX

struct LoudRow {
    const float* pcm;
    const float* hist;
    float* hist_next;
    uint64_t* energy;
    float* peak;
    int* bad;
    int64_t n_hist, n_in, v0, h0;
    int n_new, final, keep, active;
};

struct LoudGroupArgs {
    int H;
    LoudCoef shelf, hp;
    LoudRow rows[kLoudGroupMax];
};
static_assert(sizeof(LoudRow) == 96 && sizeof(LoudGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

// FQ3_LOUD_NO_KERNELS (defined by a .hip file in front of its includes, never by a header): a second translation unit that wants the
// __device__ helpers and constants above and below (fq3_level.hip) leaves the __global__ definitions to fq3_loud.hip -- they
// have external linkage and may exist once in the library.
#ifndef FQ3_LOUD_NO_KERNELS
__global__ void __launch_bounds__(kLoudLanes) loud_push_kernel(const LoudPushArgs a) {
    __shared__ LoudPushLds s;
    loud_push_body(a, (int)blockIdx.x, s);
}

__global__ void __launch_bounds__(kLoudLanes) loud_push_group_kernel(const LoudGroupArgs g) {
    __shared__ LoudPushLds s;
    const LoudRow& r = g.rows[blockIdx.y];
    if (!r.active || (int)blockIdx.x > (r.n_new + kLoudLanes - 1) / kLoudLanes) return;
    LoudPushArgs a;
    a.pcm = r.pcm; a.hist = r.hist; a.hist_next = r.hist_next; a.energy = r.energy; a.peak = r.peak; a.bad = r.bad;
    a.n_hist = r.n_hist; a.n_in = r.n_in; a.v0 = r.v0; a.h0 = r.h0;
    a.n_new = r.n_new; a.H = g.H; a.final = r.final; a.keep = r.keep;
    a.shelf = g.shelf; a.hp = g.hp;
    loud_push_body(a, (int)blockIdx.x, s);
}

#endif  // FQ3_LOUD_NO_KERNELS

struct LoudFinishArgs {
    const uint64_t* energy;
    const float* peak;
    const int* bad;
    fq3_loud_stats* out;
    int n_hops;
    uint64_t abs_gate;
    double four_h, target_power, ceiling, max_gain;
};

// sum of (count, low halves, high halves) over the workgroup; the result is valid on every thread
__device__ __forceinline__ void loud_reduce3(int tid, int& n, uint64_t& lo, uint64_t& hi, int* r_n, uint64_t* r_lo, uint64_t* r_hi) {
    __syncthreads();
    r_n[tid] = n; r_lo[tid] = lo; r_hi[tid] = hi;
    __syncthreads();
    for (int s = kLoudFinishThreads / 2; s > 0; s >>= 1) {
        if (tid < s) { r_n[tid] += r_n[tid + s]; r_lo[tid] += r_lo[tid + s]; r_hi[tid] += r_hi[tid + s]; }
        __syncthreads();
    }
    n = r_n[0]; lo = r_lo[0]; hi = r_hi[0];
}

// The gating and the gain of the contract over the hops [0, n_hops), ONE copy: loud_finish_kernel runs it over a finished stream
// (n_peaks = n_hops + 1: the partial hop behind the hops counts toward peak and non-finite count), the leveller's target kernel
// (level_kernels.cuh) over every prefix of a running one (n_peaks = n_hops).  Called by all kLoudFinishThreads threads of a workgroup;
// pk, nb, n1, n2 are valid on every thread, the doubles are formed where the caller asks for them (thread 0).
struct LoudGateLds {
    int r_n[kLoudFinishThreads];
    uint64_t r_lo[kLoudFinishThreads], r_hi[kLoudFinishThreads];
    float r_pk[kLoudFinishThreads];
};

struct LoudGate { float pk; int nb, n1, n2; uint64_t lo2, hi2; };

__device__ __forceinline__ LoudGate loud_gate(const uint64_t* energy, const float* peak, const int* bad, int n_hops, int n_peaks,
                                              uint64_t abs_gate, LoudGateLds& s) {
    const int tid = threadIdx.x;
    float pk = 0.0f;
    int nb = 0;
    for (int h = tid; h < n_peaks; h += kLoudFinishThreads) { pk = fmaxf(pk, peak[h]); nb += bad[h]; }
    s.r_pk[tid] = pk;
    uint64_t z0 = 0, z1 = 0;
    loud_reduce3(tid, nb, z0, z1, s.r_n, s.r_lo, s.r_hi);
    for (int w = kLoudFinishThreads / 2; w > 0; w >>= 1) {
        if (tid < w) s.r_pk[tid] = fmaxf(s.r_pk[tid], s.r_pk[tid + w]);
        __syncthreads();
    }
    pk = s.r_pk[0];
    const int n_blocks = n_hops >= 4 ? n_hops - 3 : 0;
    int n1 = 0;
    uint64_t lo1 = 0, hi1 = 0;
    for (int b = tid; b < n_blocks; b += kLoudFinishThreads) {
        const uint64_t B = energy[b] + energy[b + 1] + energy[b + 2] + energy[b + 3];
        if (B > abs_gate) { ++n1; lo1 += B & 0xffffffffull; hi1 += B >> 32; }
    }
    loud_reduce3(tid, n1, lo1, hi1, s.r_n, s.r_lo, s.r_hi);
    const double s1d = (double)hi1 * 4294967296.0 + (double)lo1;
    const double tenfold = (double)(10 * (int64_t)n1);
    int n2 = 0;
    uint64_t lo2 = 0, hi2 = 0;
    for (int b = tid; b < n_blocks; b += kLoudFinishThreads) {
        const uint64_t B = energy[b] + energy[b + 1] + energy[b + 2] + energy[b + 3];
        if (B > abs_gate && (double)B * tenfold > s1d) { ++n2; lo2 += B & 0xffffffffull; hi2 += B >> 32; }
    }
    loud_reduce3(tid, n2, lo2, hi2, s.r_n, s.r_lo, s.r_hi);
    return LoudGate{pk, nb, n1, n2, lo2, hi2};
}

// mean power of the blocks that passed both gates (n2 > 0)
__device__ __forceinline__ double loud_mean_power(const LoudGate& g, double four_h) {
    const double s2d = (double)g.hi2 * 4294967296.0 + (double)g.lo2;
    return s2d / ((double)g.n2 * four_h * kLoudScale);
}

// min(sqrt(target_power / mean_power), max_gain, ceiling / peak) in double, rounded once
__device__ __forceinline__ float loud_gain(double mean_power, float pk, double target_power, double ceiling, double max_gain) {
    double g = __dsqrt_rn(target_power / mean_power);
    if (max_gain < g) g = max_gain;
    if (pk > 0.0f) {
        const double c = ceiling / (double)pk;
        if (c < g) g = c;
    }
    return (float)g;
}

#ifndef FQ3_LOUD_NO_KERNELS
__global__ void __launch_bounds__(kLoudFinishThreads) loud_finish_kernel(const LoudFinishArgs a) {
    __shared__ LoudGateLds s;
    // peak and non-finite count: the hops and the partial hop behind them
    const LoudGate g = loud_gate(a.energy, a.peak, a.bad, a.n_hops, a.n_hops + 1, a.abs_gate, s);
    if (threadIdx.x != 0) return;
    fq3_loud_stats st;
    st.mean_power = 0.0; st.peak = g.pk; st.gain = 1.0f;
    st.n_hops = a.n_hops; st.n_abs = g.n1; st.n_rel = g.n2; st.n_bad = g.nb; st.valid = 0; st.reserved = 0;
    if (g.n2 > 0) {
        st.mean_power = loud_mean_power(g, a.four_h);
        if (g.nb == 0) {
            st.gain = loud_gain(st.mean_power, g.pk, a.target_power, a.ceiling, a.max_gain);
            st.valid = 1;
        }
    }
    *a.out = st;
}

__global__ void __launch_bounds__(kLoudApplyThreads) loud_apply_kernel(const float* __restrict__ gain, const float* pcm, float* out, int64_t n) {
    const float g = *gain;
    const int64_t tid = (int64_t)blockIdx.x * kLoudApplyThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kLoudApplyThreads;
    if ((((uintptr_t)pcm ^ (uintptr_t)out) & 15) != 0) {
        for (int64_t i = tid; i < n; i += stride) out[i] = pcm[i] * g;
        return;
    }
    int64_t head = (int64_t)(((16 - ((uintptr_t)pcm & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (tid < head) out[tid] = pcm[tid] * g;
    const int64_t nv = (n - head) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(pcm + head);
    float4* d4 = reinterpret_cast<float4*>(out + head);
    for (int64_t i = tid; i < nv; i += stride) {
        const float4 v = s4[i];
        d4[i] = make_float4(v.x * g, v.y * g, v.z * g, v.w * g);
    }
    const int64_t done = head + 4 * nv;
    if (done + tid < n) out[done + tid] = pcm[done + tid] * g;
}

#endif  // FQ3_LOUD_NO_KERNELS

}  // namespace fq3
