// Limiter stage (fq3_limit.hip): a true-peak look-ahead limiter over a float32 stream, FIR and integer operations only
// (include/fq3hip.h states the arithmetic).
//
// push    one launch, one 256-thread workgroup per tile of T output samples.  A tile's outputs [o, o + T) need the gains g[o + A ..],
//         those the window minima m[o .. o + T + A), those the requests q[o - A - H .. o + T + A), and those the samples
//         x[o - A - H - 5 .. o + T + A + 6]: T + 2 A + H + 11 samples, the tile plus the halo.  The workgroup
//           1. stages them through the LDS, coalesced -- 16 bytes per lane over the part that lies in the new samples, from the first
//              16-byte boundary on; element-wise in front of it, behind it and in the history -- with non-finite samples set to 0;
//           2. forms p (three 12-tap rows, separately rounded multiplies and adds) and q in the LDS;
//           3. takes the minimum over W = A + H + 1 entries by floor(log2 W) doubling passes between two LDS arrays (pass d turns
//              windows of width d into windows of width 2 d) and one pass that joins two power-of-two windows;
//           4. turns m into its prefix sums, rows of 256 at a time: a shuffle scan per wave, the four wave totals through the LDS, the
//              carry in a register.  The sums wrap in 32 bits; a difference of two is exact because a box sum stays below 2^32;
//           5. g = (P[l + A] - P[l - 1]) / (A + 1), y = x * ((float) g * 2^-23), stored one float per lane (out is at any float alignment).
//         Everything between the load and the store is exact integer work or a fixed float expression per sample, so the result
//         depends neither on the tile size nor on the cut.  One more workgroup copies the samples the next push still needs into the
//         other history buffer.  Peak, largest gain drop, limited and non-finite counts are reduced per wave and added to the
//         object's accumulators by integer atomics (max, max, add, add): order-free.
// stats   one thread turns the accumulators into an fq3_limit_report.
// No private arrays in memory, no inline assembly; results are written by ordinary vector stores.  The push is ONE __device__ body
// (limit_push_body) behind two __global__ shells: limit_push_kernel for one stream and limit_push_group_kernel for a group of streams
// of one design (fq3_limit_push_group), whose blockIdx.y picks the row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fq3hip.h"

#pragma clang fp contract(off)

namespace fq3 {

constexpr int kLimitThreads = 256;
constexpr int kLimitTaps = 12;                      // per fractional-phase row; tap t weighs x[n - 5 + t]
constexpr int kLimitBefore = 5, kLimitAfter = 6;    // samples a detector value reaches back and ahead
constexpr uint32_t kLimitOne = 1u << 23;            // gain 1 in Q23

struct LimitAcc {                                   // the object's accumulators; all zero at the start of a stream
    uint32_t peak_bits;                             // the largest p, as the bit pattern of a non-negative float
    uint32_t drop;                                  // the largest 2^23 - g applied
    unsigned long long n_limited, n_bad;
};

struct LimitPushArgs {
    const float* pcm;          // the new samples, n_in floats
    const float* hist;         // the last n_hist samples pushed before them
    float* hist_next;          // receives the samples the next push needs (the other of the object's two buffers)
    float* out;                // n_out floats
    LimitAcc* acc;
    int64_t n_hist, n_in;
    int64_t v0;                // V = hist ++ pcm; V[0] is sample v0 of the stream
    int64_t total;             // samples of the stream once this push is in; on a final push the stream ends there
    int64_t o0;                // stream index of out[0]
    int64_t n_out;
    int A, H, tile, keep;      // keep: the samples to copy to hist_next, V[m - keep, m)
    float c;
    float h[3 * kLimitTaps];
};

__device__ __forceinline__ float limit_clean(float x, bool& bad) {
    bad = !(fabsf(x) <= 3.402823466e+38f);                         // a NaN compares false
    return bad ? 0.0f : x;
}

struct LimitWaveSums { uint32_t v[2][kLimitThreads / 64]; };

// workgroup `tile_index` of a push, tile_index <= ceil(n_out / tile) (the last one keeps the history): the ONE body of the single and
// the group launch.  `limit_lds`: the launch's dynamic LDS, 3 * round_up(tile + 2 A + H + 11, 4) words; all kLimitThreads threads call it.
__device__ __forceinline__ void limit_push_body(const LimitPushArgs& a, int tile_index, unsigned char* limit_lds, LimitWaveSums& sums) {
    uint32_t (&wave_sum)[2][kLimitThreads / 64] = sums.v;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_tiles = (int)((a.n_out + a.tile - 1) / a.tile);
    const int64_t m = a.n_hist + a.n_in;
    if (tile_index == n_tiles) {
        // the workgroup behind the tiles: the history of the next push
        for (int j = tid; j < a.keep; j += kLimitThreads) {
            const int64_t cidx = m - a.keep + j;
            a.hist_next[j] = cidx < a.n_hist ? a.hist[cidx] : a.pcm[cidx - a.n_hist];
        }
        return;
    }
    const int A = a.A, H = a.H, W = A + H + 1;
    const int64_t t0 = a.o0 + (int64_t)tile_index * a.tile;                      // the tile's first output, a stream index
    const int Tn = (int)(a.o0 + a.n_out - t0 < a.tile ? a.o0 + a.n_out - t0 : a.tile);
    const int Lx = Tn + 2 * A + H + kLimitBefore + kLimitAfter;                    // samples staged
    const int Lq = Tn + 2 * A + H;                                                 // requests
    const int Lm = Tn + A;                                                         // window minima
    const int cap = a.tile + 2 * A + H + kLimitBefore + kLimitAfter;
    float* const xs = reinterpret_cast<float*>(limit_lds);                         // cap floats (cap rounded up to 4)
    uint32_t* qa = reinterpret_cast<uint32_t*>(limit_lds) + ((cap + 3) & ~3);
    uint32_t* qb = qa + ((cap + 3) & ~3);
    const int64_t xs0 = t0 - A - H - kLimitBefore;                                 // stream index of xs[0]
    const int64_t before = a.total - a.n_in;                                       // stream index of pcm[0]

    // 1. stage.  [vb, ve): the local indices read 16 bytes at a time.
    int nbad = 0;
    int64_t lo64 = before - xs0, hi64 = a.total - xs0;
    const int l_lo = (int)(lo64 < 0 ? 0 : (lo64 > Lx ? Lx : lo64)), l_hi = (int)(hi64 < 0 ? 0 : (hi64 > Lx ? Lx : hi64));
    int vb = l_lo, ve = l_lo;
    if (l_hi - l_lo >= 8) {
        const float* first = a.pcm + (xs0 + l_lo - before);
        vb = l_lo + (int)((4 - (((uintptr_t)first >> 2) & 3)) & 3);
        ve = vb + ((l_hi - vb) & ~3);
        const float4* src = reinterpret_cast<const float4*>(a.pcm + (xs0 + vb - before));
        for (int v = tid; v < (ve - vb) >> 2; v += kLimitThreads) {
            const float4 f = src[v];
            const int l = vb + 4 * v;
            const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool bad;
                xs[l + k] = limit_clean(e[k], bad);
                const int64_t sx = xs0 + l + k;
                nbad += (bad && sx >= t0 && sx < t0 + Tn) ? 1 : 0;
            }
        }
    }
    for (int l = tid; l < Lx; l += kLimitThreads) {
        if (l >= vb && l < ve) continue;
        const int64_t sx = xs0 + l;
        float x = 0.0f;
        if (sx >= 0 && sx < a.total) {
            const int64_t cidx = sx - a.v0;
            if (cidx >= 0) x = cidx < a.n_hist ? a.hist[cidx] : a.pcm[cidx - a.n_hist];
        }
        bool bad;
        xs[l] = limit_clean(x, bad);
        nbad += (bad && sx >= t0 && sx < t0 + Tn) ? 1 : 0;
    }
    __syncthreads();

    // 2. p and q; request lq is stream index t0 - A - H + lq and sits over xs[lq .. lq + 11]
    uint32_t pk = 0;
    for (int lq = tid; lq < Lq; lq += kLimitThreads) {
        const int64_t j = t0 - A - H + lq;
        uint32_t q = kLimitOne;
        if (j >= 0 && j < a.total) {
            float p = fabsf(xs[lq + kLimitBefore]);
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                float u = 0.0f;
#pragma unroll
                for (int t = 0; t < kLimitTaps; ++t) u = __fadd_rn(u, __fmul_rn(a.h[f * kLimitTaps + t], xs[lq + t]));
                p = fmaxf(p, fabsf(u));
            }
            const uint32_t pb = __float_as_uint(p);
            pk = pb > pk ? pb : pk;
            if (!(p <= a.c)) q = (uint32_t)floorf(__fdiv_rn(a.c, p) * 8388608.0f);
        }
        qa[lq] = q;
    }
    __syncthreads();

    // 3. window minimum over the W entries that end at each index
    int width = 1;
    for (; 2 * width <= W; width <<= 1) {
        for (int l = tid; l < Lq; l += kLimitThreads) {
            const uint32_t v = qa[l];
            const uint32_t w = l >= width ? qa[l - width] : v;
            qb[l] = v < w ? v : w;
        }
        __syncthreads();
        uint32_t* t = qa; qa = qb; qb = t;
    }
    const int rem = W - width;                                     // 0 <= rem < width: the two windows overlap or abut
    for (int l = tid; l < Lm; l += kLimitThreads) {
        const uint32_t v = qa[l + A + H], w = qa[l + A + H - rem];
        qb[l] = v < w ? v : w;                                     // m of stream index t0 + l
    }
    __syncthreads();

    // 4. prefix sums of m, in place, modulo 2^32
    uint32_t carry = 0;
    int par = 0;
    for (int base = 0; base < Lm; base += kLimitThreads, par ^= 1) {
        const int l = base + tid;
        uint32_t v = l < Lm ? qb[l] : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(v, o);
            if (lane >= o) v += t;
        }
        if (lane == 63) wave_sum[par][wave] = v;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kLimitThreads / 64; ++w) {
            const uint32_t s = wave_sum[par][w];
            pre += w < wave ? s : 0u;
            tot += s;
        }
        if (l < Lm) qb[l] = carry + pre + v;
        carry += tot;
    }
    __syncthreads();

    // 5. gain and output: output l is stream index t0 + l; its gain is the box over m[l .. l + A]
    const uint32_t div = (uint32_t)(A + 1);
    uint32_t drop = 0;
    int nlim = 0;
    float* const out = a.out + (t0 - a.o0);
    for (int l = tid; l < Tn; l += kLimitThreads) {
        const uint32_t s = qb[l + A] - (l > 0 ? qb[l - 1] : 0u);
        const uint32_t g = s / div;
        out[l] = xs[l + A + H + kLimitBefore] * ((float)g * 1.1920928955078125e-07f);
        const uint32_t d = kLimitOne - g;
        drop = d > drop ? d : drop;
        nlim += g < kLimitOne ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t p2 = __shfl_xor(pk, o), d2 = __shfl_xor(drop, o);
        pk = p2 > pk ? p2 : pk;
        drop = d2 > drop ? d2 : drop;
        nlim += __shfl_xor(nlim, o);
        nbad += __shfl_xor(nbad, o);
    }
    if (lane == 0) {
        if (pk) atomicMax(&a.acc->peak_bits, pk);
        if (drop) atomicMax(&a.acc->drop, drop);
        if (nlim) atomicAdd(&a.acc->n_limited, (unsigned long long)nlim);
        if (nbad) atomicAdd(&a.acc->n_bad, (unsigned long long)nbad);
    }
}

__global__ void __launch_bounds__(kLimitThreads) limit_push_kernel(const LimitPushArgs a) {
    extern __shared__ __align__(16) unsigned char limit_lds[];
    __shared__ LimitWaveSums sums;
    limit_push_body(a, (int)blockIdx.x, limit_lds, sums);
}

// ---- a group of pushes in one launch (fq3_limit_push_group) ----
// Grid (most tiles + 1 over the rows, B): blockIdx.y picks the row, blockIdx.x its tile.  The rows share the design (A, H, tile, the
// ceiling, the detector's 36 taps -- so one LDS layout); the pointers, the stream positions and the counts travel per row, BY VALUE in
// the kernel's argument block as in audio_kernels.cuh and tsm_kernels.cuh.  A workgroup behind its row's history workgroup leaves
// before any barrier; a row with nothing to do (active == 0: no input, not final) costs workgroups that leave.
constexpr int kLimitGroupMax = 32;                  // FQ3_STAGE_GROUP_MAX

struct LimitRow {
    const float* pcm;
    const float* hist;
    float* hist_next;
    float* out;
    LimitAcc* acc;
    int64_t n_hist, n_in, v0, total, o0, n_out;
    int keep, active;
};

struct LimitGroupArgs {
    int A, H, tile;
    float c;
    float h[3 * kLimitTaps];
    LimitRow rows[kLimitGroupMax];
};
static_assert(sizeof(LimitRow) == 96 && sizeof(LimitGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

__global__ void __launch_bounds__(kLimitThreads) limit_push_group_kernel(const LimitGroupArgs g) {
    extern __shared__ __align__(16) unsigned char limit_lds[];
    __shared__ LimitWaveSums sums;
    const LimitRow& r = g.rows[blockIdx.y];
    if (!r.active || (int64_t)blockIdx.x > (r.n_out + g.tile - 1) / g.tile) return;
    LimitPushArgs a;
    a.pcm = r.pcm; a.hist = r.hist; a.hist_next = r.hist_next; a.out = r.out; a.acc = r.acc;
    a.n_hist = r.n_hist; a.n_in = r.n_in; a.v0 = r.v0; a.total = r.total; a.o0 = r.o0; a.n_out = r.n_out;
    a.A = g.A; a.H = g.H; a.tile = g.tile; a.keep = r.keep; a.c = g.c;
#pragma unroll
    for (int i = 0; i < 3 * kLimitTaps; ++i) a.h[i] = g.h[i];
    limit_push_body(a, (int)blockIdx.x, limit_lds, sums);
}

__global__ void limit_stats_kernel(const LimitAcc* acc, fq3_limit_report* out) {
    fq3_limit_report st;
    st.true_peak = __uint_as_float(acc->peak_bits);
    st.min_gain_q23 = kLimitOne - acc->drop;
    st.n_limited = (int64_t)acc->n_limited;
    st.n_bad = (int64_t)acc->n_bad;
    *out = st;
}

}  // namespace fq3
