// Voice library search (fq3_voices_*): the nearest enrolled voices of up to 32 query x-vectors in a device-resident library [N][D],
// cosine, deterministic top-k.  DESIGN.md section 4.27.
//
// Layout.  Library rows are unit vectors (fp32), stored fragment-major for v_mfma_f32_16x16x4_f32's A operand in blocks of 16 rows:
//   lib[((rb * D/16 + kq) * 64 + lane) * 4 + j] = row[rb * 16 + (lane & 15)][kq * 16 + j * 4 + (lane >> 4)]
// so one float4 per lane -- 1 KB contiguous per wave load -- holds a block's operands of four consecutive K steps.  The queries are
// packed the same way as the B operand of two 16-column tiles.  A library row's score against a query is ONE chain of D / 4 MFMA
// steps in ascending K inside one wave: no K split, no atomics, so its bits depend on the two vectors alone.
//
// Keys.  (cosine descending, index ascending) is one unsigned 64-bit order: high word the cosine's bits mapped monotonically, low
// word ~index.  The largest key is the best candidate; keys are unique because indices are; 0 is "no candidate".
#pragma once
#include "fq3_common.cuh"

namespace fq3 {

typedef float f32x4_v __attribute__((ext_vector_type(4)));

constexpr int kVoiceQueries = 32;                // two 16-column MFMA tiles
constexpr int kVoiceMaxK = 16;
constexpr int kVoiceWaves = 8;                   // waves per workgroup of the scan
constexpr int kVoiceChunk = 8;                   // K quads (16 values each) per LDS-staged query chunk
constexpr int kVoiceMergeThreads = 256;

__device__ __forceinline__ unsigned long long voice_key(float cos, int idx) {
    const uint32_t b = __float_as_uint(cos + 0.0f);                                     // -0 -> +0
    const uint32_t hi = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ((unsigned long long)hi << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)idx);
}
__device__ __forceinline__ float voice_key_cos(unsigned long long key) {
    const uint32_t hi = (uint32_t)(key >> 32);
    return __uint_as_float(hi ^ ((hi >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ int voice_key_idx(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One wave: src[0 .. D) (nullptr: a zero row) scaled to unit length into slot `r` of a fragment-major operand of D/16 K quads.
// Sum of squares: lane l takes elements l, l + 64, ... in four interleaved fp32 chains (element l + 64 j goes to chain j % 4), the
// chains are added ((0 + 1) + (2 + 3)) and the lanes by wave_sum: a fixed order.  A zero vector stays zero.
__device__ __forceinline__ void voice_unit_store(const float* __restrict__ src, float* __restrict__ dst, long r, int D, int lane) {
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
    if (src)
        for (int d0 = lane; d0 < D; d0 += 256)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = d0 + 64 * j;
                const float u = d < D ? src[d] : 0.f;
                ss[j] = fmaf(u, u, ss[j]);
            }
    const float s = wave_sum((ss[0] + ss[1]) + (ss[2] + ss[3]));
    const float scale = s > 0.f ? 1.0f / sqrtf(s) : 0.f;
    float* blk = dst + (size_t)(r >> 4) * D * 16;
    const int m = (int)(r & 15);
    for (int d = lane; d < D; d += 64) {
        const int w = d & 15;
        blk[((size_t)(d >> 4) * 64 + (w & 3) * 16 + m) * 4 + (w >> 2)] = src ? src[d] * scale : 0.f;
    }
}

// ---- append `rows` embeddings at library rows first .. first + rows - 1 ---------------------------------------------------------------
// A wave per row, four per workgroup; the grid covers first .. the end of the last touched block of 16: rows behind the last
// appended one are written as zeros with live = 0 (the tail block is zero-filled; the next add overwrites them).
__global__ __launch_bounds__(256) void voices_add_kernel(const float* __restrict__ src, float* __restrict__ lib, uint8_t* __restrict__ live,
                                                        long first, long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6), r = first + i;
    if (r >= ((first + rows + 15) & ~15L)) return;
    const bool real = i < rows;
    voice_unit_store(real ? src + (size_t)i * D : nullptr, lib, r, D, lane);
    if (lane == 0) live[r] = real ? 1 : 0;
}

// ---- the queries as the B operand: 32 columns, those at and behind `rows` zero --------------------------------------------------------
__global__ __launch_bounds__(256) void voices_query_pack_kernel(const float* __restrict__ q, float* __restrict__ qp, int rows, int D) {
    const int lane = threadIdx.x & 63, c = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= kVoiceQueries) return;
    voice_unit_store(c < rows ? q + (size_t)c * D : nullptr, qp, c, D, lane);
}

// ---- scan: one workgroup of eight waves per slab of 8 * RB * 16 library rows ---------------------------------------------------------
// K loop     wave w owns the RB row blocks (slab * 8 + w) * RB .. and walks all D / 16 K quads in ascending order: per quad one float4
//            per block and per query tile, then 4 K steps x RB blocks x `tiles` MFMAs into 2 RB fp32 accumulators.  Blocks at and
//            behind the last block that holds a row are not loaded (a wave without any skips the products; a wave with some points the
//            others at its first block, whose duplicate scores are masked below).
// queries    QLDS false: every wave reads the packed queries from global memory (L2) -- RB blocks share each fragment;
//            QLDS true: the workgroup stages kVoiceChunk quads of both tiles in LDS per barrier pair and the waves read them there.
//            The library instantiates QLDS false only; the other form was measured slower and is built by the
//            measurement tool alone (tools/microbench/voices_variant.hip).
// tiles      1 when rows <= 16: the second tile's products are skipped, the first tile's chains are the same.
// top-k      scores -> LDS sc[32][S + 1] (dead rows and rows at or behind `count`: -inf); wave w then takes queries w, w + 8, w + 16,
//            w + 24 together: k rounds, each the largest key below the previous round's winner (lanes hold rows lane, lane + 64, ...;
//            a 64-lane butterfly of maxima), written to part[slab][query][round]; 0 where the slab has no candidate left.
// Dynamic LDS: 32 * (S + 1) floats, + 2 * kVoiceChunk * 64 float4 with QLDS.
template <int RB, bool QLDS>
__global__ __launch_bounds__(kVoiceWaves * 64) void voices_scan_kernel(const float* __restrict__ lib, const float* __restrict__ qp,
                                                                      const uint8_t* __restrict__ live, unsigned long long* __restrict__ part,
                                                                      long count, int kq_n, int tiles, int rows, int k) {
    extern __shared__ __attribute__((aligned(16))) float voice_sm[];
    constexpr int S = kVoiceWaves * RB * 16, LD = S + 1;
    float* sc = voice_sm;
    float4* qs = reinterpret_cast<float4*>(voice_sm + ((kVoiceQueries * LD + 3) & ~3));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long slab = blockIdx.x, nblk = (count + 15) >> 4;
    const long rb0 = (slab * kVoiceWaves + wave) * RB;
    const bool active = rb0 < nblk;
    f32x4_v acc[RB][2];
#pragma unroll
    for (int i = 0; i < RB; ++i) acc[i][0] = acc[i][1] = f32x4_v{0.f, 0.f, 0.f, 0.f};
    const float4* pl[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) pl[i] = reinterpret_cast<const float4*>(lib) + (size_t)(rb0 + i < nblk ? rb0 + i : (active ? rb0 : 0)) * kq_n * 64 + lane;
    const float4* pq = reinterpret_cast<const float4*>(qp);

    auto quad = [&](const int kq, const float4 b0, const float4 b1) {
        float4 a[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) a[i] = pl[i][(size_t)kq * 64];
        const float u0[4] = {b0.x, b0.y, b0.z, b0.w}, u1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const float av = j == 0 ? a[i].x : j == 1 ? a[i].y : j == 2 ? a[i].z : a[i].w;
                acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, u0[j], acc[i][0], 0, 0, 0);
                if (tiles > 1) acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, u1[j], acc[i][1], 0, 0, 0);
            }
    };
    if constexpr (QLDS) {
        for (int kc = 0; kc < kq_n; kc += kVoiceChunk) {
            const int nq = min(kVoiceChunk, kq_n - kc);
            __syncthreads();                                                            // the previous chunk has been read
            for (int e = tid; e < tiles * nq * 64; e += kVoiceWaves * 64) {
                const int t = e / (nq * 64), w = e - t * nq * 64;
                qs[t * kVoiceChunk * 64 + w] = pq[((size_t)t * kq_n + kc) * 64 + w];
            }
            __syncthreads();
            if (active)
                for (int kk = 0; kk < nq; ++kk) quad(kc + kk, qs[kk * 64 + lane], tiles > 1 ? qs[(kVoiceChunk + kk) * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f});
        }
    } else if (active) {
        for (int kq = 0; kq < kq_n; ++kq)
            quad(kq, pq[(size_t)kq * 64 + lane], tiles > 1 ? pq[((size_t)kq_n + kq) * 64 + lane] : float4{0.f, 0.f, 0.f, 0.f});
    }

    // C/D layout: column (query) = lane & 15, row (library row of the block) = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rl = (wave * RB + i) * 16 + (lane >> 4) * 4 + q;
            const long r = slab * S + rl;
            const bool ok = rb0 + i < nblk && r < count && live[r];
            const float v0 = acc[i][0][q], v1 = acc[i][1][q];                           // a NaN (a row or query that is not finite) is no candidate
            sc[(lane & 15) * LD + rl] = ok && v0 == v0 ? v0 : -INFINITY;
            sc[(16 + (lane & 15)) * LD + rl] = ok && tiles > 1 && v1 == v1 ? v1 : -INFINITY;
        }
    __syncthreads();

    const unsigned long long floor_key = voice_key(-INFINITY, 0) | 0xFFFFFFFFull;       // every key of a finite cosine is above it
    unsigned long long prev[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    for (int round = 0; round < k && wave < rows; ++round) {                           // query groups at or behind `rows` are skipped (wave-uniform)
        unsigned long long best[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (wave + 8 * g < rows)
                for (int rl = lane; rl < S; rl += 64) {
                    const unsigned long long key = voice_key(sc[(wave + 8 * g) * LD + rl], (int)(slab * S + rl));
                    if (key > floor_key && key < prev[g] && key > best[g]) best[g] = key;
                }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int query = wave + 8 * g;
            if (query >= rows) continue;
            best[g] = wave_max_u64(best[g]);
            if (lane == 0) part[((size_t)slab * kVoiceQueries + query) * k + round] = best[g];
            prev[g] = best[g];                                                         // 0: nothing left, and nothing is below 0
        }
    }
}

// ---- merge: one workgroup per query ---------------------------------------------------------------------------------------------------
// Every slab's k partials are in descending key order, so the best remaining candidate of a slab is the one at its cursor (LDS, a byte
// per slab).  k rounds: each thread takes the largest head of its slabs (tid, tid + 256, ...), the workgroup the largest of those; the
// one thread that owns the winning slab moves its cursor on.  Slots without a candidate: idx -1, cos -2.
__global__ __launch_bounds__(kVoiceMergeThreads) void voices_merge_kernel(const unsigned long long* __restrict__ part, int slabs, int k,
                                                                         int* __restrict__ idx, float* __restrict__ cos) {
    extern __shared__ __attribute__((aligned(16))) uint8_t voice_cur[];
    __shared__ unsigned long long red[kVoiceMergeThreads / 64];
    const int tid = threadIdx.x, query = blockIdx.x;
    for (int s = tid; s < slabs; s += kVoiceMergeThreads) voice_cur[s] = 0;
    __syncthreads();
    for (int round = 0; round < k; ++round) {
        unsigned long long best = 0ull;
        int bs = -1;
        for (int s = tid; s < slabs; s += kVoiceMergeThreads) {
            const int c = voice_cur[s];
            const unsigned long long key = c < k ? part[((size_t)s * kVoiceQueries + query) * k + c] : 0ull;
            if (key > best) { best = key; bs = s; }
        }
        const unsigned long long wbest = wave_max_u64(best);
        if ((tid & 63) == 0) red[tid >> 6] = wbest;
        __syncthreads();
        unsigned long long win = red[0];
#pragma unroll
        for (int w = 1; w < kVoiceMergeThreads / 64; ++w) win = red[w] > win ? red[w] : win;
        if (win != 0ull && best == win) voice_cur[bs] += 1;
        if (tid == 0) {
            idx[(size_t)query * k + round] = win ? voice_key_idx(win) : -1;
            cos[(size_t)query * k + round] = win ? voice_key_cos(win) : -2.0f;
        }
        __syncthreads();
    }
}

}  // namespace fq3
