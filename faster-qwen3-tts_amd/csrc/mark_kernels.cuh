// Provenance watermark (fq3_mark.hip; include/fq3hip.h states the arithmetic): a keyed spread-spectrum mark on a float32 stream at
// 24 kHz and its detector.  Frames of N = 512 samples at hop H = 256 under a sqrt-Hann window; the mark lives in the 64 bins 11 .. 74.
//
// The two DFTs are skinny GEMMs on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), with the window folded into the tables:
//   forward   X[16 frames][128]  = S[16][512] . F[512][128]      columns 0 .. 63: w cos, 64 .. 127: -w sin  (Re | Im of the band)
//   inverse   d[16 frames][512]  = D[16][128] . G[128][512]      rows    0 .. 63: (2 / N) w cos, 64 .. 127: -(2 / N) w sin
// A workgroup is four waves and owns 16 consecutive frames (one M tile).  The A operand of the forward product is the staged sample
// run itself: frame f is samples [256 f, 256 f + 512) of it, so the 17 hops are staged ONCE and every frame is a view.  The run is
// kept with 4 words of padding per hop, which spreads the 16 frame rows of an operand fetch over the banks.  Both tables are
// designed on the host in double, rounded once to fp32 and laid out fragment-major -- [N tile][K step][lane] -- so that a B operand
// is one coalesced 256-byte load per wave, streamed from L2 (2 x 256 KB; they never fit the LDS and are never staged).
//   forward   wave w forms bins 16 w .. 16 w + 15: the cos tile and the sin tile of the same bins, so Re and Im of a bin meet in one
//             lane.  K = 512 is 128 steps; each product runs as four interleaved chains (steps 4 i + c) that are added pairwise at
//             the end: eight independent MFMA chains per wave instead of two dependent ones, and a shorter sum each.
//   chips     in registers between the products: the lane holding (frame t, bin j) takes bit j of chip row t mod 128 from one
//             Philox call and scales Re and Im by +-a on their way to the LDS, where they become the inverse's A operand.
//   inverse   wave w forms samples 128 w .. 128 w + 127 of all 16 frames: 8 N tiles, K = 128 in 32 steps, the A fragments held in
//             registers (32 per lane).
//   embed     the 16 x 512 corrections go to the LDS; hop q of the workgroup's 15 is  (x + d_q[256 + m]) + d_{q + 1}[m].  The frame
//             between two workgroups is computed by both: no atomics, no traffic between workgroups.
// THE IDENTITY CONTRACT.  A row of an MFMA tile is computed from its own A row alone and in the same order in every row, the K
// order is fixed, and nothing depends on the grid: d_t is a function of frame t's 512 samples only, whatever the cut into pushes,
// the workgroup or the row the frame falls on.  A stream is therefore marked bit for bit the same however it is pushed.
//   detect    grid (frame tiles, 32 offsets).  The same staging and forward product over the received signal shifted by the offset,
//             L = ln(|Z| + 1e-9) of 16 frames to the LDS, d for the 14 inner ones, then for each of the 128 phases the partial sum
//             of d . c over the tile and the partial sum of d^2, written to the workgroup's own slot.
//   reduce    adds the tiles' partials in ascending order and divides: z[32][128].  The sums of d c and d^2 -- thousands of terms of
//             either sign -- are carried in double and rounded once per slot; everything in front of them is fp32.
// No private arrays in memory, no inline assembly; results are written by ordinary vector stores.
#pragma once
#include "fq3_common.cuh"
#include "philox.cuh"

namespace fq3 {

typedef __attribute__((ext_vector_type(4))) float mark_f32x4;      // one lane's share of a 16 x 16 MFMA tile

constexpr int kMarkN = 512, kMarkH = 256, kMarkLo = 11, kMarkBins = 64, kMarkPeriod = 128;
constexpr int kMarkThreads = 256;
constexpr int kMarkRows = 16;                       // frames of a workgroup: one M tile
constexpr int kMarkHops = kMarkRows - 1;            // hops an embed workgroup emits
constexpr int kMarkInner = kMarkRows - 2;           // frames a detect workgroup forms d for
constexpr int kMarkKeep = 3 * kMarkH;               // input samples the object keeps: a frame and the partial hop behind it
constexpr int kMarkOffsets = 32, kMarkOffsetStep = 8;
constexpr uint32_t kMarkSlot = 0xFFFFFFFEu;         // the chips' Philox slot (noise_kernels.cuh uses 0 .. G - 1 and 0xFFFFFFFF)
constexpr int kMarkFwdFloats = 8 * 128 * 64;        // [8 N tiles][128 K steps][64 lanes]
constexpr int kMarkInvFloats = 32 * 32 * 64;        // [32 N tiles][32 K steps][64 lanes]
constexpr int kMarkRun = (kMarkRows + 1) * kMarkH;  // staged samples of a workgroup: 17 hops
constexpr int kMarkRunLds = kMarkRun + (kMarkRows + 1) * 4;
constexpr int kMarkDLd = 2 * kMarkBins + 4, kMarkELd = kMarkN + 4, kMarkLLd = kMarkBins + 1;
constexpr int kMarkPartLd = kMarkPeriod + 1;        // a detect slot: 128 phase sums and the sum of squares

// The stream around a workgroup: samples [v0, before) lie in hist, [before, total) in pcm, everything else is zero.
struct MarkSrc {
    const float* pcm;
    const float* hist;
    int64_t v0, before, total;
};

__device__ __forceinline__ float mark_sample(const MarkSrc& s, int64_t i) {
    if (i < s.v0 || i >= s.total) return 0.0f;
    return i < s.before ? s.hist[i - s.v0] : s.pcm[i - s.before];
}

__device__ __forceinline__ int mark_run_at(int p) { return p + (p >> 8) * 4; }

// samples [base, base + 17 H) of the stream into the LDS run; all threads call it
__device__ __forceinline__ void mark_stage(const MarkSrc& s, int64_t base, float* run) {
    for (int p = threadIdx.x; p < kMarkRun; p += kMarkThreads) run[mark_run_at(p)] = mark_sample(s, base + p);
}

// Band DFT of the run's 16 frames.  The lane (fr = lane & 15, fq = lane >> 4) of wave w receives bin 16 w + fr of frames
// 4 fq .. 4 fq + 3 in re / im.
__device__ __forceinline__ void mark_forward(const float* run, const float* __restrict__ fwd, int wave, int lane, mark_f32x4& re_out, mark_f32x4& im_out) {
    const int fr = lane & 15, fq = lane >> 4;
    const float* tc = fwd + (size_t)wave * (128 * 64) + lane;
    const float* ts = fwd + (size_t)(4 + wave) * (128 * 64) + lane;
    mark_f32x4 re[4], im[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) re[c] = im[c] = mark_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int ks = 0; ks < 128; ks += 4)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float a = run[mark_run_at(fr * kMarkH + (ks + c) * 4 + fq)];
            re[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tc[(ks + c) * 64], re[c], 0, 0, 0);
            im[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ts[(ks + c) * 64], im[c], 0, 0, 0);
        }
    re_out = (re[0] + re[1]) + (re[2] + re[3]);
    im_out = (im[0] + im[1]) + (im[2] + im[3]);
}

// bit j of chip row p: word 2 p + (j >> 5) of the Philox row (frame 0, slot kMarkSlot), bit j & 31
__device__ __forceinline__ uint32_t mark_chip_word(int p, int j, uint32_t k0, uint32_t k1) {
    const Philox4 c = philox4x32_10((uint32_t)(p >> 1), 0u, kMarkSlot, 0u, k0, k1);
    return (p & 1) ? ((j >> 5) ? c.w : c.z) : ((j >> 5) ? c.y : c.x);
}

struct MarkPushArgs {
    MarkSrc src;               // hist ++ pcm; on a final push the stream ends at src.total
    float* hist_next;          // receives the last `keep` samples (the other of the object's two buffers)
    float* out;                // n_out floats, stream samples [o0, o0 + n_out); o0 is a multiple of H
    const float* fwd;
    const float* inv;
    int64_t o0, n_out;
    int keep;
    float a;
    uint32_t k0, k1;
};

// grid: ceil(ceil(n_out / H) / 15) workgroups of 15 hops, and one more that keeps the history
__global__ void __launch_bounds__(kMarkThreads) mark_embed_kernel(const MarkPushArgs a) {
    __shared__ float run[kMarkRunLds];
    __shared__ float D[kMarkRows * kMarkDLd];
    __shared__ float E[kMarkRows * kMarkELd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    if (blockIdx.x == gridDim.x - 1) {
        float* hn = gptr(a.hist_next);
        for (int i = tid; i < a.keep; i += kMarkThreads) hn[i] = mark_sample(a.src, a.src.total - a.keep + i);
        return;
    }
    const int64_t hop0 = a.o0 / kMarkH + (int64_t)blockIdx.x * kMarkHops;       // frame f of the tile is frame hop0 + f of the stream
    mark_stage(a.src, (hop0 - 1) * kMarkH, run);
    __syncthreads();
    mark_f32x4 re, im;
    mark_forward(run, a.fwd, wave, lane, re, im);
    const int j = wave * 16 + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = 4 * fq + r, p = (int)((hop0 + f) & (kMarkPeriod - 1));
        const float g = ((mark_chip_word(p, j, a.k0, a.k1) >> (j & 31)) & 1u) ? a.a : -a.a;
        D[f * kMarkDLd + j] = g * re[r];
        D[f * kMarkDLd + kMarkBins + j] = g * im[r];
    }
    __syncthreads();
    float af[32];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) af[ks] = D[fr * kMarkDLd + ks * 4 + fq];
    mark_f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = mark_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ti = a.inv + (size_t)(wave * 8) * (32 * 64) + lane;
#pragma unroll
    for (int ks = 0; ks < 32; ++ks)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ks], ti[(t * 32 + ks) * 64], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) E[(4 * fq + r) * kMarkELd + (wave * 8 + t) * 16 + fr] = acc[t][r];
    __syncthreads();
    float* out = gptr(a.out);
    const int64_t end = a.o0 + a.n_out;
    for (int q = 0; q < kMarkHops; ++q) {
        const int64_t n = (hop0 + q) * kMarkH + tid;
        if (n >= end) break;
        const float x = run[mark_run_at((q + 1) * kMarkH + tid)];
        out[n - a.o0] = (x + E[q * kMarkELd + kMarkH + tid]) + E[(q + 1) * kMarkELd + tid];
    }
}

struct MarkDetectArgs {
    const float* pcm;          // n received samples
    const float* fwd;
    float* part;               // [32 offsets][tiles][129]
    int64_t n;
    int T;                     // frames 0 .. T - 1 of every offset; d exists for 1 .. T - 2
    uint32_t k0, k1;
};

// grid (tiles, 32): tile i of offset o owns d of frames 1 + 14 i .. 14 + 14 i
__global__ void __launch_bounds__(kMarkThreads) mark_detect_kernel(const MarkDetectArgs a) {
    __shared__ float run[kMarkRunLds];
    __shared__ float L[kMarkRows * kMarkLLd];
    __shared__ float Dd[kMarkInner * kMarkBins];
    __shared__ uint32_t chips[2 * kMarkPeriod];
    __shared__ float P[2][kMarkPeriod];
    __shared__ float Q[kMarkBins];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int t0 = (int)blockIdx.x * kMarkInner;                                 // frame f of the tile is frame t0 + f of the offset
    const MarkSrc src{a.pcm, nullptr, 0, 0, a.n};
    mark_stage(src, (int64_t)blockIdx.y * kMarkOffsetStep + ((int64_t)t0 - 1) * kMarkH, run);
    if (tid < kMarkPeriod / 2) {
        const Philox4 c = philox4x32_10((uint32_t)tid, 0u, kMarkSlot, 0u, a.k0, a.k1);
        chips[4 * tid] = c.x; chips[4 * tid + 1] = c.y; chips[4 * tid + 2] = c.z; chips[4 * tid + 3] = c.w;
    }
    __syncthreads();
    mark_f32x4 re, im;
    mark_forward(run, a.fwd, wave, lane, re, im);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        L[(4 * fq + r) * kMarkLLd + wave * 16 + fr] = logf(sqrtf(re[r] * re[r] + im[r] * im[r]) + 1e-9f);
    __syncthreads();
    for (int e = tid; e < kMarkInner * kMarkBins; e += kMarkThreads) {
        const int q = e >> 6, j = e & 63, f = q + 1;
        float d = L[f * kMarkLLd + j] - 0.5f * (L[(f - 1) * kMarkLLd + j] + L[(f + 1) * kMarkLLd + j]);
        d = fminf(fmaxf(d, -2.0f), 2.0f);
        Dd[e] = t0 + f <= a.T - 2 ? d : 0.0f;
    }
    __syncthreads();
    {
        const int phase = tid & (kMarkPeriod - 1), hf = tid >> 7;
        double sum = 0.0;                                                        // 448 terms of either sign: summed in double, rounded once
        for (int q = hf * (kMarkInner / 2); q < (hf + 1) * (kMarkInner / 2); ++q) {
            const int p = (t0 + 1 + q + phase) & (kMarkPeriod - 1);
            const uint32_t w0 = chips[2 * p], w1 = chips[2 * p + 1];
#pragma unroll
            for (int j = 0; j < 32; ++j) sum += (double)(((w0 >> j) & 1u) ? Dd[q * kMarkBins + j] : -Dd[q * kMarkBins + j]);
#pragma unroll
            for (int j = 0; j < 32; ++j) sum += (double)(((w1 >> j) & 1u) ? Dd[q * kMarkBins + 32 + j] : -Dd[q * kMarkBins + 32 + j]);
        }
        P[hf][phase] = (float)sum;
    }
    if (tid < kMarkBins) {
        double s = 0.0;
        for (int q = 0; q < kMarkInner; ++q) s += (double)Dd[q * kMarkBins + tid] * (double)Dd[q * kMarkBins + tid];
        Q[tid] = (float)s;
    }
    __syncthreads();
    float* slot = gptr(a.part) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kMarkPartLd;
    if (tid < kMarkPeriod) slot[tid] = P[0][tid] + P[1][tid];
    if (tid == kMarkPeriod) {
        double s = 0.0;
        for (int j = 0; j < kMarkBins; ++j) s += (double)Q[j];
        slot[kMarkPeriod] = (float)s;
    }
}

// grid 32 (offsets) x 128 threads (phases): the tiles' partials in ascending order, then z = sum d c / sqrt(sum d^2) (0 for silence)
__global__ void __launch_bounds__(kMarkPeriod) mark_reduce_kernel(const float* part, int tiles, float* z) {
    const float* p = part + (size_t)blockIdx.x * tiles * kMarkPartLd;
    double s = 0.0, e = 0.0;                                                     // a long clip has thousands of tiles: summed in double
    for (int i = 0; i < tiles; ++i) {
        s += (double)p[(size_t)i * kMarkPartLd + threadIdx.x];
        e += (double)p[(size_t)i * kMarkPartLd + kMarkPeriod];
    }
    gptr(z)[blockIdx.x * kMarkPeriod + threadIdx.x] = e > 0.0 ? (float)(s / sqrt(e)) : 0.0f;
}

}  // namespace fq3
