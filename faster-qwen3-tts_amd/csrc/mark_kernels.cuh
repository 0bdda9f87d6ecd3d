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

// One push seen from workgroup wg of its n_wg: ceil(ceil(n_out / H) / 15) workgroups of 15 hops, and one more that keeps the history.
// Nothing in it looks at the grid, so the single kernel and the group kernel run the same code on a row.
__device__ __forceinline__ void mark_embed_body(const MarkPushArgs& a, const int wg, const int n_wg) {
    __shared__ float run[kMarkRunLds];
    __shared__ float D[kMarkRows * kMarkDLd];
    __shared__ float E[kMarkRows * kMarkELd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    if (wg == n_wg - 1) {
        float* hn = gptr(a.hist_next);
        for (int i = tid; i < a.keep; i += kMarkThreads) hn[i] = mark_sample(a.src, a.src.total - a.keep + i);
        return;
    }
    const int64_t hop0 = a.o0 / kMarkH + (int64_t)wg * kMarkHops;               // frame f of the tile is frame hop0 + f of the stream
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

__global__ void __launch_bounds__(kMarkThreads) mark_embed_kernel(const MarkPushArgs a) { mark_embed_body(a, (int)blockIdx.x, (int)gridDim.x); }

// ---- The pushes of up to 32 streams in ONE launch (fq3_mark_push_group) -----------------------------------------------------------------
// One packed 1-D grid over all rows: row b owns workgroups wg0[b] .. wg0[b + 1] - 1 -- its single push's grid, the history workgroup
// last -- and none when its push is empty and not final, so wg0 may hold equal neighbours.  A workgroup finds its row with the
// wave-uniform walk of mark_scan_row (the LAST row that starts at or before it, which steps over rows of no workgroups; entries past
// the last row hold the grid size), copies that row's descriptor out of the argument block into scalar registers and runs the single
// push's body on it: the tables travel once, key and strength per row.  The identity contract above makes a row's output and next
// history those of its single push, bit for bit, whatever the other rows are and wherever the row falls in the grid.
constexpr int kMarkGroupMax = 32;                   // FQ3_STAGE_GROUP_MAX

struct MarkGroupRow {
    MarkSrc src;
    float* hist_next;
    float* out;
    int64_t o0, n_out;
    int keep;
    float a;
    uint32_t k0, k1;
};

struct MarkGroupArgs {
    const float* fwd;
    const float* inv;
    int wg0[kMarkGroupMax + 1];                     // first workgroup of row b; wg0[b >= B] is the grid size
    MarkGroupRow rows[kMarkGroupMax];
};
static_assert(sizeof(MarkGroupRow) == 88 && sizeof(MarkGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

__global__ void __launch_bounds__(kMarkThreads) mark_embed_group_kernel(const MarkGroupArgs g) {
    const int wg = (int)blockIdx.x;
    int row = 0;
#pragma unroll
    for (int b = 1; b < kMarkGroupMax; ++b) row += wg >= g.wg0[b] ? 1 : 0;       // wg0 does not decrease: the last row that starts at or before wg
    const MarkGroupRow& r = g.rows[row];
    MarkPushArgs a;
    a.src = r.src; a.hist_next = r.hist_next; a.out = r.out; a.fwd = g.fwd; a.inv = g.inv;
    a.o0 = r.o0; a.n_out = r.n_out; a.keep = r.keep; a.a = r.a; a.k0 = r.k0; a.k1 = r.k1;
    mark_embed_body(a, wg - g.wg0[row], g.wg0[row + 1] - g.wg0[row]);
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

// ---- Scan: which windows of up to 32 clips carry the mark (fq3_mark_scan; include/fq3hip.h states the windows) -------------------------
// The detector's sums are kept per BLOCK of 16 d frames (block b: frames 1 + 16 b .. 16 + 16 b, cut at T - 2) instead of per clip, and
// a window is a sum over blocks: overlapping windows cost nothing in the kernel that does the DFTs.
//   blocks    one packed 1-D grid over all rows: part_wg0[b] is the first workgroup of row b (rows past the last hold the grid size,
//             as in flac_kernels.cuh); inside a row a workgroup is (range of R blocks, group of G of the 32 offsets).  It walks the
//             M tiles bt = b0 .. b1 of its range; tile bt holds L of frames 16 bt .. 16 bt + 15.
//   staging   the 32 offsets of a tile lie within 248 samples, so ONE run of 18 hops (17 + the offsets' reach) serves every offset of the
//             group: the forward product of offset o reads the run shifted by o, nothing is staged per offset.  From tile to tile the
//             run's last two hops are moved to its front inside the LDS and 16 new hops are read: every sample is read from memory once
//             per workgroup.  d of frame t needs L of t - 1 and t + 1: the last two L rows of a tile are kept per offset (Lp), so tile
//             bt yields d of frames 16 bt - 1 .. 16 bt + 14 -- the last two frames of block bt - 1 and the first 14 of block bt -- and no
//             frame's DFT is formed twice inside a range (a range costs one tile more than it has blocks, and not even that at the clip's
//             end when the tile would hold no frame up to T - 2).
//   chips     the correlation with the chips is a GEMM as well: g[16 frames][128 chip rows] = d[16][64] . C^T[64][128], K = 64 in 16
//             steps, wave w the chip rows 32 w .. 32 w + 31.  The B operand is never in memory: lane (fr, fq) of an N tile needs bits
//             4 ks + fq of ONE chip row, two Philox words it holds in registers for the whole kernel, and makes +-1.0f from a bit per
//             step.  The products are exact (+-d) and 64 of them are added in fp32 by the matrix core; frame t's contribution to phase p
//             is g[t][(t + p) mod 128], gathered from the LDS and added in double: 16 adds per phase and tile where mark_detect_kernel
//             spends 448 converts and adds per thread.
//   carry     block b's sums are closed by tile b + 1: (first 14 frames, carried in the LDS in double) + (last two frames).  The order
//             inside a block is fixed and no sum crosses a block, so S and E of a block do not depend on R, G, the range it fell in or
//             the other rows of the call, bit for bit.
//   windows   one workgroup per (row, window): the blocks' S and E in ascending order, z = S / sqrt(E), the optional table, and the
//             verdict (max z, the lowest index among equals) by a shuffle reduction.
constexpr int kMarkBlock = 16;                      // d frames of a scan block: one M tile
constexpr int kMarkScanMax = 32;                    // FQ3_STAGE_GROUP_MAX
constexpr int kMarkScanOffs = 8;                    // most offsets one workgroup walks over a staged run
constexpr int kMarkScanHops = kMarkRows + 2;        // 17 hops of 16 frames and one more for the offsets' reach (248 samples)
constexpr int kMarkScanRunLds = kMarkScanHops * (kMarkH + 4);
constexpr int kMarkDdLd = kMarkBins + 4, kMarkGLd = kMarkPeriod + 4;
constexpr int kMarkBlockDoubles = kMarkOffsets * kMarkPeriod + kMarkOffsets;     // a block's slot: S[32][128], then E[32]
constexpr int kMarkScanWinThreads = 256;

struct MarkVerdict { float z; int32_t offset, phase, present; };                // fq3_mark_window

struct MarkScanRow {
    const float* pcm;
    int n, T, NB, W;
    int blk0, win0;            // the row's first block / window in the packed workspace / outputs
    uint32_t k0, k1;
};

struct MarkScanArgs {
    const float* fwd;
    double* work;              // [sum NB][kMarkBlockDoubles]
    MarkVerdict* out;          // [sum W]
    float* tables;             // [sum W][32][128], or null
    int R, G;                  // blocks per range, offsets per workgroup (G divides 32, G <= kMarkScanOffs)
    int win_blocks, hop_blocks;
    int part_wg0[kMarkScanMax], win_wg0[kMarkScanMax];
    MarkScanRow rows[kMarkScanMax];
};
static_assert(sizeof(MarkScanRow) == 40 && sizeof(MarkScanArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

// mark_forward over the 18-hop run with every frame shifted by o samples: the same products in the same four chains (a copy, so that
// mark_forward and the kernels built on it stay untouched)
__device__ __forceinline__ void mark_forward_at(const float* run, const int o, const float* __restrict__ fwd, int wave, int lane, mark_f32x4& re_out,
                                                mark_f32x4& im_out) {
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
            const float a = run[mark_run_at(o + fr * kMarkH + (ks + c) * 4 + fq)];
            re[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tc[(ks + c) * 64], re[c], 0, 0, 0);
            im[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ts[(ks + c) * 64], im[c], 0, 0, 0);
        }
    re_out = (re[0] + re[1]) + (re[2] + re[3]);
    im_out = (im[0] + im[1]) + (im[2] + im[3]);
}

__device__ __forceinline__ int mark_scan_row(const int* wg0, const int wg) {
    int row = 0;
#pragma unroll
    for (int b = 1; b < kMarkScanMax; ++b) row += wg >= wg0[b] ? 1 : 0;         // wg0 does not decrease: the last row that starts at or before wg
    return row;
}

__global__ void __launch_bounds__(kMarkThreads) mark_scan_blocks_kernel(const MarkScanArgs a) {
    __shared__ float run[kMarkScanRunLds];
    __shared__ float L[kMarkRows * kMarkLLd];
    __shared__ float Lp[kMarkScanOffs][2][kMarkBins];          // per offset: L of the previous tile's frames 14 and 15
    __shared__ float Dd[kMarkRows * kMarkDdLd];
    __shared__ float Gm[kMarkRows * kMarkGLd];
    __shared__ double cS[kMarkScanOffs][kMarkPeriod];          // per offset: the open block's first 14 frames
    __shared__ double cE[kMarkScanOffs];
    __shared__ double Pb[kMarkPeriod];
    __shared__ double Ew[2][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wg = (int)blockIdx.x, row = mark_scan_row(a.part_wg0, wg);
    const MarkScanRow& r = a.rows[row];
    const int local = wg - a.part_wg0[row], groups = kMarkOffsets / a.G;
    const int og = local % groups, b0 = (local / groups) * a.R, b1 = min(b0 + a.R, r.NB);
    const MarkSrc src{r.pcm, nullptr, 0, 0, (int64_t)r.n};
    double* S = gptr(a.work) + (int64_t)r.blk0 * kMarkBlockDoubles;
    uint32_t cw[2][2];                                                          // the lane's two chip rows, 64 bits each
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int crow = 32 * wave + 16 * t + fr;
        cw[t][0] = mark_chip_word(crow, 0, r.k0, r.k1);
        cw[t][1] = mark_chip_word(crow, 32, r.k0, r.k1);
    }
    const int phase = tid & (kMarkPeriod - 1), hf = tid >> 7;
    for (int bt = b0; bt <= b1; ++bt) {
        const int tq0 = kMarkBlock * bt - 1;                                    // row q of the tile's d is frame tq0 + q
        if (bt == b1 && tq0 > r.T - 2) {                                        // the clip's end: no frame left for the open block
            for (int oi = 0; oi < a.G; ++oi) {
                double* slot = S + (int64_t)(bt - 1) * kMarkBlockDoubles;
                if (hf == 0) slot[(og * a.G + oi) * kMarkPeriod + phase] = cS[oi][phase];
                if (tid == 0) slot[kMarkOffsets * kMarkPeriod + og * a.G + oi] = cE[oi];
            }
            break;
        }
        const int64_t base = (int64_t)tq0 * kMarkH;
        if (bt == b0) {
            for (int p = tid; p < kMarkScanHops * kMarkH; p += kMarkThreads) run[mark_run_at(p)] = mark_sample(src, base + p);
        } else {
            float keep[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) keep[i] = run[kMarkRows * (kMarkH + 4) + min(tid + i * kMarkThreads, 2 * (kMarkH + 4) - 1)];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (tid + i * kMarkThreads < 2 * (kMarkH + 4)) run[tid + i * kMarkThreads] = keep[i];
            for (int p = 2 * kMarkH + tid; p < kMarkScanHops * kMarkH; p += kMarkThreads) run[mark_run_at(p)] = mark_sample(src, base + p);
        }
        __syncthreads();
        for (int oi = 0; oi < a.G; ++oi) {
            const int oidx = og * a.G + oi;
            mark_f32x4 re, im;
            mark_forward_at(run, oidx * kMarkOffsetStep, a.fwd, wave, lane, re, im);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                L[(4 * fq + q) * kMarkLLd + wave * 16 + fr] = logf(sqrtf(re[q] * re[q] + im[q] * im[q]) + 1e-9f);
            __syncthreads();
            double eA = 0.0, eB = 0.0;                                          // d^2 of the closing block (rows 0, 1) and of the open one
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = wave + 4 * i;                                     // d row q from L rows q - 2 .. q, rows -2 and -1 in Lp
                const float l0 = q >= 2 ? L[max(q - 2, 0) * kMarkLLd + lane] : Lp[oi][q & 1][lane];
                const float l1 = q >= 1 ? L[max(q - 1, 0) * kMarkLLd + lane] : Lp[oi][1][lane];
                float d = l1 - 0.5f * (l0 + L[q * kMarkLLd + lane]);
                d = fminf(fmaxf(d, -2.0f), 2.0f);
                const bool ok = tq0 + q >= 1 && tq0 + q <= r.T - 2 && (q >= 2 || bt > b0);
                d = ok ? d : 0.0f;
                Dd[q * kMarkDdLd + lane] = d;
                if (q < 2) eA += (double)d * (double)d; else eB += (double)d * (double)d;
            }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) { eA += __shfl_xor(eA, m); eB += __shfl_xor(eB, m); }
            if (lane == 0) { Ew[0][wave] = eA; Ew[1][wave] = eB; }
            __syncthreads();
            if (tid < 2 * kMarkBins) Lp[oi][tid >> 6][lane] = L[(kMarkRows - 2 + (tid >> 6)) * kMarkLLd + lane];
            mark_f32x4 g[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t) g[t][0] = g[t][1] = mark_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                const float av = Dd[fr * kMarkDdLd + ks * 4 + fq];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const uint32_t clear = (~cw[t][ks >> 3] >> ((ks & 7) * 4 + fq)) & 1u;
                    g[t][ks & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(0x3f800000u | (clear << 31)), g[t][ks & 1], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const mark_f32x4 gg = g[t][0] + g[t][1];
#pragma unroll
                for (int q = 0; q < 4; ++q) Gm[(4 * fq + q) * kMarkGLd + 32 * wave + 16 * t + fr] = gg[q];
            }
            __syncthreads();
            double sumA = 0.0, sumB = 0.0;                                      // rows 0, 1 close block bt - 1; rows 2 .. 15 open block bt
            if (hf == 0) {
                for (int q = 0; q < 2; ++q) sumA += (double)Gm[q * kMarkGLd + ((tq0 + q + phase) & (kMarkPeriod - 1))];
                for (int q = 2; q < 9; ++q) sumB += (double)Gm[q * kMarkGLd + ((tq0 + q + phase) & (kMarkPeriod - 1))];
            } else {
                for (int q = 9; q < kMarkRows; ++q) sumB += (double)Gm[q * kMarkGLd + ((tq0 + q + phase) & (kMarkPeriod - 1))];
                Pb[phase] = sumB;
            }
            __syncthreads();
            double* slot = S + (int64_t)(bt - 1) * kMarkBlockDoubles;           // written only when bt > b0
            if (hf == 0) {
                if (bt > b0) slot[oidx * kMarkPeriod + phase] = cS[oi][phase] + sumA;
                cS[oi][phase] = sumB + Pb[phase];
            }
            if (tid == 0) {
                if (bt > b0) slot[kMarkOffsets * kMarkPeriod + oidx] = cE[oi] + ((Ew[0][0] + Ew[0][1]) + (Ew[0][2] + Ew[0][3]));
                cE[oi] = (Ew[1][0] + Ew[1][1]) + (Ew[1][2] + Ew[1][3]);
            }
        }
    }
}

// grid: one workgroup per (row, window), packed as above
__global__ void __launch_bounds__(kMarkScanWinThreads) mark_scan_windows_kernel(const MarkScanArgs a) {
    __shared__ double Es[kMarkOffsets];
    __shared__ float bz[kMarkScanWinThreads / 64];
    __shared__ int bi[kMarkScanWinThreads / 64];
    constexpr int kPer = kMarkOffsets * kMarkPeriod / kMarkScanWinThreads;      // 16 table entries per thread
    const int tid = threadIdx.x, wg = (int)blockIdx.x, row = mark_scan_row(a.win_wg0, wg);
    const MarkScanRow& r = a.rows[row];
    const int w = wg - a.win_wg0[row];
    const int nb = min(r.NB, a.win_blocks), s = min(w * a.hop_blocks, r.NB - nb);
    const double* S = gptr(a.work) + (int64_t)(r.blk0 + s) * kMarkBlockDoubles;
    if (tid < kMarkOffsets) {
        double e = 0.0;
        for (int b = 0; b < nb; ++b) e += S[(int64_t)b * kMarkBlockDoubles + kMarkOffsets * kMarkPeriod + tid];
        Es[tid] = e;
    }
    double acc[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) acc[i] = 0.0;
    for (int b = 0; b < nb; ++b)
#pragma unroll
        for (int i = 0; i < kPer; ++i) acc[i] += S[(int64_t)b * kMarkBlockDoubles + tid + i * kMarkScanWinThreads];
    __syncthreads();
    float* tab = a.tables ? gptr(a.tables) + (int64_t)(r.win0 + w) * (kMarkOffsets * kMarkPeriod) : nullptr;
    float best = 0.0f;
    int at = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int idx = tid + i * kMarkScanWinThreads;
        const double e = Es[idx >> 7];
        const float z = e > 0.0 ? (float)(acc[i] / sqrt(e)) : 0.0f;
        if (tab) tab[idx] = z;
        if (i == 0 || z > best) { best = z; at = idx; }                         // ascending idx: the lowest index among equals stays
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float oz = __shfl_xor(best, m);
        const int oa = __shfl_xor(at, m);
        if (oz > best || (oz == best && oa < at)) { best = oz; at = oa; }
    }
    if ((tid & 63) == 0) { bz[tid >> 6] = best; bi[tid >> 6] = at; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < kMarkScanWinThreads / 64; ++v)
            if (bz[v] > best || (bz[v] == best && bi[v] < at)) { best = bz[v]; at = bi[v]; }
        MarkVerdict out;
        out.z = best; out.offset = (at >> 7) * kMarkOffsetStep; out.phase = at & (kMarkPeriod - 1); out.present = best >= 6.0f ? 1 : 0;
        gptr(a.out)[r.win0 + w] = out;
    }
}

}  // namespace fq3
