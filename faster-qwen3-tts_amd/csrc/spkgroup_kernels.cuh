// Speaker encoder, group form (fq3_refenc_speaker_group): the x-vectors of up to 32 clips of different lengths in a number of
// launches that does not depend on how many clips there are, and the cosine of embedding pairs (fq3_refenc_similarity).
// DESIGN.md section 4.25.
//
// Rows.  Clip b has F_b log-mel frames.  Two packed row spaces serve the whole stack:
//   compact   clip b's frames at rows frow_b .. frow_b + F_b - 1, the clips back to back (the log-mel output [sum F][mel_dim]);
//   gapped    clip b's frames at rows prow_b .. prow_b + F_b - 1 with prow_b = frow_b + b * gap, gap = the widest (k - 1) * dilation
//             of the stack.  Every activation of the TDNN stack lives here.  A layer with k taps first writes the clip's
//             reflect-padded rows (F_b + 2 pad <= F_b + gap of them) from prow_b on -- spk_pad_group_kernel, the clip's own
//             reflection at both of its ends -- and the tap GEMM over ALL rows then reads rows m + i * dilation for output row m:
//             output row prow_b + t sees exactly the padded rows of clip b.  The gap rows are computed from whatever the buffers hold
//             and never read: a GEMM output row depends on its own A rows only, and every kernel below walks a clip's own rows.
// The dense products are conv_gemm_kernel<float, 64, 64> (gemm_launch<float> has that one fp32 tile, whatever the row count), whose
// per-element MFMA chain does not depend on where the row sits: a clip's numbers are those of any other placement.
//
// Launches use the group convention of mark_kernels.cuh / flac_kernels.cuh: row descriptors by value, one packed 1-D grid with a table
// of first workgroups (entries past the last row hold the grid size), and a wave-uniform walk that steps over rows of no workgroups.
#pragma once
#include "refenc_kernels.cuh"

namespace fq3 {

constexpr int kSpkGroupMax = 32;                 // FQ3_STAGE_GROUP_MAX
constexpr int kMelTile = 32;                     // frames per workgroup of the front end: two 16-row MFMA tiles share every table operand
constexpr int kMelWaves = 8;
constexpr int kSpkLdPad = 4;                     // LDS row padding (floats): lane (row, k) of an A operand load goes to bank 4 row + k

struct SpkRow {
    const float* pcm;
    int n, F;                                    // samples, log-mel frames
    int frow, prow;                              // first row in the compact / the gapped row space
};
struct SpkGroupArgs {
    SpkRow rows[kSpkGroupMax];
    int wg0[kSpkGroupMax + 1];                   // first workgroup of row b in THIS launch; wg0[b >= n_rows] is the grid size
    int n_rows;
};
static_assert(sizeof(SpkRow) == 24 && sizeof(SpkGroupArgs) <= 1024, "the descriptors travel in the argument block");

__device__ __forceinline__ int spk_row_of(const int* wg0, const int wg) {
    int row = 0;
#pragma unroll
    for (int b = 1; b < kSpkGroupMax; ++b) row += wg >= wg0[b] ? 1 : 0;          // wg0 does not decrease: the last row that starts at or before wg
    return row;
}

// torch "reflect" (no edge repeat) of index t into [0, T); the clamp is reachable only past a clip's padded extent (tile tails)
__device__ __forceinline__ int spk_reflect(int t, const int T) {
    if (t < 0) t = -t;
    if (t >= T) t = 2 * (T - 1) - t;
    return t < 0 ? 0 : (t >= T ? T - 1 : t);
}

// Fragment-major copy of a row-major operand table src [R][K] (R, K multiples of 16) for v_mfma_f32_16x16x4_f32's B operand:
//   dst[((rb * K/16 + kq) * 64 + lane) * 4 + j] = src[rb * 16 + (lane & 15)][kq * 16 + j * 4 + (lane >> 4)]
// so one float4 per lane -- 1 KB contiguous per wave -- holds the operands of four consecutive K steps of a 16-row block.
__global__ void spk_frag_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)R * K) return;
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const long t = i >> 8;
    const int kq = (int)(t % (K / 16)), rb = (int)(t / (K / 16));
    dst[i] = src[(size_t)(rb * 16 + (lane & 15)) * K + kq * 16 + j * 4 + (lane >> 4)];
}

// ---- packed log-mel front end: pcm of every clip -> mel [sum F][mel_dim], one launch -------------------------------------------------
// A workgroup owns kMelTile frames of one clip.
//   staging    the tile's (kMelTile - 1) * hop + n_fft samples go to LDS once, as (kMelTile - 1 + n_fft / hop) chunks of hop samples in rows
//              of hop + 4 floats; the reflect padding of the clip's ends is resolved in the load index (no padded signal exists).
//              Frame f, sample k of the window = chunk f + k / hop, column k % hop: the A operand of K step k (lanes: frame = lane & 15,
//              k + (lane >> 4)) is one conflict-free ds_read per 16-frame tile.
//   DFT        wave w takes the 16-bin blocks w, w + 8, ...: for each, the re and the im accumulators of both frame tiles (4 x f32x4)
//              against the fragment-major table, K ascending in steps of 4 -- the chain of the single path's tap GEMM.
//   magnitude  sqrt(re^2 + im^2 + 1e-9) in registers (re and im of a bin sit in the same lane), parked in LDS [kMelTile][NB + 4].
//   mel, log   after one barrier: wave w takes the 16-filter blocks w, w + 8, ... of the second product out of LDS, log(max(v, 1e-5)).
// Dynamic LDS: ((kMelTile - 1 + n_fft / hop) * (hop + 4) + kMelTile * (NB + 4)) floats: 104 KB at n_fft 1024, hop 256.
__global__ __launch_bounds__(kMelWaves * 64) void spk_logmel_group_kernel(const SpkGroupArgs g, const float* __restrict__ dft_frag,
                                                                         const float* __restrict__ mel_frag, float* __restrict__ mel,
                                                                         int n_fft, int hop, int NB, int mel_dim) {
    extern __shared__ __attribute__((aligned(16))) float spk_sm[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wg = (int)blockIdx.x, row = spk_row_of(g.wg0, wg);
    const SpkRow& r = g.rows[row];
    const int f0 = (wg - g.wg0[row]) * kMelTile, nf = min(kMelTile, r.F - f0);
    const int taps = n_fft / hop, chunks = kMelTile - 1 + taps, ldc = hop + kSpkLdPad, ldm = NB + kSpkLdPad;
    float* sig = spk_sm;
    float* mag = spk_sm + chunks * ldc;
    const int s0 = f0 * hop - (n_fft - hop) / 2;             // clip index of the tile's first sample (negative: inside the left reflection)
    for (int c = wave; c < chunks; c += kMelWaves)
        for (int w = lane; w < hop; w += 64) sig[c * ldc + w] = r.pcm[spk_reflect(s0 + c * hop + w, r.n)];
    __syncthreads();
    const int kq_n = n_fft / 16, nblk = NB / 16;
    const float4* tab = reinterpret_cast<const float4*>(dft_frag);
    for (int b = wave; b < nblk; b += kMelWaves) {
        f32x4_t re[2], im[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) { re[i] = f32x4_t{0.f, 0.f, 0.f, 0.f}; im[i] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
        const float4* pre = tab + (size_t)b * kq_n * 64 + lane;
        const float4* pim = tab + (size_t)(nblk + b) * kq_n * 64 + lane;
        for (int tap = 0; tap < taps; ++tap) {
            const float* a0 = sig + (fr + tap) * ldc + fq;
            for (int kw = 0; kw < hop; kw += 16) {
                const float4 wre = *pre, wim = *pim;
                pre += 64; pim += 64;
                const float wr[4] = {wre.x, wre.y, wre.z, wre.w}, wi[4] = {wim.x, wim.y, wim.z, wim.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x0 = a0[kw + j * 4], x1 = a0[16 * ldc + kw + j * 4];
                    re[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, wr[j], re[0], 0, 0, 0);
                    re[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, wr[j], re[1], 0, 0, 0);
                    im[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, wi[j], im[0], 0, 0, 0);
                    im[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, wi[j], im[1], 0, 0, 0);
                }
            }
        }
        // C/D layout: column (bin) = lane & 15, row (frame) = (lane >> 4) * 4 + reg
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float re_ = re[i][q], im_ = im[i][q];
                mag[(i * 16 + fq * 4 + q) * ldm + b * 16 + fr] = sqrtf(re_ * re_ + im_ * im_ + 1e-9f);
            }
    }
    __syncthreads();
    const float4* bas = reinterpret_cast<const float4*>(mel_frag);
    for (int cb = wave; cb < mel_dim / 16; cb += kMelWaves) {
        f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
        const float4* pw = bas + (size_t)cb * nblk * 64 + lane;
        const float* a0 = mag + fr * ldm + fq;
        for (int kq = 0; kq < nblk; ++kq) {
            const float4 wv = pw[(size_t)kq * 64];
            const float w4[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[kq * 16 + j * 4], w4[j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[16 * ldm + kq * 16 + j * 4], w4[j], acc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int f = i * 16 + fq * 4 + q;
                if (f < nf) mel[(size_t)(r.frow + f0 + f) * mel_dim + cb * 16 + fr] = logf(fmaxf(acc[i][q] + 0.f, 1e-5f));
            }
    }
}

// ---- reflect-padded rows of every clip, back to back (the group form of pad_rows_kernel, mode 0) ------------------------------------
// dst[prow_b + p][c] = src1[base_b + t][c] (+ src2[base_b + t][c]), p in [0, F_b + 2 pad), t = reflect(p - pad) in [0, F_b);
// base_b = frow_b (compact source: the log-mel frames) or prow_b.  C % 4 == 0 and 16-byte aligned slices: float4 accesses.
// Row b owns ceil((F_b + 2 pad) * C / 4 / 256) workgroups.
__global__ __launch_bounds__(256) void spk_pad_group_kernel(const SpkGroupArgs g, const float* __restrict__ src1, int ld1, const float* __restrict__ src2, int ld2,
                                                           int compact, float* __restrict__ dst, int C, int pad) {
    const int wg = (int)blockIdx.x, row = spk_row_of(g.wg0, wg);
    const SpkRow& r = g.rows[row];
    const int c4n = C / 4;
    const long i = (long)(wg - g.wg0[row]) * 256 + threadIdx.x;
    if (i >= (long)(r.F + 2 * pad) * c4n) return;
    const int p = (int)(i / c4n), c = (int)(i - (long)p * c4n) * 4;
    const size_t t = (size_t)(compact ? r.frow : r.prow) + spk_reflect(p - pad, r.F);
    float4 v = *reinterpret_cast<const float4*>(src1 + t * ld1 + c);
    if (src2) {
        const float4 u = *reinterpret_cast<const float4*>(src2 + t * ld2 + c);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    *reinterpret_cast<float4*>(dst + ((size_t)r.prow + p) * C + c) = v;
}

// ---- segmented statistics: col_stats_kernel's arithmetic per (clip, block of 64 channels) --------------------------------------------
// Row b owns ceil(C / 64) workgroups; each walks the clip's own F_b rows in col_stats_body's fixed order (16 time slices, summed in
// slice order).  mean / stdv are [rows][ldo].  logits: the attentive pooling's softmax over the clip's own frames.
__global__ __launch_bounds__(64 * kStatSlices) void spk_stats_group_kernel(const SpkGroupArgs g, const float* __restrict__ x, int ldx,
                                                                          const float* __restrict__ logits, int ldl, float* __restrict__ mean,
                                                                          float* __restrict__ stdv, int ldo, int C, float eps) {
    const int wg = (int)blockIdx.x, row = spk_row_of(g.wg0, wg);
    const SpkRow& r = g.rows[row];
    col_stats_body(x + (size_t)r.prow * ldx, ldx, logits ? logits + (size_t)r.prow * ldl : nullptr, ldl, mean ? mean + (size_t)row * ldo : nullptr,
                   stdv ? stdv + (size_t)row * ldo : nullptr, r.F, C, eps, wg - g.wg0[row]);
}

// ---- per-clip channel vectors applied to the clip's rows ----------------------------------------------------------------------------
// MODE 0 (se_scale_kernel's group form): y[t][c] = x[t][c] * vec[b][c] + res[t][c]
// MODE 1 (the attention TDNN's bias, which holds the clip's [mean | std] projection): y[t][c] = tanh(max(x[t][c] + vec[b][c], 0)), in place
// Row b owns ceil(F_b * C / 4 / 256) workgroups; t runs over the gapped rows prow_b ..
template <int MODE>
__global__ __launch_bounds__(256) void spk_rowvec_group_kernel(const SpkGroupArgs g, const float* __restrict__ x, int ldx, const float* __restrict__ vec, int ldv,
                                                              const float* __restrict__ res, int ldr, float* __restrict__ y, int ldy, int C) {
    const int wg = (int)blockIdx.x, row = spk_row_of(g.wg0, wg);
    const SpkRow& r = g.rows[row];
    const int c4n = C / 4;
    const long i = (long)(wg - g.wg0[row]) * 256 + threadIdx.x;
    if (i >= (long)r.F * c4n) return;
    const int tl = (int)(i / c4n), c = (int)(i - (long)tl * c4n) * 4;
    const size_t t = (size_t)r.prow + tl;
    const float4 xv = *reinterpret_cast<const float4*>(x + t * ldx + c);
    const float4 gv = *reinterpret_cast<const float4*>(vec + (size_t)row * ldv + c);
    float4 o;
    if constexpr (MODE == 0) {
        const float4 rv = *reinterpret_cast<const float4*>(res + t * ldr + c);
        o.x = xv.x * gv.x + rv.x; o.y = xv.y * gv.y + rv.y; o.z = xv.z * gv.z + rv.z; o.w = xv.w * gv.w + rv.w;
    } else {
        o.x = tanhf(fmaxf(xv.x + gv.x, 0.f)); o.y = tanhf(fmaxf(xv.y + gv.y, 0.f));
        o.z = tanhf(fmaxf(xv.z + gv.z, 0.f)); o.w = tanhf(fmaxf(xv.w + gv.w, 0.f));
    }
    *reinterpret_cast<float4*>(y + t * ldy + c) = o;
}

// ---- cosine of `rows` embedding pairs: a wave per row -------------------------------------------------------------------------------
// Lane l sums elements l, l + 64, ... in four interleaved fp32 chains (element l + 64 j goes to chain j % 4), the chains are added
// ((0 + 1) + (2 + 3)) and the lanes by the xor butterfly: a fixed order.  A zero vector on either side gives 0.
__global__ __launch_bounds__(256) void spk_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int rows, int dim) {
    const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* pa = a + (size_t)row * dim;
    const float* pb = b + (size_t)row * dim;
    float ab[4] = {0.f, 0.f, 0.f, 0.f}, aa[4] = {0.f, 0.f, 0.f, 0.f}, bb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = lane; d0 < dim; d0 += 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = d0 + 64 * j;
            const float u = d < dim ? pa[d] : 0.f, v = d < dim ? pb[d] : 0.f;
            ab[j] = fmaf(u, v, ab[j]); aa[j] = fmaf(u, u, aa[j]); bb[j] = fmaf(v, v, bb[j]);
        }
    }
    const float sab = wave_sum((ab[0] + ab[1]) + (ab[2] + ab[3]));
    const float saa = wave_sum((aa[0] + aa[1]) + (aa[2] + aa[3]));
    const float sbb = wave_sum((bb[0] + bb[1]) + (bb[2] + bb[3]));
    if (lane == 0) out[row] = (saa > 0.f && sbb > 0.f) ? sab / (sqrtf(saa) * sqrtf(sbb)) : 0.f;
}

}  // namespace fq3
