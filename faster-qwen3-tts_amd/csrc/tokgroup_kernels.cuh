// Speech-tokenizer encoder, group form (fq3_refenc_encode_group): the reference codes of up to 32 clips of different lengths in a
// number of launches that does not depend on how many clips there are.  DESIGN.md section 4.26.
//
// Rows.  P = prod(ratios) samples make one 25 Hz row.  Clip b with t25_b rows at 25 Hz owns the SLOT of 25 Hz rows [lo25_b, p25_b + t25_b):
// a leading gap [lo25_b, p25_b) of at least g25 rows, then its own rows from the EVEN row p25_b on; lo25_b is where clip b - 1 ended.
// At the stage whose rows are R samples long (R = the product of the ratios passed so far, R divides P) the same slot is rows
// [lo25_b P / R, (p25_b + t25_b) P / R), the clip's first row is p25_b P / R and it has T rows, T = the single call's length at that stage
// (T R <= t25_b P, so the clip and the zero tail a strided conv wants behind it stay inside the slot).  Two invariants:
//   causality   every row of the slot that is not one of the clip's T rows is ZERO in every buffer a conv with more than one tap reads;
//               g25 P / R is at least that stage's reach (k - 1) dilation (a strided conv: one view row = its ratio), so the taps that
//               the single call reads as zeros in front of row 0 read zeros here;
//   alignment   p25_b is even, so the clip's first row is a multiple of every stage's ratio and of the 2 of the stride-2 conv: the
//               [T / r][r C] view of the packed rows cuts every clip where its own view would.
// The dense products run once over ALL rows through conv_gemm_kernel<float, 64, 64> (gemm_launch<float> has that one fp32 tile, whatever
// the row count), whose per-element MFMA chain does not depend on where the row sits.  They write bias and ELU into the gap rows, so
// tok_clear_kernel zeroes the non-clip rows of the activated buffer again after every product whose output a tap conv reads.
//
// Launches use the group convention of spkgroup_kernels.cuh: row descriptors by value, one packed 1-D grid with a table of first
// workgroups (entries past the last row hold the grid size), and a wave-uniform walk that steps over rows of no workgroups.
#pragma once
#include "refenc_kernels.cuh"

namespace fq3 {

constexpr int kTokGroupMax = 32;                 // FQ3_STAGE_GROUP_MAX
constexpr int kTokTile = 256;                    // packed samples per workgroup of the front stage

struct TokRow {
    const float* pcm;
    int64_t* codes;                              // [t5][num_quantizers]
    int n, t25, t5;                              // samples, 25 Hz rows, 12.5 Hz frames
    int lo25, p25;                               // the slot's first 25 Hz row, the clip's first 25 Hz row (even)
    int q;                                       // first row of the clip's replicate-padded rows (2 + 2 t5 of them; even)
};
struct TokGroupArgs {
    TokRow rows[kTokGroupMax];
    int wg0[kTokGroupMax + 1];                   // first workgroup of row b in THIS launch; wg0[b >= n_rows] is the grid size
    int n_rows;
};
// the non-clip rows of one stage: span j lies in front of clip j, span n_rows behind the last clip
struct TokSpans {
    int lo[kTokGroupMax + 1], hi[kTokGroupMax + 1];
    int wg0[kTokGroupMax + 2];
};
static_assert(sizeof(TokRow) == 40 && sizeof(TokGroupArgs) <= 2048 && sizeof(TokSpans) <= 512, "the descriptors travel in the argument block");

__device__ __forceinline__ int tok_row_of(const int* wg0, const int wg) {
    int row = 0;
#pragma unroll
    for (int b = 1; b < kTokGroupMax; ++b) row += wg >= wg0[b] ? 1 : 0;          // wg0 does not decrease: the last row that starts at or before wg
    return row;
}

// ---- packed front stage: conv_in_kernel over every slot, one launch ------------------------------------------------------------------
// Row b owns ceil(slot samples / kTokTile) workgroups.  A workgroup stages its tile of samples plus the K - 1 causal halo in LDS once
// (zeros before the clip's first and behind its last sample) and serves all C channels from it: a thread keeps the K taps and the bias of
// four neighbouring channels in registers and walks the tile in steps of 256 / (C / 4) samples, one float4 per output and store.  The
// samples of the slot that are not the clip's -- the gap in front and the tail behind -- get zeros in both outputs: this kernel owns the
// first zeroing of the gap rows.  Per element the chain is conv_in_kernel's: acc = bias, then fmaf in ascending tap order over the taps
// that do not reach in front of the clip.
__global__ __launch_bounds__(256) void tok_conv_in_group_kernel(const TokGroupArgs g, const float* __restrict__ w, const float* __restrict__ b,
                                                               float* __restrict__ y, float* __restrict__ e, int C, int K, int P) {
    __shared__ float xs[kTokTile + kMaxTaps];
    const int tid = threadIdx.x, wg = (int)blockIdx.x, row = tok_row_of(g.wg0, wg);
    const TokRow& r = g.rows[row];
    const long slot1 = (long)(r.p25 + r.t25) * P;
    const long R0 = (long)r.lo25 * P + (long)(wg - g.wg0[row]) * kTokTile;       // the tile's first packed sample
    const int nt = (int)min((long)kTokTile, slot1 - R0);
    const int t0 = (int)(R0 - (long)r.p25 * P);                                   // ... and its index in the clip (negative: inside the gap)
    for (int j = tid; j < nt + K - 1; j += 256) {
        const int t = t0 - (K - 1) + j;
        xs[j] = (t >= 0 && t < r.n) ? r.pcm[t] : 0.f;
    }
    __syncthreads();
    const int c4n = C / 4, spp = 256 / c4n;
    if (tid >= spp * c4n) return;
    const int c = (tid % c4n) * 4;
    float wr[4][kMaxTaps], bi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bi[q] = b[c + q];
#pragma unroll
        for (int k = 0; k < kMaxTaps; ++k) wr[q][k] = k < K ? w[(c + q) * K + k] : 0.f;
    }
    for (int i = tid / c4n; i < nt; i += spp) {
        const int t = t0 + i;
        float yo[4] = {0.f, 0.f, 0.f, 0.f}, eo[4] = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < r.n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float acc = bi[q];
#pragma unroll
                for (int k = 0; k < kMaxTaps; ++k)
                    if (k < K && t - (K - 1) + k >= 0) acc = fmaf(wr[q][k], xs[i + k], acc);
                yo[q] = acc;
                eo[q] = elu1(acc);
            }
        }
        const size_t o = (size_t)(R0 + i) * C + c;
        *reinterpret_cast<float4*>(y + o) = make_float4(yo[0], yo[1], yo[2], yo[3]);
        *reinterpret_cast<float4*>(e + o) = make_float4(eo[0], eo[1], eo[2], eo[3]);
    }
}

// ---- zero the non-clip rows of buf [rows][C]: span j owns ceil((hi_j - lo_j) C / 4 / 256) workgroups ---------------------------------
__global__ __launch_bounds__(256) void tok_clear_kernel(const TokSpans sp, float* __restrict__ buf, int C) {
    const int wg = (int)blockIdx.x;
    int j = 0;
#pragma unroll
    for (int b = 1; b <= kTokGroupMax; ++b) j += wg >= sp.wg0[b] ? 1 : 0;
    const long n4 = (long)(sp.hi[j] - sp.lo[j]) * (C / 4);
    const long i = (long)(wg - sp.wg0[j]) * 256 + threadIdx.x;
    if (i >= n4) return;
    *reinterpret_cast<float4*>(buf + (size_t)sp.lo[j] * C + (size_t)i * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- RoPE on the q and k thirds of every clip's rows, position = the row's index IN ITS CLIP (rope_rows_kernel<float>'s arithmetic) ---
// Row b owns ceil(t25_b * 2 (QD / HD) (HD / 2) / 256) workgroups.
__global__ __launch_bounds__(256) void tok_rope_group_kernel(const TokGroupArgs g, float* qkv, const float* __restrict__ cos_tab,
                                                            const float* __restrict__ sin_tab, int QD, int HD) {
    const int wg = (int)blockIdx.x, row = tok_row_of(g.wg0, wg);
    const TokRow& r = g.rows[row];
    const size_t i = (size_t)(wg - g.wg0[row]) * 256 + threadIdx.x;
    const int half = HD / 2, per_row = 2 * (QD / HD) * half;
    if (i >= (size_t)r.t25 * per_row) return;
    const int t = (int)(i / per_row), rr = (int)(i % per_row);
    const int head = rr / half, j = rr % half;            // heads 0..QD/HD-1 = q, then k
    float* p = qkv + (size_t)(r.p25 + t) * 3 * QD + (size_t)head * HD;
    const float cs = cos_tab[(size_t)t * half + j], sn = sin_tab[(size_t)t * half + j];
    const float x0 = DT<float>::ld(p + j), x1 = DT<float>::ld(p + j + half);
    DT<float>::st(p + j, DT<float>::rnd(x0 * cs) + DT<float>::rnd(-x1 * sn));
    DT<float>::st(p + j + half, DT<float>::rnd(x1 * cs) + DT<float>::rnd(x0 * sn));
}

// ---- causal sliding-window attention per clip: win_attn_body on the clip's own rows ------------------------------------------------------
// Grid (sum ceil(t25_b / 4), heads).  Keys stay inside the query's clip because the body sees the clip's rows as rows 0 .. t25_b - 1.
// NP covers the longest clip of the group; a pass past a shorter clip's keys adds exact zeros to its sums.
template <int HD, int NP>
__global__ __launch_bounds__(256) void tok_attn_group_kernel(const TokGroupArgs g, const float* __restrict__ qkv, float* __restrict__ out,
                                                            int NH, int window, float scale) {
    const int wg = (int)blockIdx.x, row = tok_row_of(g.wg0, wg);
    const TokRow& r = g.rows[row];
    const int QD = NH * HD;
    win_attn_body<HD, NP>(qkv + (size_t)r.p25 * 3 * QD, out + (size_t)r.p25 * QD, r.t25, NH, window, scale, wg - g.wg0[row], (int)blockIdx.y);
}

// ---- the stride-2 conv's replicate padding per clip (pad_rows_kernel mode 1, pad_l = 2): dst rows q_b .. q_b + 2 + 2 t5_b ---------------
// dst[q_b + p][c] = x[p25_b + clamp(p - 2, 0, t25_b - 1)][c].  Row b owns ceil((2 + 2 t5_b) C / 4 / 256) workgroups.
__global__ __launch_bounds__(256) void tok_pad_group_kernel(const TokGroupArgs g, const float* __restrict__ x, float* __restrict__ dst, int C) {
    const int wg = (int)blockIdx.x, row = tok_row_of(g.wg0, wg);
    const TokRow& r = g.rows[row];
    const int c4n = C / 4;
    const long i = (long)(wg - g.wg0[row]) * 256 + threadIdx.x;
    if (i >= (long)(2 + 2 * r.t5) * c4n) return;
    const int p = (int)(i / c4n), c = (int)(i - (long)p * c4n) * 4;
    int t = p - 2;
    t = t < 0 ? 0 : (t >= r.t25 ? r.t25 - 1 : t);
    *reinterpret_cast<float4*>(dst + ((size_t)r.q + p) * C + c) = *reinterpret_cast<const float4*>(x + ((size_t)r.p25 + t) * C + c);
}

// ---- split residual VQ of every clip's frames: rvq_encode_body per (clip, frame, quantizer group) -----------------------------------------
// Grid (sum t5_b, 2).  Frame t of clip b reads row q_b / 2 + t of proj [view rows][2 D] and writes codes_b[t][*].
template <int VEC, int PER>
__global__ __launch_bounds__(256) void tok_rvq_group_kernel(const TokGroupArgs g, RvqEncArgs a, const float* __restrict__ proj) {
    const int wg = (int)blockIdx.x, row = tok_row_of(g.wg0, wg);
    const TokRow& r = g.rows[row];
    const int t = wg - g.wg0[row];
    rvq_encode_body<VEC, PER>(a, proj + ((size_t)(r.q / 2) + t) * 2 * a.D, r.codes + (size_t)t * a.nq, (int)blockIdx.y);
}

}  // namespace fq3
