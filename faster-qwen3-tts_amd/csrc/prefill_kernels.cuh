// Kernels of the matrix-core prefill of the talker (fq3_prefill.hip holds the host side: paged_kv, pack_seq and the launch choosers):
// head RMSNorm + RoPE + K/V write into the paged cache, the per-row wave attention kernel and the flash-style MFMA attention kernels.
// A header of their own so that a conformance probe (tools/microbench/prefill_attn_probe.hip) can launch each of them alone.
// Shared bodies: flash_tile (one key tile of every flash kernel) and flash_acc_init.  The remaining arithmetic -- norm + RoPE + store,
// the wave-attention loop, the K/V staging with the transposed V store, the epilogues, the merge loop -- is written out in each
// kernel of its family ON PURPOSE: moved into __forceinline__ functions it compiles to other instruction streams and register counts
// than the text in place (even the two-line sequence lookup does), and these kernels are kept at their measured code.  The copies must
// stay the same instructions on the same values in the same order: the bit-equality tests between the families
// (tests/test_gpu_prefill_*_reference.py, tests/test_gpu_prefix_cache*.py) hold them to it, so a fix to one copy goes into all of them.
// Host side: flash_cont_splits is flash_cont_pack_splits for a pack of one.
#pragma once
#include "decode_kernels.cuh"
#include "codec_kernels.cuh"

namespace fq3 {

// One layer of a context's paged talker cache (fq3_ctx.h): pool arrays [n_blocks][n_kv][64][128], the block table, elements per block.
// Row `key` of kv head g: base + table[key / 64] * blk_stride + (g * 64 + key % 64) * 128.
template <typename T> struct PagedKV { T* k; T* v; const int* table; int blk_stride; };
template <typename T>
__device__ __forceinline__ size_t paged_row(const PagedKV<T>& kv, int g, int key) {
    return (size_t)kv.table[key / kKeysPerTile] * kv.blk_stride + ((size_t)g * kKeysPerTile + key % kKeysPerTile) * kHeadDim;
}

// per (token, head): RMSNorm over 128 + RoPE for q (in place) and k (-> cache); v copied to the cache
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_kernel(T* qkv, const T* qw, const T* kw, float eps, const float* cos_tab,
                                                              const float* sin_tab, int rope_len, int rope_delta, PagedKV<T> kv,
                                                              int L, int n_pad, int NH, int NKV) {
    constexpr int HD = kHeadDim;
    const int per = NH + 2 * NKV;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= L * per) return;
    const int t = w / per, v = w - t * per;
    if (t < n_pad) return;
    T* src = qkv + (size_t)t * per * HD + (size_t)v * HD;
    float x0 = DT<T>::ld(src + lane), x1 = DT<T>::ld(src + lane + 64);
    if (v < NH + NKV) {
        const T* gw = v < NH ? qw : kw;
        const float ss = wave_sum(fmaf(x0, x0, x1 * x1));
        const float rs = 1.0f / sqrtf(ss / (float)HD + eps);
        const float n0 = DT<T>::rnd(DT<T>::ld(gw + lane) * DT<T>::rnd(x0 * rs));
        const float n1 = DT<T>::rnd(DT<T>::ld(gw + lane + 64) * DT<T>::rnd(x1 * rs));
        int rp = t + rope_delta;
        rp = rp < 0 ? 0 : (rp >= rope_len ? rope_len - 1 : rp);
        const float cs = cos_tab[(size_t)rp * 64 + lane], sn = sin_tab[(size_t)rp * 64 + lane];
        x0 = DT<T>::rnd(DT<T>::rnd(n0 * cs) + DT<T>::rnd(-n1 * sn));
        x1 = DT<T>::rnd(DT<T>::rnd(n1 * cs) + DT<T>::rnd(n0 * sn));
    }
    T* dst = v < NH ? src : (v < NH + NKV ? kv.k + paged_row(kv, v - NH, t) : kv.v + paged_row(kv, v - NH - NKV, t));
    DT<T>::st(dst + lane, x0);
    DT<T>::st(dst + lane + 64, x1);
}

// causal attention for the prompt: one wave per (query row, q head); 16 lanes per key (8 dims each),
// 16 keys in flight per trip; fp32 online softmax, one rounding at the end.
template <typename T>
__global__ __launch_bounds__(256) void prefill_attn_kernel(const T* qkv, PagedKV<T> kv, T* out,
                                                           int L, int n_pad, int NH, int NKV, float scale) {
    constexpr int HD = kHeadDim;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= L * NH) return;
    const int t = w / NH, h = w - t * NH;
    const int per = NH + 2 * NKV, g = h / (NH / NKV);
    const int sub = lane >> 4, c = lane & 15;
    T* op = out + ((size_t)t * NH + h) * HD;
    if (t < n_pad) {
        if (sub == 0)
#pragma unroll
            for (int i = 0; i < 8; ++i) DT<T>::st(op + c * 8 + i, 0.f);
        return;
    }
    Raw8<T> qraw;
    ldraw<false>(qraw, qkv + (size_t)t * per * HD + (size_t)h * HD + c * 8);
    float q[8];
    unpack(qraw, q);
    float m = -1e30f, l = 0.f, o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = 0.f;
    for (int k0 = n_pad; k0 <= t; k0 += 16) {
        Raw8<T> kr[4], vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int key = k0 + i * 4 + sub;
            key = key <= t ? key : t;
            const size_t off = paged_row(kv, g, key) + c * 8;
            ldraw<false>(kr[i], kv.k + off);
            ldraw<false>(vr[i], kv.v + off);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool valid = k0 + i * 4 + sub <= t;
            float kf[8], vf[8];
            unpack(kr[i], kf); unpack(vr[i], vf);
            float sc = 0.f;
#pragma unroll
            for (int d = 0; d < 8; ++d) sc = fmaf(q[d], kf[d], sc);
            sc += __shfl_xor(sc, 1, 64); sc += __shfl_xor(sc, 2, 64);
            sc += __shfl_xor(sc, 4, 64); sc += __shfl_xor(sc, 8, 64);
            sc = valid ? sc * scale : -INFINITY;
            const float mn = fmaxf(m, sc), al = __expf(m - mn), p = __expf(sc - mn);
            l = fmaf(l, al, p);
#pragma unroll
            for (int d = 0; d < 8; ++d) o[d] = fmaf(o[d], al, valid ? p * vf[d] : 0.f);
            m = mn;
        }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(l, off, 64);
        const float M = fmaxf(m, mo), wa = __expf(m - M), wb = __expf(mo - M);
        l = l * wa + lo * wb;
#pragma unroll
        for (int d = 0; d < 8; ++d) { const float oo = __shfl_xor(o[d], off, 64); o[d] = o[d] * wa + oo * wb; }
        m = M;
    }
    if (sub == 0)
#pragma unroll
        for (int i = 0; i < 8; ++i) DT<T>::st(op + c * 8 + i, o[i] / l);
}

// ---------------------------------------------------------------------------------------------------------------------
// Flash-style causal attention on the matrix cores (bf16 contexts; long prompts: BASELINE configs[4], 4k tokens).
// One workgroup = one q head x 64 queries (16 per wave); key tiles of 64 keys stream through LDS (K row-major, V
// TRANSPOSED so that both MFMAs read 16-byte fragments); S = Q K^T and O += P V on v_mfma_f32_16x16x32_bf16, online
// softmax in fp32 on the accumulator layout (row statistics by DPP inside the 16-lane groups).  The probabilities enter
// the second MFMA as bf16, which the oracle's fp32 softmax(QK^T) V does not round: P is therefore split into a bf16 high
// part and a bf16 residual (two MFMAs), leaving a 2^-16 relative error instead of 2^-9 -- below the one rounding to T of
// the output.  The next tile's K/V global loads are issued before the current tile's arithmetic (register staging).
// fp32 contexts keep prefill_attn_kernel (exact fp32 products).
// ---------------------------------------------------------------------------------------------------------------------
// CONTRACT: P = 0 is multiplied by whatever the dead rows of an OWNED block hold (rows below n_pad, rows beyond L in the last tile): they must be finite -- the pool is zeroed at creation (fq3_api.hip) and recycled blocks hold finite bf16.
constexpr int kFaQ = 64, kFaK = 64, kFaKLd = kHeadDim + 8, kFaVLd = kFaK + 8, kFaPLd = kFaK + 8;

// One 64-key tile of the flash-style attention for ONE wave (16 queries): S = Q K^T, mask + online softmax on the accumulator layout, P
// (bf16 high part + residual) through the wave's private LDS region, O += P V.  Shared by flash_prefill_kernel (tiles streamed through one
// LDS stage) and flash_prefill_small_kernel (every tile resident): the same instructions on the same values in the same order.
__device__ __forceinline__ void flash_tile(const bf16_t* Ks, const bf16_t* Vt, bf16_t* ph, bf16_t* pl, const bf16x8_t (&qf)[4], f32x4_t (&o)[8],
                                           float (&m)[4], float (&l)[4], int tile, int q0, int wave, int fr, int fq, int n_pad, float sl2) {
        // ---- S = Q K^T: 4 key blocks of 16 ----
        f32x4_t sacc[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            sacc[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(&Ks[(nb * 16 + fr) * kFaKLd + ks * 32 + fq * 8]);
                sacc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[ks], kf, sacc[nb], 0, 0, 0);
            }
        }
        // ---- mask + online softmax (accumulator layout: column = key nb*16 + fr, row = query fq*4 + r) ----
        float p[4][4], alpha[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + wave * 16 + fq * 4 + r;
            float mx = -1e30f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int key = tile * kFaK + nb * 16 + fr;
                const bool ok = key <= qi && key >= n_pad;
                const float v = ok ? sacc[nb][r] * sl2 : -1e30f;
                p[nb][r] = v;
                mx = fmaxf(mx, v);
            }
            mx = row16_max(mx);
            const float mn = fmaxf(m[r], mx);
            alpha[r] = exp2f(m[r] - mn);
            float rs = 0.f;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const float e = p[nb][r] > -1e29f ? exp2f(p[nb][r] - mn) : 0.f;
                p[nb][r] = e;
                rs += e;
            }
            rs = row16_sum(rs);
            l[r] = l[r] * alpha[r] + rs;
            m[r] = mn;
        }
#pragma unroll
        for (int d = 0; d < 8; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[d][r] *= alpha[r];
        // ---- P -> LDS as bf16 high part + bf16 residual, [query][key] (this wave's private region) ----
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = p[nb][r];
                const bf16_t hi = f_to_bf16(v);
                ph[(fq * 4 + r) * kFaPLd + nb * 16 + fr] = hi;
                pl[(fq * 4 + r) * kFaPLd + nb * 16 + fr] = f_to_bf16(v - bf16_to_f(hi));
            }
        __builtin_amdgcn_s_waitcnt(0xc07f);                               // lgkmcnt(0): the wave's own LDS writes have landed
        __builtin_amdgcn_wave_barrier();
        // ---- O += P V: A = P [query fr][keys fq*8 + 32 ks], B = V^T [dim db*16 + fr][keys fq*8 + 32 ks] ----
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8_t pah = *reinterpret_cast<const bf16x8_t*>(&ph[fr * kFaPLd + ks * 32 + fq * 8]);
            const bf16x8_t pal = *reinterpret_cast<const bf16x8_t*>(&pl[fr * kFaPLd + ks * 32 + fq * 8]);
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(&Vt[(d * 16 + fr) * kFaVLd + ks * 32 + fq * 8]);
                o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pah, vf, o[d], 0, 0, 0);
                o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pal, vf, o[d], 0, 0, 0);
            }
        }
}

// fresh accumulators of a wave's 16 queries: O = 0, running row maximum m = -1e30 (base-2 units), running row sum l = 0
__device__ __forceinline__ void flash_acc_init(f32x4_t (&o)[8], float (&m)[4], float (&l)[4]) {
#pragma unroll
    for (int d = 0; d < 8; ++d) o[d] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -1e30f; l[r] = 0.f; }
}

// NW waves = 16 * NW queries per block (4: 64 queries, the short-prompt shape; 8: 128 queries -- a staged K/V tile feeds twice the
// MFMA work).  PAIRED: the workgroup handles query block bx and then block nqb - 1 - bx, so that under the causal mask every
// workgroup walks the same number of key tiles (nqb + 1) instead of 1 .. nqb of them: a 4096-token prompt at 128 queries per block
// is 16 pairs x 16 heads = 256 equal workgroups, one per CU.
template <int NW, bool PAIRED>
__global__ __launch_bounds__(64 * NW) void flash_prefill_kernel(const bf16_t* qkv, PagedKV<bf16_t> kv, bf16_t* out,
                                                                int L, int n_pad, int NH, int NKV, float scale, int nqb) {
    constexpr int HD = kHeadDim, Q = 16 * NW, CPT = 16 / NW;             // CPT: 16-byte chunks of a K (and V) row staged per thread
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kFaK * kFaKLd];            // [key][dim]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * kFaVLd];              // [dim][key]
    __shared__ __attribute__((aligned(16))) bf16_t Ps[NW][2][16 * kFaPLd];       // per wave: P high / residual, [query][key]
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, g = h / (NH / NKV), per = NH + 2 * NKV;
    // a key tile IS a block of the paged cache: tile t of kv head g = 64 contiguous rows at block table[t]
    const bf16_t* kc = kv.k + (size_t)g * kFaK * HD;
    const bf16_t* vc = kv.v + (size_t)g * kFaK * HD;
    const float sl2 = scale * 1.4426950408889634f;                        // softmax in base 2: exp(x) = exp2(x * log2 e)
    // staging: thread -> key (tid & 63), 16-byte chunks (tid >> 6) + NW j of that key's K and V rows
    const int skey = tid & 63, sch = tid >> 6;
    for (int pass = 0; pass < (PAIRED ? 2 : 1); ++pass) {
    const int qb = pass == 0 ? (int)blockIdx.x : nqb - 1 - (int)blockIdx.x;
    if (pass == 1 && qb <= (int)blockIdx.x) break;                        // odd block count: the middle block was pass 0
    const int q0 = qb * Q;
    if (q0 >= L) continue;
    // Q fragments of this wave's 16 rows (A operand: row = fr, dims fq*8 + 32*ks), kept in registers
    const int qrow = q0 + wave * 16 + fr;
    const int qrc = qrow < L ? qrow : L - 1;
    bf16x8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        qf[ks] = *reinterpret_cast<const bf16x8_t*>(qkv + (size_t)qrc * per * HD + (size_t)h * HD + ks * 32 + fq * 8);
    f32x4_t o[8];
    float m[4], l[4];
    flash_acc_init(o, m, l);
    const int q_hi = min(q0 + Q, L) - 1;                                  // last query of the block
    const int t_lo = n_pad / kFaK, t_hi = q_hi / kFaK;                    // key tiles [t_lo, t_hi]
    u32x4 kst[CPT], vst[CPT];
    auto issue = [&](int tile) {
        const size_t off = (size_t)kv.table[tile] * kv.blk_stride + (size_t)skey * HD;       // tile <= t_hi: a block this prompt owns
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            kst[j] = *reinterpret_cast<const u32x4*>(kc + off + (sch + NW * j) * 8);
            vst[j] = *reinterpret_cast<const u32x4*>(vc + off + (sch + NW * j) * 8);
        }
    };
    issue(t_lo);
    for (int tile = t_lo; tile <= t_hi; ++tile) {
        __syncthreads();                                                  // everyone is done reading the previous tile
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            *reinterpret_cast<u32x4*>(&Ks[skey * kFaKLd + (sch + NW * j) * 8]) = kst[j];
            // transposed store (dim-major image of V), two keys per 32-bit write: lanes 2i / 2i + 1 hold keys k / k + 1; they swap
            // words (DPP quad_perm [1,0,3,2]), the even lane writes the even dim of each pair for both keys, the odd lane the odd dim
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t mine = vst[j][w];
                const uint32_t other = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);
                const bool odd = skey & 1;
                const uint32_t word = odd ? ((other >> 16) | (mine & 0xFFFF0000u)) : ((mine & 0xFFFFu) | (other << 16));
                const int dim = (sch + NW * j) * 8 + 2 * w + (odd ? 1 : 0);
                *reinterpret_cast<uint32_t*>(&Vt[dim * kFaVLd + (skey & ~1)]) = word;
            }
        }
        __syncthreads();
        if (tile < t_hi) issue(tile + 1);                                 // next tile's loads fly under the MFMAs
        flash_tile(Ks, Vt, Ps[wave][0], Ps[wave][1], qf, o, m, l, tile, q0, wave, fr, fq, n_pad, sl2);
    }
    // ---- normalise, one rounding, store (left-padded query rows are zeros, like prefill_attn_kernel) ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + wave * 16 + fq * 4 + r;
        if (qi >= L) continue;
        const float inv = (qi >= n_pad && l[r] > 0.f) ? 1.0f / l[r] : 0.f;
#pragma unroll
        for (int d = 0; d < 8; ++d) out[((size_t)qi * NH + h) * HD + d * 16 + fr] = f_to_bf16(o[d][r] * inv);
    }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Short prompts (round 5): every sequence has at most 256 rows = four key tiles, and ALL of a query block's key tiles fit the LDS at
// once (4 x (K 17 KB + V^T 18 KB) + the waves' P regions = 158 KB).  flash_prefill_kernel walks the tiles one after the other through a
// single stage -- global loads, two workgroup barriers and the tile's arithmetic in series per tile: 14.8 us per layer at 200 rows
// (profiles/r03_prefill200_kernel_trace.txt), a four-deep latency chain.  Here the tiles are staged back to back (two register sets,
// the loads of tile i + 1 in flight while tile i is written; unconditional, clamped), ONE barrier, then every wave walks the resident
// tiles on its own (flash_tile: the same instructions in the same order, so the output is bit-identical to flash_prefill_kernel).
// The sequences of a PACKED prefill (fq3_prefill_batch) share the launch: blockIdx.z = sequence, its rows / pad / block table from a
// by-value table -- one launch per layer instead of one per prompt and layer (280 launches per 10-prompt group before).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kMaxPack = 64;                        // fq3_prefill_batch takes at most 64 prompts
constexpr int kFsTiles = 4, kFsMaxRows = kFsTiles * kFaK;
struct PackSeq {
    const int* table[kMaxPack];                     // block table of each sequence's context (all of ONE pool)
    int off[kMaxPack + 1];                          // first packed row of each sequence
    int n_pad[kMaxPack];
    int rope_delta[kMaxPack];
    int n;
};
constexpr size_t kFsLdsBytes = (size_t)kFsTiles * (kFaK * kFaKLd + kHeadDim * kFaVLd) * 2 + (size_t)4 * 2 * 16 * kFaPLd * 2;

__global__ __launch_bounds__(256) void flash_prefill_small_kernel(const bf16_t* qkv_all, PagedKV<bf16_t> kv, bf16_t* out_all, PackSeq sq,
                                                                  int NH, int NKV, float scale) {
    constexpr int HD = kHeadDim, NW = 4, Q = 64, CPT = 16 / NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];
    bf16_t* KsAll = reinterpret_cast<bf16_t*>(fs_smem);                                   // [tile][key][dim]
    bf16_t* VtAll = KsAll + (size_t)kFsTiles * kFaK * kFaKLd;                               // [tile][dim][key]
    bf16_t* PsAll = VtAll + (size_t)kFsTiles * HD * kFaVLd;                                 // [wave][hi | lo][query][key]
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sqi = blockIdx.z;
    const int off = sq.off[sqi], L = sq.off[sqi + 1] - off, n_pad = sq.n_pad[sqi];
    const int q0 = (int)blockIdx.x * Q;
    if (q0 >= L) return;
    const int* table = sq.table[sqi];
    const int h = blockIdx.y, g = h / (NH / NKV), per = NH + 2 * NKV;
    const bf16_t* qkv = qkv_all + (size_t)off * per * HD;
    bf16_t* out = out_all + (size_t)off * NH * HD;
    const bf16_t* kc = kv.k + (size_t)g * kFaK * HD;
    const bf16_t* vc = kv.v + (size_t)g * kFaK * HD;
    const float sl2 = scale * 1.4426950408889634f;
    const int skey = tid & 63, sch = tid >> 6;
    const int qrow = q0 + wave * 16 + fr;
    const int qrc = qrow < L ? qrow : L - 1;
    bf16x8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        qf[ks] = *reinterpret_cast<const bf16x8_t*>(qkv + (size_t)qrc * per * HD + (size_t)h * HD + ks * 32 + fq * 8);
    const int q_hi = min(q0 + Q, L) - 1;
    const int t_lo = n_pad / kFaK, t_hi = q_hi / kFaK;                    // key tiles [t_lo, t_hi]: at most kFsTiles of them
    // ---- stage every tile (slot i = tile t_lo + i; slots past t_hi repeat tile t_hi and are never read) ----
    u32x4 kst[2][CPT], vst[2][CPT];
    auto issue = [&](u32x4 (&kr)[CPT], u32x4 (&vr)[CPT], int i) {
        const int tile = t_lo + i < t_hi ? t_lo + i : t_hi;
        const size_t o_ = (size_t)table[tile] * kv.blk_stride + (size_t)skey * HD;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            kr[j] = *reinterpret_cast<const u32x4*>(kc + o_ + (sch + NW * j) * 8);
            vr[j] = *reinterpret_cast<const u32x4*>(vc + o_ + (sch + NW * j) * 8);
        }
    };
    auto stage = [&](const u32x4 (&kr)[CPT], const u32x4 (&vr)[CPT], int i) {
        bf16_t* Ks = KsAll + (size_t)i * kFaK * kFaKLd;
        bf16_t* Vt = VtAll + (size_t)i * HD * kFaVLd;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            *reinterpret_cast<u32x4*>(&Ks[skey * kFaKLd + (sch + NW * j) * 8]) = kr[j];
            // transposed store, two keys per 32-bit write (see flash_prefill_kernel)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t mine = vr[j][w];
                const uint32_t other = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);
                const bool odd = skey & 1;
                const uint32_t word = odd ? ((other >> 16) | (mine & 0xFFFF0000u)) : ((mine & 0xFFFFu) | (other << 16));
                const int dim = (sch + NW * j) * 8 + 2 * w + (odd ? 1 : 0);
                *reinterpret_cast<uint32_t*>(&Vt[dim * kFaVLd + (skey & ~1)]) = word;
            }
        }
    };
    issue(kst[0], vst[0], 0);
    issue(kst[1], vst[1], 1);
    stage(kst[0], vst[0], 0);
    issue(kst[0], vst[0], 2);
    stage(kst[1], vst[1], 1);
    issue(kst[1], vst[1], 3);
    stage(kst[0], vst[0], 2);
    stage(kst[1], vst[1], 3);
    __syncthreads();
    f32x4_t o[8];
    float m[4], l[4];
    flash_acc_init(o, m, l);
    bf16_t* ph = PsAll + (size_t)(wave * 2 + 0) * 16 * kFaPLd;
    bf16_t* pl = PsAll + (size_t)(wave * 2 + 1) * 16 * kFaPLd;
    for (int tile = t_lo; tile <= t_hi; ++tile) {
        const int i = tile - t_lo;
        flash_tile(KsAll + (size_t)i * kFaK * kFaKLd, VtAll + (size_t)i * HD * kFaVLd, ph, pl, qf, o, m, l, tile, q0, wave, fr, fq, n_pad, sl2);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + wave * 16 + fq * 4 + r;
        if (qi >= L) continue;
        const float inv = (qi >= n_pad && l[r] > 0.f) ? 1.0f / l[r] : 0.f;
#pragma unroll
        for (int d = 0; d < 8; ++d) out[((size_t)qi * NH + h) * HD + d * 16 + fr] = f_to_bf16(o[d][r] * inv);
    }
}

// q / k head-norm + RoPE + K / V write for the packed rows of several sequences in one launch (see qk_norm_rope_kv_kernel)
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_pack_kernel(T* qkv, const T* qw, const T* kw, float eps, const float* cos_tab,
                                                                   const float* sin_tab, int rope_len, PagedKV<T> kvp, PackSeq sq, int NH, int NKV) {
    constexpr int HD = kHeadDim;
    const int per = NH + 2 * NKV;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int Lt = sq.off[sq.n];
    if (w >= Lt * per) return;
    const int tg = w / per, v = w - tg * per;
    int qi = 0;                                          // the sequence of packed row tg (uniform per wave: scalar compares)
    for (int q = 1; q < sq.n; ++q) qi = tg >= sq.off[q] ? q : qi;
    const int t = tg - sq.off[qi];
    if (t < sq.n_pad[qi]) return;
    PagedKV<T> kv = kvp;
    kv.table = sq.table[qi];
    T* src = qkv + (size_t)tg * per * HD + (size_t)v * HD;
    float x0 = DT<T>::ld(src + lane), x1 = DT<T>::ld(src + lane + 64);
    if (v < NH + NKV) {
        const T* gw = v < NH ? qw : kw;
        const float ss = wave_sum(fmaf(x0, x0, x1 * x1));
        const float rs = 1.0f / sqrtf(ss / (float)HD + eps);
        const float n0 = DT<T>::rnd(DT<T>::ld(gw + lane) * DT<T>::rnd(x0 * rs));
        const float n1 = DT<T>::rnd(DT<T>::ld(gw + lane + 64) * DT<T>::rnd(x1 * rs));
        int rp = t + sq.rope_delta[qi];
        rp = rp < 0 ? 0 : (rp >= rope_len ? rope_len - 1 : rp);
        const float cs = cos_tab[(size_t)rp * 64 + lane], sn = sin_tab[(size_t)rp * 64 + lane];
        x0 = DT<T>::rnd(DT<T>::rnd(n0 * cs) + DT<T>::rnd(-n1 * sn));
        x1 = DT<T>::rnd(DT<T>::rnd(n1 * cs) + DT<T>::rnd(n0 * sn));
    }
    T* dst = v < NH ? src : (v < NH + NKV ? kv.k + paged_row(kv, v - NH, t) : kv.v + paged_row(kv, v - NH - NKV, t));
    DT<T>::st(dst + lane, x0);
    DT<T>::st(dst + lane + 64, x1);
}

// ---------------------------------------------------------------------------------------------------------------------
// Continuation prefill (fq3_prefill_continue): rows [start, start + n) of a prompt whose K/V rows [0, start) are already in the paged
// cache.  qkv / out hold the n NEW rows only (local row t = position start + t); no left padding.
// ---------------------------------------------------------------------------------------------------------------------

// qk_norm_rope_kv_kernel with a position base: local row t is normalised and rotated at RoPE row clamp(start + t + rope_delta), q in
// place at local row t, K / V to cache row start + t.  Cache rows below start are not touched.
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_cont_kernel(T* qkv, const T* qw, const T* kw, float eps, const float* cos_tab,
                                                                   const float* sin_tab, int rope_len, int rope_delta, PagedKV<T> kv,
                                                                   int start, int n, int NH, int NKV) {
    constexpr int HD = kHeadDim;
    const int per = NH + 2 * NKV;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n * per) return;
    const int t = w / per, v = w - t * per, pos = start + t;
    T* src = qkv + (size_t)t * per * HD + (size_t)v * HD;
    float x0 = DT<T>::ld(src + lane), x1 = DT<T>::ld(src + lane + 64);
    if (v < NH + NKV) {
        const T* gw = v < NH ? qw : kw;
        const float ss = wave_sum(fmaf(x0, x0, x1 * x1));
        const float rs = 1.0f / sqrtf(ss / (float)HD + eps);
        const float n0 = DT<T>::rnd(DT<T>::ld(gw + lane) * DT<T>::rnd(x0 * rs));
        const float n1 = DT<T>::rnd(DT<T>::ld(gw + lane + 64) * DT<T>::rnd(x1 * rs));
        int rp = pos + rope_delta;
        rp = rp < 0 ? 0 : (rp >= rope_len ? rope_len - 1 : rp);
        const float cs = cos_tab[(size_t)rp * 64 + lane], sn = sin_tab[(size_t)rp * 64 + lane];
        x0 = DT<T>::rnd(DT<T>::rnd(n0 * cs) + DT<T>::rnd(-n1 * sn));
        x1 = DT<T>::rnd(DT<T>::rnd(n1 * cs) + DT<T>::rnd(n0 * sn));
    }
    T* dst = v < NH ? src : (v < NH + NKV ? kv.k + paged_row(kv, v - NH, pos) : kv.v + paged_row(kv, v - NH - NKV, pos));
    DT<T>::st(dst + lane, x0);
    DT<T>::st(dst + lane + 64, x1);
}

// prefill_attn_kernel with a query base: one wave per (new row, q head); local row t attends to keys 0 .. start + t with the loop of
// prefill_attn_kernel (16 lanes per key, 16 keys per trip, fp32 online softmax, one rounding at the end).
template <typename T>
__global__ __launch_bounds__(256) void prefill_attn_cont_kernel(const T* qkv, PagedKV<T> kv, T* out, int start, int n, int NH, int NKV,
                                                                float scale) {
    constexpr int HD = kHeadDim;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n * NH) return;
    const int t = w / NH, h = w - t * NH, last = start + t;               // last: the row's own key
    const int per = NH + 2 * NKV, g = h / (NH / NKV);
    const int sub = lane >> 4, c = lane & 15;
    T* op = out + ((size_t)t * NH + h) * HD;
    Raw8<T> qraw;
    ldraw<false>(qraw, qkv + (size_t)t * per * HD + (size_t)h * HD + c * 8);
    float q[8];
    unpack(qraw, q);
    float m = -1e30f, l = 0.f, o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = 0.f;
    for (int k0 = 0; k0 <= last; k0 += 16) {
        Raw8<T> kr[4], vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int key = k0 + i * 4 + sub;
            key = key <= last ? key : last;
            const size_t off = paged_row(kv, g, key) + c * 8;
            ldraw<false>(kr[i], kv.k + off);
            ldraw<false>(vr[i], kv.v + off);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool valid = k0 + i * 4 + sub <= last;
            float kf[8], vf[8];
            unpack(kr[i], kf); unpack(vr[i], vf);
            float sc = 0.f;
#pragma unroll
            for (int d = 0; d < 8; ++d) sc = fmaf(q[d], kf[d], sc);
            sc += __shfl_xor(sc, 1, 64); sc += __shfl_xor(sc, 2, 64);
            sc += __shfl_xor(sc, 4, 64); sc += __shfl_xor(sc, 8, 64);
            sc = valid ? sc * scale : -INFINITY;
            const float mn = fmaxf(m, sc), al = __expf(m - mn), p = __expf(sc - mn);
            l = fmaf(l, al, p);
#pragma unroll
            for (int d = 0; d < 8; ++d) o[d] = fmaf(o[d], al, valid ? p * vf[d] : 0.f);
            m = mn;
        }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(l, off, 64);
        const float M = fmaxf(m, mo), wa = __expf(m - M), wb = __expf(mo - M);
        l = l * wa + lo * wb;
#pragma unroll
        for (int d = 0; d < 8; ++d) { const float oo = __shfl_xor(o[d], off, 64); o[d] = o[d] * wa + oo * wb; }
        m = M;
    }
    if (sub == 0)
#pragma unroll
        for (int i = 0; i < 8; ++i) DT<T>::st(op + c * 8 + i, o[i] / l);
}

// Continuation flash kernel (bf16).  One workgroup = one q head x 64 NEW queries (4 waves) x one KEY SPLIT: a continuation has few
// query blocks and many key tiles (128 new rows behind 3968 cached keys: 2 blocks x 16 heads, 64 tiles each), so the key tiles
// [0, nt) of a query block (nt = tiles up to its last query's own key) are cut into S contiguous ranges of ceil(nt / S) tiles, one per
// blockIdx.z.  A tile is found by its ABSOLUTE index through the block table and streamed through the LDS stage of
// flash_prefill_kernel; flash_tile gets the absolute query position, so a tile's arithmetic is that of the whole prefill.
// S == 1: normalise, round once, write `out`.  S > 1: each split writes its un-normalised fp32 (m, l, o[128]) per (row, head) to
// `ws` ([split][row][head][kFcRec]) with plain stores and flash_cont_merge_kernel -- a SECOND launch; no counters, flags or spins --
// merges them in split order and rounds once.  A split with no tile (nt < S ranges) stores (m = -1e30, l = 0, o = 0): weight 0.
// S is fixed by the launcher per (start, n): the same call gives the same bits.
// CONTRACT (as flash_prefill_kernel): P = 0 is multiplied by whatever the dead rows of an OWNED block hold (rows past start + n in the
// last tile): every block a context owns must be finite -- the pool is zeroed at creation, recycled blocks hold finite bf16, and
// fq3_kv_copy copies WHOLE blocks, dead rows included.
constexpr int kFcRec = 2 + kHeadDim;               // floats per (split, row, head) record: m, l, o[128]
__global__ __launch_bounds__(256) void flash_prefill_cont_kernel(const bf16_t* qkv, PagedKV<bf16_t> kv, bf16_t* out, float* ws,
                                                                 int start, int n, int NH, int NKV, float scale, int S) {
    constexpr int HD = kHeadDim, NW = 4, Q = 16 * NW, CPT = 16 / NW;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kFaK * kFaKLd];            // [key][dim]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * kFaVLd];              // [dim][key]
    __shared__ __attribute__((aligned(16))) bf16_t Ps[NW][2][16 * kFaPLd];       // per wave: P high / residual, [query][key]
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, g = h / (NH / NKV), per = NH + 2 * NKV, z = blockIdx.z;
    const bf16_t* kc = kv.k + (size_t)g * kFaK * HD;
    const bf16_t* vc = kv.v + (size_t)g * kFaK * HD;
    const float sl2 = scale * 1.4426950408889634f;
    const int skey = tid & 63, sch = tid >> 6;
    const int q0 = (int)blockIdx.x * Q;                                   // first LOCAL row of the block (grid.x covers n)
    const int qrow = q0 + wave * 16 + fr;
    const int qrc = qrow < n ? qrow : n - 1;
    bf16x8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        qf[ks] = *reinterpret_cast<const bf16x8_t*>(qkv + (size_t)qrc * per * HD + (size_t)h * HD + ks * 32 + fq * 8);
    f32x4_t o[8];
    float m[4], l[4];
    flash_acc_init(o, m, l);
    const int nt = (start + min(q0 + Q, n) - 1) / kFaK + 1;               // key tiles [0, nt): up to the block's last query's own key
    const int tps = (nt + S - 1) / S;
    const int t_lo = z * tps, t_end = min(nt, t_lo + tps);                // this split: tiles [t_lo, t_end), maybe none
    u32x4 kst[CPT], vst[CPT];
    auto issue = [&](int tile) {
        const size_t off = (size_t)kv.table[tile] * kv.blk_stride + (size_t)skey * HD;       // tile < nt: a block this context owns
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            kst[j] = *reinterpret_cast<const u32x4*>(kc + off + (sch + NW * j) * 8);
            vst[j] = *reinterpret_cast<const u32x4*>(vc + off + (sch + NW * j) * 8);
        }
    };
    if (t_lo < t_end) issue(t_lo);
    for (int tile = t_lo; tile < t_end; ++tile) {
        __syncthreads();                                                  // everyone is done reading the previous tile
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            *reinterpret_cast<u32x4*>(&Ks[skey * kFaKLd + (sch + NW * j) * 8]) = kst[j];
            // transposed store, two keys per 32-bit write (see flash_prefill_kernel)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t mine = vst[j][w];
                const uint32_t other = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);
                const bool odd = skey & 1;
                const uint32_t word = odd ? ((other >> 16) | (mine & 0xFFFF0000u)) : ((mine & 0xFFFFu) | (other << 16));
                const int dim = (sch + NW * j) * 8 + 2 * w + (odd ? 1 : 0);
                *reinterpret_cast<uint32_t*>(&Vt[dim * kFaVLd + (skey & ~1)]) = word;
            }
        }
        __syncthreads();
        if (tile + 1 < t_end) issue(tile + 1);                            // next tile's loads fly under the MFMAs
        flash_tile(Ks, Vt, Ps[wave][0], Ps[wave][1], qf, o, m, l, tile, start + q0, wave, fr, fq, 0, sl2);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + wave * 16 + fq * 4 + r;                       // local row
        if (qi >= n) continue;
        if (S == 1) {
            const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
#pragma unroll
            for (int d = 0; d < 8; ++d) out[((size_t)qi * NH + h) * HD + d * 16 + fr] = f_to_bf16(o[d][r] * inv);
        } else {
            float* rec = ws + (((size_t)z * n + qi) * NH + h) * kFcRec;
            if (fr == 0) { rec[0] = m[r]; rec[1] = l[r]; }
#pragma unroll
            for (int d = 0; d < 8; ++d) rec[2 + d * 16 + fr] = o[d][r];
        }
    }
}

// merge of the key splits of flash_prefill_cont_kernel: one thread per (row, head, dim); M = max of the splits' m (base-2 units),
// then l and o accumulated in split order with weights 2^(m_s - M), one division, one rounding to bf16.
__global__ __launch_bounds__(256) void flash_cont_merge_kernel(const float* ws, bf16_t* out, int n, int NH, int S) {
    const int i = blockIdx.x * 2 + (threadIdx.x >> 7), d = threadIdx.x & 127;          // i = row * NH + head
    if (i >= n * NH) return;
    const size_t split = (size_t)n * NH * kFcRec;
    const float* rec = ws + (size_t)i * kFcRec;
    float M = -1e30f;
    for (int s = 0; s < S; ++s) M = fmaxf(M, rec[s * split]);
    float l = 0.f, o = 0.f;
    for (int s = 0; s < S; ++s) {
        const float w = exp2f(rec[s * split] - M);
        l = fmaf(rec[s * split + 1], w, l);
        o = fmaf(rec[s * split + 2 + d], w, o);
    }
    out[(size_t)i * kHeadDim + d] = f_to_bf16(l > 0.f ? o / l : 0.f);
}

constexpr int kFcMinTiles = 4, kFcMaxSplit = 16;       // key-split rule (flash_cont_pack_splits below): tiles per split at least, splits at most

// ---------------------------------------------------------------------------------------------------------------------
// Packed continuation prefill (fq3_prefill_continue_batch): n sequences, each with cnt[q] NEW rows behind its own cached rows
// [0, start[q]), share the launches of a layer the way the sequences of fq3_prefill_batch do (PackSeq).  qkv / out hold the packed new
// rows: sequence q's local row t is packed row off[q] + t = position start[q] + t of that sequence.
// ---------------------------------------------------------------------------------------------------------------------
struct PackCont {
    const int* table[kMaxPack];                     // block table of each sequence's context (all of ONE pool)
    int off[kMaxPack + 1];                          // first packed row of each sequence
    int start[kMaxPack];                            // cached rows in front of each sequence's new rows
    int rope_delta[kMaxPack];
    int zoff[kMaxPack + 1];                         // prefix sum of the key splits S[q]: the (sequence, split) axis of the flash grid
    int wsoff[kMaxPack];                            // first float of each sequence's split records ([split][row][head][kFcRec]; S[q] > 1 only)
    int n;
};

// qk_norm_rope_kv_cont_kernel for the pack: the sequence of a packed row by scalar compares (uniform per wave, as
// qk_norm_rope_kv_pack_kernel), position start[q] + t, K / V through that sequence's table.  zoff / wsoff are not read.
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_cont_pack_kernel(T* qkv, const T* qw, const T* kw, float eps, const float* cos_tab,
                                                                        const float* sin_tab, int rope_len, PagedKV<T> kvp, PackCont sq,
                                                                        int NH, int NKV) {
    constexpr int HD = kHeadDim;
    const int per = NH + 2 * NKV;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int Lt = sq.off[sq.n];
    if (w >= Lt * per) return;
    const int tg = w / per, v = w - tg * per;
    int qi = 0;                                          // the sequence of packed row tg (uniform per wave: scalar compares)
    for (int q = 1; q < sq.n; ++q) qi = tg >= sq.off[q] ? q : qi;
    const int pos = sq.start[qi] + (tg - sq.off[qi]);
    PagedKV<T> kv = kvp;
    kv.table = sq.table[qi];
    T* src = qkv + (size_t)tg * per * HD + (size_t)v * HD;
    float x0 = DT<T>::ld(src + lane), x1 = DT<T>::ld(src + lane + 64);
    if (v < NH + NKV) {
        const T* gw = v < NH ? qw : kw;
        const float ss = wave_sum(fmaf(x0, x0, x1 * x1));
        const float rs = 1.0f / sqrtf(ss / (float)HD + eps);
        const float n0 = DT<T>::rnd(DT<T>::ld(gw + lane) * DT<T>::rnd(x0 * rs));
        const float n1 = DT<T>::rnd(DT<T>::ld(gw + lane + 64) * DT<T>::rnd(x1 * rs));
        int rp = pos + sq.rope_delta[qi];
        rp = rp < 0 ? 0 : (rp >= rope_len ? rope_len - 1 : rp);
        const float cs = cos_tab[(size_t)rp * 64 + lane], sn = sin_tab[(size_t)rp * 64 + lane];
        x0 = DT<T>::rnd(DT<T>::rnd(n0 * cs) + DT<T>::rnd(-n1 * sn));
        x1 = DT<T>::rnd(DT<T>::rnd(n1 * cs) + DT<T>::rnd(n0 * sn));
    }
    T* dst = v < NH ? src : (v < NH + NKV ? kv.k + paged_row(kv, v - NH, pos) : kv.v + paged_row(kv, v - NH - NKV, pos));
    DT<T>::st(dst + lane, x0);
    DT<T>::st(dst + lane + 64, x1);
}

// flash_prefill_cont_kernel for the pack (bf16, one pool).  Grid (max query blocks of a sequence, NH, sum of S[q]): blockIdx.z is a
// (sequence, split) pair found in the prefix sum zoff by scalar compares; a workgroup whose query block lies beyond its sequence
// returns at once (as flash_prefill_small_kernel).  From there on it is flash_prefill_cont_kernel on that sequence's slice: the same
// LDS stage, the same tile ranges, flash_tile with the absolute query position -- so a (sequence, split) does that kernel's
// arithmetic in that kernel's order.  S[q] == 1 writes `out`; S[q] > 1 stores the fp32 records at ws + wsoff[q] with plain stores for
// flash_cont_pack_merge_kernel.  No atomics, counters or spins.  The dead-rows CONTRACT of flash_prefill_cont_kernel holds.
__global__ __launch_bounds__(256) void flash_prefill_cont_pack_kernel(const bf16_t* qkv_all, PagedKV<bf16_t> kv, bf16_t* out_all, float* ws_all,
                                                                      PackCont sq, int NH, int NKV, float scale) {
    constexpr int HD = kHeadDim, NW = 4, Q = 16 * NW, CPT = 16 / NW;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[kFaK * kFaKLd];            // [key][dim]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * kFaVLd];              // [dim][key]
    __shared__ __attribute__((aligned(16))) bf16_t Ps[NW][2][16 * kFaPLd];       // per wave: P high / residual, [query][key]
    const int zz = blockIdx.z;
    int sqi = 0;                                                          // uniform per workgroup: scalar compares
    for (int q = 1; q < sq.n; ++q) sqi = zz >= sq.zoff[q] ? q : sqi;
    const int off = sq.off[sqi], n = sq.off[sqi + 1] - off, start = sq.start[sqi];
    const int z = zz - sq.zoff[sqi], S = sq.zoff[sqi + 1] - sq.zoff[sqi];
    const int q0 = (int)blockIdx.x * Q;                                   // first LOCAL row of the block
    if (q0 >= n) return;
    const int* table = sq.table[sqi];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, g = h / (NH / NKV), per = NH + 2 * NKV;
    const bf16_t* qkv = qkv_all + (size_t)off * per * HD;
    bf16_t* out = out_all + (size_t)off * NH * HD;
    float* ws = ws_all + sq.wsoff[sqi];
    const bf16_t* kc = kv.k + (size_t)g * kFaK * HD;
    const bf16_t* vc = kv.v + (size_t)g * kFaK * HD;
    const float sl2 = scale * 1.4426950408889634f;
    const int skey = tid & 63, sch = tid >> 6;
    const int qrow = q0 + wave * 16 + fr;
    const int qrc = qrow < n ? qrow : n - 1;
    bf16x8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        qf[ks] = *reinterpret_cast<const bf16x8_t*>(qkv + (size_t)qrc * per * HD + (size_t)h * HD + ks * 32 + fq * 8);
    f32x4_t o[8];
    float m[4], l[4];
    flash_acc_init(o, m, l);
    const int nt = (start + min(q0 + Q, n) - 1) / kFaK + 1;               // key tiles [0, nt): up to the block's last query's own key
    const int tps = (nt + S - 1) / S;
    const int t_lo = z * tps, t_end = min(nt, t_lo + tps);                // this split: tiles [t_lo, t_end), maybe none
    u32x4 kst[CPT], vst[CPT];
    auto issue = [&](int tile) {
        const size_t o_ = (size_t)table[tile] * kv.blk_stride + (size_t)skey * HD;          // tile < nt: a block this sequence owns
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            kst[j] = *reinterpret_cast<const u32x4*>(kc + o_ + (sch + NW * j) * 8);
            vst[j] = *reinterpret_cast<const u32x4*>(vc + o_ + (sch + NW * j) * 8);
        }
    };
    if (t_lo < t_end) issue(t_lo);
    for (int tile = t_lo; tile < t_end; ++tile) {
        __syncthreads();                                                  // everyone is done reading the previous tile
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            *reinterpret_cast<u32x4*>(&Ks[skey * kFaKLd + (sch + NW * j) * 8]) = kst[j];
            // transposed store, two keys per 32-bit write (see flash_prefill_kernel)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t mine = vst[j][w];
                const uint32_t other = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);
                const bool odd = skey & 1;
                const uint32_t word = odd ? ((other >> 16) | (mine & 0xFFFF0000u)) : ((mine & 0xFFFFu) | (other << 16));
                const int dim = (sch + NW * j) * 8 + 2 * w + (odd ? 1 : 0);
                *reinterpret_cast<uint32_t*>(&Vt[dim * kFaVLd + (skey & ~1)]) = word;
            }
        }
        __syncthreads();
        if (tile + 1 < t_end) issue(tile + 1);                            // next tile's loads fly under the MFMAs
        flash_tile(Ks, Vt, Ps[wave][0], Ps[wave][1], qf, o, m, l, tile, start + q0, wave, fr, fq, 0, sl2);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + wave * 16 + fq * 4 + r;                       // local row
        if (qi >= n) continue;
        if (S == 1) {
            const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
#pragma unroll
            for (int d = 0; d < 8; ++d) out[((size_t)qi * NH + h) * HD + d * 16 + fr] = f_to_bf16(o[d][r] * inv);
        } else {
            float* rec = ws + (((size_t)z * n + qi) * NH + h) * kFcRec;
            if (fr == 0) { rec[0] = m[r]; rec[1] = l[r]; }
#pragma unroll
            for (int d = 0; d < 8; ++d) rec[2 + d * 16 + fr] = o[d][r];
        }
    }
}

// flash_cont_merge_kernel for the pack: one thread per (packed row, head, dim); rows of a sequence with S[q] == 1 were written by the
// flash kernel and are left alone; the others merge their S[q] records in split order with that kernel's arithmetic.
__global__ __launch_bounds__(256) void flash_cont_pack_merge_kernel(const float* ws_all, bf16_t* out, PackCont sq, int NH) {
    const int i = blockIdx.x * 2 + (threadIdx.x >> 7), d = threadIdx.x & 127;          // i = packed row * NH + head
    const int Lt = sq.off[sq.n];
    if (i >= Lt * NH) return;
    const int tg = i / NH;
    int qi = 0;                                                           // uniform per wave (a wave holds one i)
    for (int q = 1; q < sq.n; ++q) qi = tg >= sq.off[q] ? q : qi;
    const int S = sq.zoff[qi + 1] - sq.zoff[qi];
    if (S == 1) return;
    const int n = sq.off[qi + 1] - sq.off[qi];
    const size_t split = (size_t)n * NH * kFcRec;
    const float* rec = ws_all + sq.wsoff[qi] + (size_t)(i - sq.off[qi] * NH) * kFcRec;
    float M = -1e30f;
    for (int s = 0; s < S; ++s) M = fmaxf(M, rec[s * split]);
    float l = 0.f, o = 0.f;
    for (int s = 0; s < S; ++s) {
        const float w = exp2f(rec[s * split] - M);
        l = fmaf(rec[s * split + 1], w, l);
        o = fmaf(rec[s * split + 2 + d], w, o);
    }
    out[(size_t)i * kHeadDim + d] = f_to_bf16(l > 0.f ? o / l : 0.f);
}

// floats of split records a pack with these S[] stores (sequences with S == 1 store none)
inline long flash_cont_pack_ws_floats(const int* cnt, int n, int NH, const int* S) {
    long t = 0;
    for (int q = 0; q < n; ++q) t += S[q] > 1 ? (long)S[q] * cnt[q] * NH * kFcRec : 0;
    return t;
}

// key splits of a packed continuation, a pure function of (start[], cnt[]) and the CU count: blocks x heads x S about half to one times
// the CU count -- the CU budget is divided by the pack's total query blocks x heads (whole multiples, rounded down); per sequence at
// least kFcMinTiles key tiles per split and at most kFcMaxSplit; while the records of the whole pack exceed the workspace the largest S
// (the first of equals) loses one.
inline void flash_cont_pack_splits(const int* start, const int* cnt, int n, int NH, int n_cu, long ws_floats, int* S) {
    long nqb = 0;
    for (int q = 0; q < n; ++q) nqb += (cnt[q] + kFaQ - 1) / kFaQ;
    const int budget = (int)(n_cu / (nqb * NH));
    for (int q = 0; q < n; ++q) {
        const int nt = (start[q] + cnt[q] + kFaK - 1) / kFaK;
        int s = budget < nt / kFcMinTiles ? budget : nt / kFcMinTiles;
        s = s < kFcMaxSplit ? s : kFcMaxSplit;
        S[q] = s < 1 ? 1 : s;
    }
    while (flash_cont_pack_ws_floats(cnt, n, NH, S) > ws_floats) {
        int big = 0;
        for (int q = 1; q < n; ++q) big = S[q] > S[big] ? q : big;
        --S[big];                                        // > 1 here: records exist only where S > 1
    }
}

// the key splits of one prompt's continuation: the pack of one
inline int flash_cont_splits(int start, int n, int NH, int n_cu, long ws_floats) {
    int S;
    flash_cont_pack_splits(&start, &n, 1, NH, n_cu, ws_floats, &S);
    return S;
}

// RMSNorm of prompt rows, one wave per row, the whole row in registers: 16-byte loads, one reduction, 16-byte stores (the row-loop
// kernel the codec uses takes 10 us on 200 rows of 1024: 32 dependent 2-byte accesses per lane).  Per element the arithmetic is
// the same -- w * rnd(x * rs), rounded on store; only the order of the sum of squares differs.  C = NCH * 512.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void rmsnorm_rows_vec_kernel(const T* x, const T* w, T* y, int rows, float eps) {
    constexpr int C = NCH * 512;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    Raw8<T> xr[NCH], wr[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        ldraw<false>(xr[j], x + (size_t)row * C + j * 512 + lane * 8);
        ldraw<false>(wr[j], w + j * 512 + lane * 8);
    }
    float xv[NCH][8], ss = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        unpack(xr[j], xv[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) ss = fmaf(xv[j][i], xv[j][i], ss);
    }
    ss = wave_sum(ss);
    const float rs = 1.0f / sqrtf(ss / (float)C + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        float wv[8];
        unpack(wr[j], wv);
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[j][i] = wv[i] * DT<T>::rnd(xv[j][i] * rs);
        DT<T>::st8(y + (size_t)row * C + j * 512 + lane * 8, xv[j]);
    }
}
template <typename T>
void rmsnorm_rows(const T* x, const T* w, T* y, int rows, int C, float eps, hipStream_t s) {
    const dim3 grid((rows + 3) / 4), block(256);
    if (C == 1024) hipLaunchKernelGGL((rmsnorm_rows_vec_kernel<T, 2>), grid, block, 0, s, x, w, y, rows, eps);
    else if (C == 2048) hipLaunchKernelGGL((rmsnorm_rows_vec_kernel<T, 4>), grid, block, 0, s, x, w, y, rows, eps);
    else hipLaunchKernelGGL((rmsnorm_rows_kernel<T>), grid, block, 0, s, x, w, y, 0, rows, C, eps);
}

}  // namespace fq3
