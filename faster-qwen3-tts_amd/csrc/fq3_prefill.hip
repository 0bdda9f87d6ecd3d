// Matrix-core prefill of the talker (replaces the upstream eager `talker.forward(inputs_embeds=...)`,
// faster_qwen3_tts/generate.py:107-122): all prompt rows go through each layer as GEMMs
// on MFMA (conv_gemm_kernel with one tap), K/V are normalised, rotated and written straight into the
// static cache layout the decode kernels read, attention is causal over the live (non-padded) keys.
// Rounding points are those of the decode path (one rounding to T per Linear / norm / RoPE / residual add),
// so prefill + decode match the oracle's matrix-form prefill.
// Map: prefill_begin (checks, workspace, packed copy) and prefill_layers (per layer norm / qkv GEMM / attention step / o-proj, norm,
// SwiGLU, down, then the final norm and head) are the one skeleton.  The attention step comes from the entry point's family:
// prefill_batch_t (fq3_prefill, fq3_prefill_batch) runs pack_attention_layer or prompt_attention per prompt;
// prefill_continue_batch_t (fq3_prefill_continue, fq3_prefill_continue_batch) runs pack_cont_attention_layer or prompt_attention_cont
// per prompt.  The single-prompt entry points are the batch forms of one.
#define FQ3_SKINNY_DEFINE           // skinny_gemm.cuh: the weight-stationary GEMM kernels are instantiated in fq3_prefill.hip only
#include "fq3_ctx.h"
#include <vector>
#include "prefill_kernels.cuh"

using namespace fq3;

namespace {

// One layer of a context's paged talker cache as the kernels take it (PagedKV: prefill_kernels.cuh)
template <typename T> PagedKV<T> paged_kv(const fq3_ctx* c, int layer) {
    return PagedKV<T>{(T*)c->tk.k[layer], (T*)c->tk.v[layer], c->tk.d_table, (int)c->tk.pool->blk_elems};
}

static bool flash_small_prepare() { return lds_limit_at_least<flash_prefill_small_kernel>(kFsLdsBytes); }
// every sequence short enough, one pool, bf16: the packed attention kernels take the whole group (false: the per-prompt launches)
static bool pack_attention_ok(fq3_ctx* const* cs, int n, const int* L) {
    if (n < 1 || n > kMaxPack || cs[0]->cfg.dtype != FQ3_BF16 || !cs[0]->opt_flash_prefill || !cs[0]->opt_flash_small) return false;
    for (int q = 0; q < n; ++q)
        if (L[q] > kFsMaxRows || cs[q]->tk.pool != cs[0]->tk.pool || cs[q]->opt_flash_small == 0) return false;
    return flash_small_prepare();
}
static PackSeq pack_seq(fq3_ctx* const* cs, int n, const int* L, const int* n_pad) {
    PackSeq sq{};
    sq.n = n;
    for (int q = 0; q < n; ++q) {
        sq.table[q] = cs[q]->tk.d_table; sq.off[q + 1] = sq.off[q] + L[q]; sq.n_pad[q] = n_pad[q]; sq.rope_delta[q] = cs[q]->rope_delta;
    }
    return sq;
}
// one layer's q / k norm + RoPE + KV write and causal attention for every sequence of the pack: two launches
static bool pack_attention_layer(fq3_ctx* c0, int layer, const fq3_layer_weights& w, const PackSeq& sq, int Lmax, bf16_t* QKV, bf16_t* ATT,
                                 float scale, hipStream_t s) {
    const fq3_stack_dims& d = c0->cfg.talker;
    const int NH = d.n_heads, NKV = d.n_kv_heads, Lt = sq.off[sq.n];
    const PagedKV<bf16_t> kv = paged_kv<bf16_t>(c0, layer);
    hipLaunchKernelGGL((qk_norm_rope_kv_pack_kernel<bf16_t>), dim3((Lt * (NH + 2 * NKV) + 3) / 4), dim3(256), 0, s, QKV, (const bf16_t*)w.q_norm,
                       (const bf16_t*)w.k_norm, d.rms_eps, c0->wt.talker_cos, c0->wt.talker_sin, c0->wt.talker_rope_len, kv, sq, NH, NKV);
    hipLaunchKernelGGL(flash_prefill_small_kernel, dim3((Lmax + kFaQ - 1) / kFaQ, NH, sq.n), dim3(256), kFsLdsBytes, s, (const bf16_t*)QKV, kv, ATT, sq,
                       NH, NKV, scale);
    return hipGetLastError() == hipSuccess;                // a refused launch (e.g. the 158 KB of LDS) must not leave ATT stale silently
}

// the same for a packed continuation (PackCont: prefill_kernels.cuh); S[q] = the key splits of sequence q
static PackCont pack_cont(fq3_ctx* const* cs, int n, const int* start, const int* cnt, const int* S) {
    const int NH = cs[0]->cfg.talker.n_heads;
    PackCont sq{};
    sq.n = n;
    for (int q = 0; q < n; ++q) {
        sq.table[q] = cs[q]->tk.d_table; sq.off[q + 1] = sq.off[q] + cnt[q]; sq.start[q] = start[q]; sq.rope_delta[q] = cs[q]->rope_delta;
        sq.zoff[q + 1] = sq.zoff[q] + S[q];
        sq.wsoff[q] = q == 0 ? 0 : sq.wsoff[q - 1] + (S[q - 1] > 1 ? S[q - 1] * cnt[q - 1] * NH * kFcRec : 0);
    }
    return sq;
}
// norm + RoPE + K/V write in one launch, one flash launch over every (sequence, query block, head, key split) -- nqb_max = the most
// query blocks of a sequence -- plus one merge launch when some sequence splits; the records live in the split-K workspace pf_ws
static void pack_cont_attention_layer(fq3_ctx* c0, int layer, const fq3_layer_weights& w, const PackCont& sq, int nqb_max, bf16_t* QKV, bf16_t* ATT,
                                      float scale, hipStream_t s) {
    const fq3_stack_dims& d = c0->cfg.talker;
    const int NH = d.n_heads, NKV = d.n_kv_heads, n = sq.n, Lt = sq.off[n];
    const PagedKV<bf16_t> kv = paged_kv<bf16_t>(c0, layer);
    hipLaunchKernelGGL((qk_norm_rope_kv_cont_pack_kernel<bf16_t>), dim3((Lt * (NH + 2 * NKV) + 3) / 4), dim3(256), 0, s, QKV, (const bf16_t*)w.q_norm,
                       (const bf16_t*)w.k_norm, d.rms_eps, c0->wt.talker_cos, c0->wt.talker_sin, c0->wt.talker_rope_len, kv, sq, NH, NKV);
    hipLaunchKernelGGL(flash_prefill_cont_pack_kernel, dim3(nqb_max, NH, sq.zoff[n]), dim3(256), 0, s, (const bf16_t*)QKV, kv, ATT, (float*)c0->pf_ws,
                       sq, NH, NKV, scale);
    if (sq.zoff[n] > n) hipLaunchKernelGGL(flash_cont_pack_merge_kernel, dim3((Lt * NH + 1) / 2), dim3(256), 0, s, (const float*)c0->pf_ws, ATT, sq, NH);
}

// shape choice: short prompts keep 64-query blocks, one per workgroup (parallelism first); from 1024 tokens the blocks are paired
// (equal work per workgroup under the causal mask), from 3072 tokens they hold 128 queries
static void flash_prefill_launch(const bf16_t* qkv, const PagedKV<bf16_t>& kv, bf16_t* out, int L, int n_pad, int NH,
                                 int NKV, float scale, hipStream_t s) {
    if (L >= 3072) {
        const int nqb = (L + 127) / 128;
        hipLaunchKernelGGL((flash_prefill_kernel<8, true>), dim3((nqb + 1) / 2, NH), dim3(512), 0, s, qkv, kv, out, L, n_pad, NH, NKV, scale, nqb);
    } else if (L >= 1024) {
        const int nqb = (L + 63) / 64;
        hipLaunchKernelGGL((flash_prefill_kernel<4, true>), dim3((nqb + 1) / 2, NH), dim3(256), 0, s, qkv, kv, out, L, n_pad, NH, NKV, scale, nqb);
    } else {
        const int nqb = (L + 63) / 64;
        hipLaunchKernelGGL((flash_prefill_kernel<4, false>), dim3(nqb, NH), dim3(256), 0, s, qkv, kv, out, L, n_pad, NH, NKV, scale, nqb);
    }
}

constexpr long kPrefillWsFloats = 8L << 20;       // split-K partials of the short-prompt GEMMs (32 MB)
// every prefill GEMM lends the split-K workspace: that also marks it free to take the weight-stationary kernel (skinny_gemm.cuh)
// (kind: 0 = a plain matrix, 1 = [gate | up] halves -- which fragment-major copy the weight-stationary kernel would read, fq3_ctx.h)
template <typename T>
GemmArgs lin(fq3_ctx* c, const void* A, int M, int K, const void* W, int N, void* Y, int kind = 0) {
    GemmArgs a{}; a.A = A; a.lda = K; a.M = M; a.a_rows = M; a.n_taps = 1; a.tap_off[0] = 0; a.Cin = K; a.W = W; a.N = N;
    a.bias_mod = N; a.Y = Y; a.ldy = N; a.ws = (float*)c->pf_ws; a.ws_floats = kPrefillWsFloats; a.no_skinny = c->opt_no_skinny;
    if (sizeof(T) == 2 && c->opt_packed && M <= kSkinnyMaxRows) a.Wp = fq3_packed_find_(W, kind);
    if (sizeof(T) == 2 && kind == 1 && c->opt_swiglu_tile && M > kSkinnyMaxRows) a.Wi = fq3_packed_find_(W, 2);
    return a;
}
template <typename T> void gemm(const GemmArgs& a, hipStream_t s) { gemm_launch<T>(a, s); }

// CUs of the current device (the key-split rule of the continuation's flash attention); asked once
static int device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}

// The prefill of n prompts at once is one skeleton for every entry point, in two steps.  Everything row-wise (norms, the four GEMMs,
// SwiGLU) runs over the PACKED rows of all prompts (rows[q] of prompt q from packed row off[q] on) -- one pass over the layer's weights
// instead of n -- on the workspaces of cs[0] (sum of the rows <= its max_seq_len).  Per element the arithmetic does not depend on n;
// what can differ is the GEMM tile / split-K choice, which depends on the row count (bf16: last-bit level).
// Step 1: dimension checks, the workspace, off[0 .. n] and the packed copy of the embeddings.
template <typename T>
int prefill_begin(fq3_ctx* const* cs, int n, const void* const* embeds, const int* rows, int (&off)[kMaxPack + 1], hipStream_t s) {
    fq3_ctx* c = cs[0];
    const int H = c->cfg.talker.hidden, I = c->cfg.talker.inter;
    if (H % 32 || I % 32) return fq3_fail_(FQ3_EUNSUPPORTED, "MFMA prefill needs hidden and intermediate sizes that are multiples of 32");
    if (int r = fq3_prefill_reserve_(c)) return r;
    off[0] = 0;
    for (int q = 0; q < n; ++q) off[q + 1] = off[q] + rows[q];
    for (int q = 0; q < n; ++q)
        if (hipMemcpyAsync((T*)c->pf_x + (size_t)off[q] * H, embeds[q], (size_t)rows[q] * H * c->esz, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fq3_fail_(FQ3_EHIP, "prefill: copy of the prompt embeddings failed");
    return 0;
}
// Step 2: the layers, then the final norm of each prompt's last row -> out_hidden[q] and its logits through the decode-path head GEMV
// where out_logits[q] is given.  Only the sequence-specific step is the caller's: attn(layer, weights, QKV, ATT) does q/k norm + RoPE +
// KV write into each context's own cache and the causal attention over it, QKV -> ATT, and returns 0 or the error to return.
template <typename T, typename Attn>
int prefill_layers(fq3_ctx* const* cs, int n, const int* off, void* const* out_logits, void* const* out_hidden, hipStream_t s, Attn&& attn) {
    fq3_ctx* c = cs[0];
    const fq3_stack_dims& d = c->cfg.talker;
    const int H = d.hidden, I = d.inter, QD = d.n_heads * kHeadDim, per = QD + 2 * d.n_kv_heads * kHeadDim, Lt = off[n];
    T *X = (T*)c->pf_x, *XN = (T*)c->pf_xn, *QKV = (T*)c->pf_qkv, *ATT = (T*)c->pf_att, *GU = (T*)c->pf_gu, *ACT = (T*)c->pf_act;
    for (int i = 0; i < d.n_layers; ++i) {
        const fq3_layer_weights& w = c->tl[i];
        rmsnorm_rows<T>((const T*)X, (const T*)w.input_norm, XN, Lt, H, d.rms_eps, s);
        gemm<T>(lin<T>(c, XN, Lt, H, w.qkv, per, QKV), s);
        if (int r = attn(i, w, QKV, ATT)) return r;
        { GemmArgs a = lin<T>(c, ATT, Lt, QD, w.o, H, X); a.res = X; a.ldr = H; gemm<T>(a, s); }
        rmsnorm_rows<T>((const T*)X, (const T*)w.post_norm, XN, Lt, H, d.rms_eps, s);
        gemm_swiglu_halves<T>(lin<T>(c, XN, Lt, H, w.gate_up, 2 * I, GU, 1), ACT, s);
        { GemmArgs a = lin<T>(c, ACT, Lt, I, w.down, H, X); a.res = X; a.ldr = H; gemm<T>(a, s); }
    }
    for (int q = 0; q < n; ++q) {
        hipLaunchKernelGGL((rmsnorm_kernel<T>), dim3(1), dim3(256), 0, s, (const T*)X + (size_t)(off[q + 1] - 1) * H, (const T*)c->wt.talker_final_norm,
                           (T*)out_hidden[q], H, d.rms_eps);
        if (out_logits && out_logits[q])
            if (int r = fq3_codec_head_launch_(cs[q], out_hidden[q], out_logits[q], s)) return r;
    }
    return 0;
}

static float attn_scale() { return 1.0f / sqrtf((float)kHeadDim); }

// one prompt's attention step on its slice of the packed rows (tables and options of c0 = the pack's first context, cache and
// rope_delta of the prompt's own cq): norm + RoPE + KV write, then the flash kernels (bf16 with flash_prefill) or the wave kernel
template <typename T>
void prompt_attention(fq3_ctx* c0, fq3_ctx* cq, int layer, const fq3_layer_weights& w, T* qkv, T* att, int L, int n_pad, hipStream_t s) {
    const fq3_stack_dims& d = c0->cfg.talker;
    const int NH = d.n_heads, NKV = d.n_kv_heads;
    const PagedKV<T> kv = paged_kv<T>(cq, layer);
    hipLaunchKernelGGL((qk_norm_rope_kv_kernel<T>), dim3((L * (NH + 2 * NKV) + 3) / 4), dim3(256), 0, s, qkv, (const T*)w.q_norm,
                       (const T*)w.k_norm, d.rms_eps, c0->wt.talker_cos, c0->wt.talker_sin, c0->wt.talker_rope_len, cq->rope_delta,
                       kv, L, n_pad, NH, NKV);
    if constexpr (sizeof(T) == 2) {
        if (c0->opt_flash_prefill) return flash_prefill_launch(qkv, kv, att, L, n_pad, NH, NKV, attn_scale(), s);
    }
    hipLaunchKernelGGL((prefill_attn_kernel<T>), dim3((L * NH + 3) / 4), dim3(256), 0, s, (const T*)qkv, kv, att, L, n_pad, NH, NKV, attn_scale());
}

// the same for a continuation: the prompt's n new rows behind its cached rows [0, start).  S > 0: the flash kernel with S key splits (+
// the merge launch when S > 1), its records in the split-K workspace pf_ws -- the GEMMs that lend it run before and after the
// attention, and the prompts of a pack take it in turn: stream order.  S == 0: the wave kernel.
template <typename T>
void prompt_attention_cont(fq3_ctx* c0, fq3_ctx* cq, int layer, const fq3_layer_weights& w, T* qkv, T* att, int start, int n, int S,
                           hipStream_t s) {
    const fq3_stack_dims& d = c0->cfg.talker;
    const int NH = d.n_heads, NKV = d.n_kv_heads;
    const PagedKV<T> kv = paged_kv<T>(cq, layer);
    hipLaunchKernelGGL((qk_norm_rope_kv_cont_kernel<T>), dim3((n * (NH + 2 * NKV) + 3) / 4), dim3(256), 0, s, qkv, (const T*)w.q_norm,
                       (const T*)w.k_norm, d.rms_eps, c0->wt.talker_cos, c0->wt.talker_sin, c0->wt.talker_rope_len, cq->rope_delta,
                       kv, start, n, NH, NKV);
    if constexpr (sizeof(T) == 2) {
        if (S > 0) {
            hipLaunchKernelGGL(flash_prefill_cont_kernel, dim3((n + kFaQ - 1) / kFaQ, NH, S), dim3(256), 0, s, (const bf16_t*)qkv, kv, att,
                               (float*)c0->pf_ws, start, n, NH, NKV, attn_scale(), S);
            if (S > 1) hipLaunchKernelGGL(flash_cont_merge_kernel, dim3((n * NH + 1) / 2), dim3(256), 0, s, (const float*)c0->pf_ws, att, n, NH, S);
            return;
        }
    }
    hipLaunchKernelGGL((prefill_attn_cont_kernel<T>), dim3((n * NH + 3) / 4), dim3(256), 0, s, (const T*)qkv, kv, att, start, n, NH, NKV, attn_scale());
}

// fq3_prefill / fq3_prefill_batch: prompts of L[q] rows, the first n_pad[q] of them left padding.  Every prompt <= 256 rows, one pool,
// bf16: the pack's attention in two launches per layer (every key tile resident: flash_prefill_small_kernel); else per prompt.
template <typename T>
int prefill_batch_t(fq3_ctx* const* cs, int n, const void* const* embeds, const int* L, const int* n_pad, void* const* out_logits,
                    void* const* out_hidden, hipStream_t s) {
    fq3_ctx* c = cs[0];
    const int QD = c->cfg.talker.n_heads * kHeadDim, per = QD + 2 * c->cfg.talker.n_kv_heads * kHeadDim;
    int off[kMaxPack + 1];
    if (int r = prefill_begin<T>(cs, n, embeds, L, off, s)) return r;
    const bool small = pack_attention_ok(cs, n, L);
    const PackSeq sq = small ? pack_seq(cs, n, L, n_pad) : PackSeq{};
    int Lmax = 0;
    for (int q = 0; q < n; ++q) Lmax = std::max(Lmax, L[q]);
    return prefill_layers<T>(cs, n, off, out_logits, out_hidden, s, [&](int i, const fq3_layer_weights& w, T* QKV, T* ATT) {
        if (small) {
            if (!pack_attention_layer(c, i, w, sq, Lmax, (bf16_t*)QKV, (bf16_t*)ATT, attn_scale(), s))
                return fq3_fail_(FQ3_EHIP, "prefill: the packed attention launch failed");
            return 0;
        }
        for (int q = 0; q < n; ++q)
            prompt_attention<T>(c, cs[q], i, w, QKV + (size_t)off[q] * per, ATT + (size_t)off[q] * QD, L[q], n_pad[q], s);
        return 0;
    });
}

// fq3_prefill_continue / fq3_prefill_continue_batch: cnt[q] NEW rows of each prompt behind K/V rows [0, start[q]) that are already in
// its cache.  may_pack (bf16, flash_prefill, one pool): norm + RoPE + K/V write take each sequence's position base and table from a
// PackCont in one launch, and the attention of the whole pack is one flash launch over every (sequence, query block, head, key split)
// plus one merge launch when some sequence splits.  Else the single-prompt kernels run on each prompt's slice.  The key splits are a
// pure function of (start, cnt): fixed once per call.
template <typename T>
int prefill_continue_batch_t(fq3_ctx* const* cs, int n, const void* const* embeds, const int* start, const int* cnt, void* const* out_logits,
                             void* const* out_hidden, bool may_pack, hipStream_t s) {
    fq3_ctx* c = cs[0];
    const int NH = c->cfg.talker.n_heads, NKV = c->cfg.talker.n_kv_heads, QD = NH * kHeadDim, per = QD + 2 * NKV * kHeadDim;
    int off[kMaxPack + 1];
    if (int r = prefill_begin<T>(cs, n, embeds, cnt, off, s)) return r;
    const bool flash = sizeof(T) == 2 && c->opt_flash_prefill;
    bool pack = may_pack && flash;
    for (int q = 0; q < n; ++q) pack = pack && cs[q]->tk.pool == c->tk.pool;
    int S[kMaxPack] = {}, nqb_max = 0;                    // per prompt: its key splits; 0 = the wave kernel
    if (pack) flash_cont_pack_splits(start, cnt, n, NH, device_cus(), kPrefillWsFloats, S);
    else if (flash)
        for (int q = 0; q < n; ++q) S[q] = flash_cont_splits(start[q], cnt[q], NH, device_cus(), kPrefillWsFloats);
    const PackCont sq = pack ? pack_cont(cs, n, start, cnt, S) : PackCont{};
    for (int q = 0; q < n; ++q) nqb_max = std::max(nqb_max, (cnt[q] + kFaQ - 1) / kFaQ);
    return prefill_layers<T>(cs, n, off, out_logits, out_hidden, s, [&](int i, const fq3_layer_weights& w, T* QKV, T* ATT) {
        if (pack) {
            pack_cont_attention_layer(c, i, w, sq, nqb_max, (bf16_t*)QKV, (bf16_t*)ATT, attn_scale(), s);
            return 0;
        }
        for (int q = 0; q < n; ++q)
            prompt_attention_cont<T>(c, cs[q], i, w, QKV + (size_t)off[q] * per, ATT + (size_t)off[q] * QD, start[q], cnt[q], S[q], s);
        return 0;
    });
}

}  // namespace

// The matrix-core prefill's activation workspace (max_seq_len rows of x, norm(x), qkv, attention, gate|up, act + the split-K
// partials): allocated on first use, or up front through fq3_prefill_reserve -- a scheduler that prefills into spare contexts
// while other lanes decode must not meet a hipMalloc there.
int fq3_prefill_reserve_(fq3_ctx* c) {
    if (c->pf_x) return 0;
    const fq3_stack_dims& d = c->cfg.talker;
    const size_t H = d.hidden, I = d.inter, QD = (size_t)d.n_heads * kHeadDim, per = QD + 2 * (size_t)d.n_kv_heads * kHeadDim;
    const size_t rows = (size_t)c->cfg.max_seq_len;
    int r;
    void* x = nullptr;
    if ((r = fq3_dmalloc_(c, &x, rows * H * c->esz))) return r;
    if ((r = fq3_dmalloc_(c, &c->pf_xn, rows * H * c->esz))) return r;
    if ((r = fq3_dmalloc_(c, &c->pf_qkv, rows * per * c->esz))) return r;
    if ((r = fq3_dmalloc_(c, &c->pf_att, rows * QD * c->esz))) return r;
    if ((r = fq3_dmalloc_(c, &c->pf_gu, rows * 2 * I * c->esz))) return r;
    if ((r = fq3_dmalloc_(c, &c->pf_act, rows * I * c->esz))) return r;
    if ((r = fq3_dmalloc_(c, &c->pf_ws, (size_t)kPrefillWsFloats * sizeof(float)))) return r;
    c->pf_x = x;                                   // set last: marks the whole set as present
    return 0;
}

int fq3_prefill_batch_mfma_(fq3_ctx* const* cs, int n, const void* const* embeds, const int* L, const int* n_pad, void* const* out_logits,
                            void* const* out_hidden, hipStream_t s) {
    return cs[0]->cfg.dtype == FQ3_BF16 ? prefill_batch_t<bf16_t>(cs, n, embeds, L, n_pad, out_logits, out_hidden, s)
                                        : prefill_batch_t<float>(cs, n, embeds, L, n_pad, out_logits, out_hidden, s);
}

int fq3_prefill_mfma_(fq3_ctx* c, const void* embeds, int L, int n_pad, void* out_logits, void* out_hidden, hipStream_t s) {
    return fq3_prefill_batch_mfma_(&c, 1, &embeds, &L, &n_pad, &out_logits, &out_hidden, s);
}

static int prefill_continue_any(fq3_ctx* const* cs, int n, const void* const* embeds, const int* start, const int* cnt, void* const* out_logits,
                                void* const* out_hidden, bool may_pack, hipStream_t s) {
    return cs[0]->cfg.dtype == FQ3_BF16 ? prefill_continue_batch_t<bf16_t>(cs, n, embeds, start, cnt, out_logits, out_hidden, may_pack, s)
                                        : prefill_continue_batch_t<float>(cs, n, embeds, start, cnt, out_logits, out_hidden, may_pack, s);
}

int fq3_prefill_continue_batch_mfma_(fq3_ctx* const* cs, int n, const void* const* embeds, const int* start, const int* cnt,
                                     void* const* out_logits, void* const* out_hidden, hipStream_t s) {
    return prefill_continue_any(cs, n, embeds, start, cnt, out_logits, out_hidden, cs[0]->opt_cont_pack != 0, s);
}

// the single continuation keeps the single-prompt kernels: it may not use the pack kernels
int fq3_prefill_continue_mfma_(fq3_ctx* c, const void* embeds, int start, int n, void* out_logits, void* out_hidden, hipStream_t s) {
    return prefill_continue_any(&c, 1, &embeds, &start, &n, &out_logits, &out_hidden, false, s);
}
