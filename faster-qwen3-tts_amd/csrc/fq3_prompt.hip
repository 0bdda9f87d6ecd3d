// Prompt builder on the device: replaces the ~40 small ATen launches of the reference's
// _build_talker_inputs_local (/root/reference/faster_qwen3_tts/model.py:583-805) and upstream generate_icl_prompt
// (called at model.py:699-712) with: one gather, two matrix-core GEMMs (text_projection: fc1 + SiLU, fc2) over ALL text
// tokens of the prompt at once, and one row-assembly kernel.  Rounding points are those of the module-by-module Torch
// execution: one rounding to T after fc1, after SiLU, after fc2, after the 16-way embedding sum, after text + codec.
#define FQ3_SKINNY_EXTERN           // skinny_gemm.cuh: the weight-stationary GEMM kernels are instantiated in fq3_prefill.hip only
#include "fq3_ctx.h"
#include "codec_kernels.cuh"
#include "prompt_kernels.cuh"

using namespace fq3;

namespace {

// the three launches of text_projection(text_embedding(ids)) over workspaces x, h of at least n rows of text_hidden
template <typename T>
void text_project_launch(fq3_ctx* c, const int64_t* ids, int n, void* x, void* h, void* out, hipStream_t s) {
    const fq3_prompt_weights& w = c->pw;
    const int Ht = w.text_hidden, H = c->cfg.talker.hidden;
    hipLaunchKernelGGL((text_gather_kernel<T>), dim3(n), dim3(256), 0, s, ids, (const T*)w.text_embedding, (T*)x, n, Ht, w.text_vocab);
    GemmArgs a{};
    a.A = x; a.lda = Ht; a.M = n; a.a_rows = n; a.n_taps = 1; a.tap_off[0] = 0; a.Cin = Ht; a.W = w.fc1_w; a.N = Ht;
    a.bias = w.fc1_b; a.bias_mod = Ht; a.Y = h; a.ldy = Ht; a.act = 3;
    // fc1 output and SiLU output are two module outputs in Torch (two roundings): the epilogue rounds after the bias and
    // again after the activation
    gemm_launch<T>(a, s);
    GemmArgs b{};
    b.A = h; b.lda = Ht; b.M = n; b.a_rows = n; b.n_taps = 1; b.tap_off[0] = 0; b.Cin = Ht; b.W = w.fc2_w; b.N = H;
    b.bias = w.fc2_b; b.bias_mod = H; b.Y = out; b.ldy = H;
    gemm_launch<T>(b, s);
}

template <typename T>
int text_project_t(fq3_ctx* c, const int64_t* ids, int n, void* out, hipStream_t s) {
    const int Ht = c->pw.text_hidden;
    if (n > c->pw_cap) {
        const int cap = (n + 255) / 256 * 256;
        void *x = nullptr, *h = nullptr;
        if (int r = fq3_dmalloc_(c, &x, (size_t)cap * Ht * c->esz)) return r;       // old workspaces stay owned by the context
        if (int r = fq3_dmalloc_(c, &h, (size_t)cap * Ht * c->esz)) return r;
        c->pw_x = x; c->pw_h = h; c->pw_cap = cap;
    }
    text_project_launch<T>(c, ids, n, c->pw_x, c->pw_h, out, s);
    return 0;
}

}  // namespace

// text_projection(text_embedding(ids)) into out[n][H] over the caller's workspaces x, h (n rows of text_hidden each): the launches of
// fq3_text_project / fq3_decode_text_append, for fq3_batch_text_append (fq3_batch.hip)
void fq3_text_project_launch_(fq3_ctx* c, const int64_t* ids, int n, void* x, void* h, void* out, hipStream_t s) {
    if (c->cfg.dtype == FQ3_BF16) text_project_launch<bf16_t>(c, ids, n, x, h, out, s);
    else text_project_launch<float>(c, ids, n, x, h, out, s);
}

extern "C" int fq3_bind_prompt_weights(fq3_ctx* c, const fq3_prompt_weights* w) {
    if (!c || !w) return fq3_fail_(FQ3_EINVAL, "null argument");
    if (!w->text_embedding || !w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b) return fq3_fail_(FQ3_EINVAL, "prompt weight table has null entries");
    if (w->text_vocab <= 0 || w->text_hidden <= 0 || w->text_hidden % 32 || c->cfg.talker.hidden % 32)
        return fq3_fail_(FQ3_EUNSUPPORTED, "text_hidden and the talker hidden size must be multiples of 32 (MFMA K step)");
    c->pw = *w;
    c->pw_bound = true;
    return FQ3_OK;
}

extern "C" int fq3_text_project(fq3_ctx* c, const int64_t* ids, int n, void* out, void* stream) {
    if (!c || !ids || !out) return fq3_fail_(FQ3_EINVAL, "null argument");
    if (!c->pw_bound) return fq3_fail_(FQ3_ESTATE, "prompt weights not bound");
    if (n <= 0) return fq3_fail_(FQ3_EINVAL, "need at least one token");
    hipStream_t s = (hipStream_t)stream;
    int r = c->cfg.dtype == FQ3_BF16 ? text_project_t<bf16_t>(c, ids, n, out, s) : text_project_t<float>(c, ids, n, out, s);
    if (r) return r;
    if (hipGetLastError() != hipSuccess) return fq3_fail_(FQ3_EHIP, "fq3_text_project launch failed");
    return FQ3_OK;
}

extern "C" int fq3_decode_text_open(fq3_ctx* c, int capacity_rows, void* stream) {
    if (!c) return fq3_fail_(FQ3_EINVAL, "null ctx");
    if (capacity_rows <= 0) return fq3_fail_(FQ3_EINVAL, "capacity_rows must be positive");
    if (!c->pw_bound) return fq3_fail_(FQ3_ESTATE, "prompt weights not bound");
    if (!c->armed) return fq3_fail_(FQ3_ESTATE, "fq3_decode_text_open needs fq3_decode_begin first");
    if (c->tt_session) return fq3_fail_(FQ3_ESTATE, "this loop's text table has been opened already");
    if (capacity_rows < c->begin_trailing_len) return fq3_fail_(FQ3_EINVAL, "capacity_rows is smaller than the table fq3_decode_begin was given");
    const int Ht = c->pw.text_hidden, H = c->cfg.talker.hidden;
    if (capacity_rows > c->tt_alloc) {
        // a longer table than any session before: new buffers (the old ones stay owned by the context; no captured graph holds their
        // addresses -- the frame reads the table through DecodeState::trailing_text)
        const int cap = (capacity_rows + 255) / 256 * 256;
        void *t = nullptr, *x = nullptr, *h = nullptr;
        if (int r = fq3_dmalloc_(c, &t, (size_t)cap * H * c->esz)) return r;
        if (int r = fq3_dmalloc_(c, &x, (size_t)cap * Ht * c->esz)) return r;
        if (int r = fq3_dmalloc_(c, &h, (size_t)cap * Ht * c->esz)) return r;
        c->tt_tab = t; c->tt_x = x; c->tt_h = h; c->tt_alloc = cap;
    }
    const int words = (int)((size_t)c->begin_trailing_len * H * c->esz / 4);
    hipLaunchKernelGGL(text_open_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c->st, (uint32_t*)c->tt_tab,
                       (const uint32_t*)c->begin_trailing, words);
    if (hipGetLastError() != hipSuccess) return fq3_fail_(FQ3_EHIP, "fq3_decode_text_open launch failed");
    c->tt_cap = capacity_rows; c->tt_rows = c->begin_trailing_len; c->tt_open = true; c->tt_session = true;
    return FQ3_OK;
}

extern "C" int fq3_decode_text_append(fq3_ctx* c, const int64_t* ids, int n, int final, void* stream) {
    if (!c) return fq3_fail_(FQ3_EINVAL, "null ctx");
    if (n < 0 || (n > 0 && !ids) || (n == 0 && !final)) return fq3_fail_(FQ3_EINVAL, "need ids, or final with no ids");
    if (!c->tt_open) return fq3_fail_(FQ3_ESTATE, "the text table is not open");
    if (n > c->tt_cap - c->tt_rows) return fq3_fail_(FQ3_EINVAL, "append past the capacity of the text table");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        void* out = (char*)c->tt_tab + (size_t)c->tt_rows * c->cfg.talker.hidden * c->esz;
        if (c->cfg.dtype == FQ3_BF16) text_project_launch<bf16_t>(c, ids, n, c->tt_x, c->tt_h, out, s);
        else text_project_launch<float>(c, ids, n, c->tt_x, c->tt_h, out, s);
    }
    hipLaunchKernelGGL(text_publish_kernel, dim3(1), dim3(1), 0, s, c->st, c->tt_rows + n, final ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return fq3_fail_(FQ3_EHIP, "fq3_decode_text_append launch failed");
    c->tt_rows += n;
    if (final) c->tt_open = false;
    return FQ3_OK;
}

extern "C" int fq3_decode_text_rows(const fq3_ctx* c, int* n_rows, int* closed) {
    if (!c) return fq3_fail_(FQ3_EINVAL, "null ctx");
    if (!c->tt_session) return fq3_fail_(FQ3_ESTATE, "no text table was opened for this loop");
    if (n_rows) *n_rows = c->tt_rows;
    if (closed) *closed = c->tt_open ? 0 : 1;
    return FQ3_OK;
}

extern "C" int fq3_decode_text_read(fq3_ctx* c, int from, int count, void* out, void* stream) {
    if (!c || !out) return fq3_fail_(FQ3_EINVAL, "null argument");
    if (!c->tt_session) return fq3_fail_(FQ3_ESTATE, "no text table was opened for this loop");
    if (from < 0 || count < 0 || from + count > c->tt_rows) return fq3_fail_(FQ3_EINVAL, "range");
    if (count == 0) return FQ3_OK;
    const size_t row = (size_t)c->cfg.talker.hidden * c->esz;
    if (hipMemcpyAsync(out, (const char*)c->tt_tab + from * row, count * row, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return fq3_fail_(FQ3_EHIP, "fq3_decode_text_read copy failed");
    return FQ3_OK;
}

extern "C" int fq3_prompt_rows(fq3_ctx* c, const void* text_rows, int n_text, const int32_t* prog, int n_rows,
                               const int64_t* ref_codes, int n_ref, const void* spk_embed, void* out, void* stream) {
    if (!c || !prog || !out) return fq3_fail_(FQ3_EINVAL, "null argument");
    if (!c->bound) return fq3_fail_(FQ3_ESTATE, "weights not bound");
    if (n_rows <= 0) return fq3_fail_(FQ3_EINVAL, "need at least one row");
    if (c->cfg.num_code_groups != 16) return fq3_fail_(FQ3_EUNSUPPORTED, "the prompt builder is built for 16 code groups");
    if (c->cfg.talker.hidden % 8) return fq3_fail_(FQ3_EUNSUPPORTED, "hidden size must be a multiple of 8");
    RowTables tabs{};
    tabs.t[0] = c->wt.codec_embedding;
    for (int i = 1; i < 16; ++i) tabs.t[i] = c->pemb[i - 1];
    hipStream_t s = (hipStream_t)stream;
    const int H = c->cfg.talker.hidden, V0 = c->cfg.talker.vocab, V1 = c->cfg.predictor.vocab;
    if (c->cfg.dtype == FQ3_BF16)
        hipLaunchKernelGGL((prompt_rows_kernel<bf16_t>), dim3(n_rows), dim3(256), 0, s, (const bf16_t*)text_rows, text_rows ? n_text : 0, prog,
                           ref_codes, ref_codes ? n_ref : 0, (const bf16_t*)spk_embed, tabs, V0, V1, (bf16_t*)out, H);
    else
        hipLaunchKernelGGL((prompt_rows_kernel<float>), dim3(n_rows), dim3(256), 0, s, (const float*)text_rows, text_rows ? n_text : 0, prog,
                           ref_codes, ref_codes ? n_ref : 0, (const float*)spk_embed, tabs, V0, V1, (float*)out, H);
    if (hipGetLastError() != hipSuccess) return fq3_fail_(FQ3_EHIP, "fq3_prompt_rows launch failed");
    return FQ3_OK;
}
