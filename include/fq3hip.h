/*
 * fq3hip.h -- C ABI of libfq3hip.so: the MI355X (gfx950) fast decode path for Qwen3-TTS.
 *
 * This is the drop-in boundary.  Every entry point is extern "C", takes plain device pointers,
 * sizes and a hipStream_t passed as void*; there are no torch types in any signature.  Python binds
 * it with ctypes (faster-qwen3-tts_amd/fq3hip/_lib.py); INTEGRATION.md shows the stub a reference
 * maintainer would add.  The precedent for a ctypes-bound native runtime in the reference is the
 * libqwen adapter, /root/reference/faster_qwen3_tts/ggml_backend.py:31-39.
 *
 * Each function cites the reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - return 0 on success, a negative FQ3_E* code on failure; fq3_last_error() gives the message.
 *     Nothing throws across the ABI.
 *   - all work is enqueued on the stream argument and is asynchronous to the host unless stated.
 *   - a context is bound to one device and is NOT re-entrant (static buffers), exactly like the
 *     reference's graph objects (examples/openai_server.py:71 serialises callers with a lock).
 *   - "T" below is the context dtype: bf16 (FQ3_BF16) or fp32 (FQ3_F32).  Weights, activations, KV
 *     cache, logits and sampling noise are all T; accumulation is fp32.
 *   - weight pointers are BORROWED: the caller keeps the allocations alive for the context lifetime.
 */
#ifndef FQ3HIP_H
#define FQ3HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQ3_ABI_VERSION 5

enum { FQ3_BF16 = 0, FQ3_F32 = 1,
       FQ3_BF16X2 = 2 };   /* codec decoder only: activations kept as a bf16 high part + a bf16 residual (16 mantissa bits), products of the
                            * two halves with the bf16 weights on v_mfma_f32_16x16x32_bf16; see fq3_codec_config.dtype */
enum { FQ3_OK = 0, FQ3_EINVAL = -1, FQ3_EHIP = -2, FQ3_ESTATE = -3, FQ3_ETOOLONG = -4, FQ3_EUNSUPPORTED = -5, FQ3_ENOMEM = -6 };

typedef struct fq3_stack_dims {
    int32_t hidden, inter, n_layers, n_heads, n_kv_heads, head_dim, vocab;
    float rms_eps;
} fq3_stack_dims;

typedef struct fq3_config {
    int32_t dtype;              /* FQ3_BF16 | FQ3_F32 */
    fq3_stack_dims talker;      /* talker_graph.py:36-37 */
    fq3_stack_dims predictor;   /* predictor_graph.py:42-46 */
    int32_t num_code_groups;    /* 16: generate.py:42 */
    int32_t max_seq_len;        /* static talker KV length: model.py:113, talker_graph.py:43 */
    int32_t codec_eos_token_id; /* generate.py:41 */
    int32_t has_projection;     /* small_to_mtp_projection present: predictor_graph.py:54 */
    int32_t max_frames;         /* capacity of the on-device code buffer (>= max_new_tokens) */
} fq3_config;

/* One pre-norm GQA decoder layer.  qkv = rows [q | k | v] of the three projections concatenated,
 * gate_up = rows [gate | up].  All row-major [out, in], no biases (Appendix D of SURVEY.md). */
typedef struct fq3_layer_weights {
    const void* input_norm;  /* [H] */
    const void* qkv;         /* [q_dim + 2*kv_dim, H] */
    const void* q_norm;      /* [head_dim] */
    const void* k_norm;      /* [head_dim] */
    const void* o;           /* [H, q_dim] */
    const void* post_norm;   /* [H] */
    const void* gate_up;     /* [2*I, H] */
    const void* down;        /* [H, I] */
} fq3_layer_weights;

typedef struct fq3_weight_table {
    const fq3_layer_weights* talker_layers;     /* talker.n_layers entries (host array) */
    const void* talker_final_norm;              /* [H] */
    const void* codec_embedding;                /* [V, H]   talker.get_input_embeddings(), generate.py:100 */
    const void* codec_head;                     /* [V, H]   generate.py:101 */
    const fq3_layer_weights* predictor_layers;  /* predictor.n_layers entries */
    const void* predictor_final_norm;           /* [Hp] */
    const void* proj_w;                         /* [Hp, H] or NULL (identity)  predictor_graph.py:54 */
    const void* proj_b;                         /* [Hp] or NULL */
    const void* const* predictor_embeddings;    /* 15 x [Vp, H]   predictor_graph.py:57 */
    const void* const* lm_heads;                /* 15 x [Vp, Hp]  predictor_graph.py:56 */
    /* RoPE tables, fp32 values already rounded through T, [n_pos, head_dim/2] each.  Built by the
     * host with the same torch ops as the upstream rotary module so they are bit-identical to it. */
    const float* talker_cos;  const float* talker_sin;  int32_t talker_rope_len;
    const float* pred_cos;    const float* pred_sin;    int32_t pred_rope_len;
} fq3_weight_table;

/* Sampling policy (sampling.py:32-41 keyword arguments + generate.py:26-30). */
typedef struct fq3_sampling {
    float temperature;
    int32_t top_k;
    float top_p;
    int32_t do_sample;
    float repetition_penalty;
} fq3_sampling;

typedef struct fq3_ctx fq3_ctx;

const char* fq3_last_error(void);
int fq3_abi_version(void);

/* Replaces TalkerGraph.__init__ + PredictorGraph.__init__ (talker_graph.py:27-58,
 * predictor_graph.py:34-76): allocates the KV cache, I/O buffers and scratch on the current device.  The talker's KV cache is
 * PAGED: blocks of 64 keys (one attention tile) addressed through a per-context block table; this entry point gives the
 * context a private pool of ceil(max_seq_len / 64) blocks, all taken at creation -- the static cache of the reference
 * (talker_graph.py:43,153-170). */
int fq3_ctx_create(const fq3_config* cfg, fq3_ctx** out);
int fq3_ctx_destroy(fq3_ctx* ctx);

/* ---- paged KV: a block pool shared by the contexts of one scheduler (no reference equivalent: the reference reserves
 * max_seq_len slots per graph object, talker_graph.py:43) ------------------------------------------------------------------
 * A pool holds n_blocks blocks of 64 keys for every talker layer (K and V).  A pooled context owns nothing when idle; prefill
 * (fq3_prefill / fq3_prefill_batch / fq3_kv_import) takes the blocks of the prompt, fq3_decode_begin those of
 * prefill_len + max_new_tokens, fq3_talker_step that of its position; FQ3_ENOMEM (and nothing taken) when the pool is short.
 * fq3_kv_release hands blocks back; the caller makes sure that the context's queued work has finished (the same condition
 * under which a static cache may be overwritten).  Not thread-safe per context; the pool itself is. */
typedef struct fq3_kv_pool fq3_kv_pool;
int fq3_kv_pool_create(const fq3_config* cfg, int n_blocks, fq3_kv_pool** out);
int fq3_kv_pool_destroy(fq3_kv_pool* pool);            /* FQ3_ESTATE while contexts are attached */
/* blocks in total / free now / most ever in use at once; bytes of one block over all layers (K + V) */
int fq3_kv_pool_stats(const fq3_kv_pool* pool, int* n_blocks, int* n_free, int* high_water, int64_t* bytes_per_block);
int fq3_ctx_create_pooled(const fq3_config* cfg, fq3_kv_pool* pool, fq3_ctx** out);
/* take the blocks of key slots [0, n_positions) (capped at max_seq_len) now -- what a scheduler does BEFORE it prefills a request
 * into a spare context (prompt + max_new_tokens + 1), so that a short pool shows up before any work is queued; FQ3_ENOMEM and
 * nothing taken otherwise.  New table entries are written on `stream`. */
int fq3_kv_reserve(fq3_ctx* ctx, int n_positions, void* stream);
/* keep the blocks of key slots [0, keep_positions), return the others to the pool (0: all of them) */
int fq3_kv_release(fq3_ctx* ctx, int keep_positions);
/* blocks this context owns now */
int fq3_kv_blocks(const fq3_ctx* ctx);

/* Kernel-variant switches, all parity-tested both ways (no reference equivalent; the defaults are the measured-fastest):
 *   "weight_nt" 0|1|2 (non-temporal weight loads: none | talker | all), "pred_m2" 0|1 (predictor two-token prefill as one
 *   M = 2 pass), "pred_attn" 0|1 (one-wave predictor attention), "rows_per_wave_max" 1|2, "prefill_mode" 0|1,
 *   "flash_prefill" 0|1 (bf16 prefill attention as a flash-style matrix-core kernel), "skinny_gemm" 0|1 (prompts of <= 416 rows:
 *   weight-stationary GEMMs with the SwiGLU fused into the [gate | up] launch; 0 = the tiled / split-K kernels of longer prompts),
 *   "flash_small" 0|1 (round 5; prompts of <= 256 rows: every key tile of a query block resident in LDS, and the prompts of a packed
 *   fq3_prefill_batch over ONE pool share two attention launches per layer; 0 = the streamed-tile kernel, per prompt; bit-identical),
 *   "packed_weights" 0|1 (round 6; the weight-stationary GEMMs read the fragment-major copies of the layer matrices; bit-identical),
 *   "swiglu_tile" 0|1 (round 6; prefills of more than 416 rows run gate | up on the ring tile over a 16-row-interleaved copy of the
 *   weight with SwiGLU in the epilogue instead of GEMM + elementwise pass; bit-identical),
 *   "cont_pack" 0|1 (fq3_prefill_continue_batch: the attention of the whole pack in one launch per layer; 0 = per prompt).
 * Resets a captured graph. */
int fq3_set_option(fq3_ctx* ctx, const char* key, int value);

/* Replaces the module references the graph objects keep (predictor_graph.py:52-58, talker_graph.py:40).
 * Round 6: for a bf16 context the call also takes a reference on a FRAGMENT-MAJOR copy of every layer matrix and head whose shape the
 * weight-stationary GEMM serves (K in {1024, 2048, 3072, 6144}, whole 16-row blocks): [row block][K / 32][64 lanes][8] -- the kilobyte one
 * wave's matrix-core operand load reads is contiguous (from the row-major matrix it is 16 rows x 64 B: 40 GB/s per CU against 125-135
 * out of the L2).  The first context of a weight replica builds the copies (+ one replica's layer matrices of HBM, gate | up in two blockings: 1.5 GB
 * at 0.6B, 3.9 GB at 1.7B), the others share them; fq3_ctx_destroy / a re-bind returns the references.  The table's matrices must not change
 * while bound (re-bind after an in-place update). */
int fq3_bind_weights(fq3_ctx* ctx, const fq3_weight_table* table);

/* ---- talker -------------------------------------------------------------------------------- */

/* TalkerGraph.prefill_kv (talker_graph.py:153-170): copy one layer of an externally computed prefill
 * cache, k and v laid out [n_kv_heads, L, head_dim] (the HF [1, kvh, L, d] tensor), into static slots
 * [0, L).  FQ3_ETOOLONG if L > max_seq_len (the reference raises RuntimeError, :163-167). */
int fq3_kv_import(fq3_ctx* ctx, int layer, const void* k, const void* v, int L, void* stream);
/* Test hook: copy static KV slots [0, L) of one layer back out in the same layout. */
int fq3_kv_export(fq3_ctx* ctx, int layer, void* k, void* v, int L, void* stream);
/* `dst` takes over the KV rows [0, L) of every talker layer from `src`.  Contexts of ONE pool: a block-table hand-over -- dst
 * returns its own blocks, receives src's block ids (one tiny launch rewrites its device table) and src is left empty; no KV row
 * moves.  Contexts of different pools (or private ones): the rows are copied block by block in one launch and src keeps its
 * blocks.  No reference equivalent: it lets a server prefill the next request into a spare context while the lock-step batch
 * keeps decoding, and hand the result to whichever lane frees up (fq3hip/batching.py).  FQ3_ETOOLONG if L > dst's max_seq_len. */
int fq3_kv_adopt(fq3_ctx* dst, fq3_ctx* src, int L, void* stream);

/* dst receives a COPY of K/V rows [0, L) of every talker layer (whole 64-key blocks, one launch); src keeps its blocks, whether
 * or not the two contexts share a pool.  dst takes the blocks it needs (FQ3_ENOMEM and nothing taken when its pool is short). */
int fq3_kv_copy(fq3_ctx* dst, fq3_ctx* src, int L, void* stream);

/* TalkerGraph.set_generation_state (talker_graph.py:172-196): left-pad count of the prompt mask and
 * the rope delta; replaces the 2048-row additive mask table with two integers. */
int fq3_set_generation_state(fq3_ctx* ctx, int n_pad, int rope_delta);

/* TalkerGraph.run (talker_graph.py:198-214): one token through all talker layers + final norm.
 * embeds T[H]; position = static cache slot; out_hidden T[H] (post-norm). */
int fq3_talker_step(fq3_ctx* ctx, const void* embeds, int position, void* out_hidden, void* stream);

/* Prefill (generate.py:107-122): L prompt embeddings T[L,H] through the talker, KV written to slots
 * [0,L); outputs last-position logits T[V] and post-norm hidden T[H].  n_pad = left padding. */
int fq3_prefill(fq3_ctx* ctx, const void* embeds, int L, int n_pad, void* out_logits, void* out_hidden,
                void* stream);
/* Rows [start, start + n) of a prompt whose rows [0, start) are already in this context's cache (written by fq3_prefill,
 * fq3_prefill_continue, fq3_kv_copy, fq3_kv_adopt or fq3_kv_import, without left padding): embeds T[n, H] are the NEW rows only;
 * K/V of the new rows go to slots [start, start + n); row start + t attends to keys 0 .. start + t.  Outputs as fq3_prefill
 * (last new row).  Sets the generation state to (n_pad 0, rope_delta 0) like fq3_prefill does for an unpadded prompt.
 * start == 0 is a whole prefill through the continuation kernels.  FQ3_ESTATE when the context owns fewer than ceil(start / 64)
 * blocks, FQ3_ETOOLONG when start + n > max_seq_len.  bf16: the attention splits the keys of a query block over several
 * workgroups and merges them in a second launch, in a fixed order: the same call gives the same bits. */
int fq3_prefill_continue(fq3_ctx* ctx, const void* embeds, int start, int n, void* out_logits, void* out_hidden, void* stream);
/* The same prefill for n prompts with ONE pass over the weights: row-wise work (norms, GEMMs, SwiGLU) on the packed rows of
 * all prompts, q/k norm + RoPE + KV write and causal attention per prompt into ctxs[q]'s own cache.  ctxs must share one
 * weight table; workspaces are ctxs[0]'s (sum of L <= its max_seq_len) -- otherwise this is n fq3_prefill calls.  No
 * reference equivalent (its prefill is one upstream forward per request, generate.py:107-118); used when a lock-step batch
 * admits several requests at once.  out_logits may be null, or hold nulls. */
int fq3_prefill_batch(fq3_ctx* const* ctxs, int n, const void* const* embeds, const int* L, const int* n_pad,
                      void* const* out_logits, void* const* out_hidden, void* stream);

/* fq3_prefill_continue for n prompts with ONE pass over the weights: embeds[q] T[cnt[q], H] are the NEW rows of prompt q, whose rows
 * [0, start[q]) are already in ctxs[q]'s cache; K/V go to slots [start[q], start[q] + cnt[q]), row start[q] + t attends to keys
 * 0 .. start[q] + t, outputs come from each prompt's last new row.  Packing as fq3_prefill_batch: row-wise work on the packed new rows
 * on ctxs[0]'s workspace (sum of cnt <= its max_seq_len), one weight table, n <= 64.  bf16 with contexts of one pool: one norm + RoPE +
 * K/V launch and one flash attention launch per layer for the whole pack (+ one merge launch when a sequence splits its keys; fixed
 * order, the same call gives the same bits); otherwise per-prompt launches of the fq3_prefill_continue kernels ("cont_pack" 0 forces
 * them).  All-or-nothing, checked before anything is queued: FQ3_EINVAL (n < 1, n > 64, cnt < 1, start < 0, mixed weight tables or
 * dtypes), FQ3_ESTATE (a context owns fewer than ceil(start / 64) blocks), FQ3_ETOOLONG (start + cnt > max_seq_len, or the packed rows
 * exceed the workspace), FQ3_ENOMEM (pool short: nothing taken).  Sets each context's generation state to (n_pad 0, rope_delta 0). */
int fq3_prefill_continue_batch(fq3_ctx* const* ctxs, int n, const void* const* embeds, const int* start, const int* cnt,
                               void* const* out_logits, void* const* out_hidden, void* stream);

/* Allocate the matrix-core prefill's activation workspace of this context now (max_seq_len rows; otherwise it is allocated by
 * the first fq3_prefill / fq3_prefill_batch that leads with this context).  A scheduler that prefills into spare contexts on a
 * side stream while lock-step lanes decode calls this when it is built, so that no device allocation happens under the decode. */
int fq3_prefill_reserve(fq3_ctx* ctx);

/* Test hook: 0 = matrix-core prefill (default), 1 = walk the prompt token by token through the decode kernels. */
int fq3_set_prefill_mode(fq3_ctx* ctx, int mode);

/* talker.codec_head (generate.py:182): logits T[V] = codec_head(hidden T[H]) (hidden is post-norm). */
int fq3_codec_head(fq3_ctx* ctx, const void* hidden, void* out_logits, void* stream);

/* ---- predictor ----------------------------------------------------------------------------- */

/* Construction-time predictor sampling policy (model.py:209-218, predictor_graph.py:47-50). */
int fq3_set_predictor_sampling(fq3_ctx* ctx, const fq3_sampling* s);

/* PredictorGraph.run (predictor_graph.py:204-214 = _full_loop :115-167): pred_input T[2,H_talker];
 * noise T[15, Vp] of Exp(1) variates or NULL when greedy; out_ids int64[15]; optional out_logits
 * T[15, Vp] (may be NULL) for parity tests. */
int fq3_predictor_loop(fq3_ctx* ctx, const void* pred_input, const void* noise, int64_t* out_ids,
                       void* out_logits, void* stream);

/* ---- sampler ------------------------------------------------------------------------------- */

/* sample_logits + apply_repetition_penalty (sampling.py:10-66): logits T[V] (not modified);
 * history int64[n_hist] of previous first-codebook ids (may be NULL); suppress range [sup_lo, sup_hi)
 * except keep_id (generate.py:46-50), plus eos when suppress_eos (generate.py:125,188);
 * noise T[V] Exp(1) (NULL when !do_sample); out_token int64[1]. */
int fq3_sample(fq3_ctx* ctx, const void* logits, int V, const fq3_sampling* s, const int64_t* history,
               int n_hist, int sup_lo, int sup_hi, int keep_id, int suppress_eos, const void* noise,
               int64_t* out_token, void* stream);

/* apply_repetition_penalty (sampling.py:10-29) alone, in place on logits T[V]: ids in history get x/p (x > 0) or x*p. */
int fq3_apply_repetition_penalty(fq3_ctx* ctx, void* logits, int V, const int64_t* history, int n_hist, float penalty,
                                 void* stream);

/* ---- fused on-device decode loop (generate.py:149-199 / streaming.py:106-154) -------------- */

typedef struct fq3_decode_params {
    fq3_sampling talker;         /* per-call sampling arguments */
    int32_t min_new_tokens;
    int32_t max_new_tokens;
    int32_t prefill_len;         /* talker_graph.prefill_kv return value */
    int32_t gen_step;            /* out.generation_step of the prefill (generate.py:122) */
    int32_t first_token;         /* token sampled from the prefill logits (generate.py:124-134) */
    const void* past_hidden;     /* T[H]: out.past_hidden (generate.py:121) */
    const void* trailing_text;   /* T[trailing_len, H] (generate.py:168-169) */
    int32_t trailing_len;
    const void* tts_pad_embed;   /* T[H] (generate.py:171) */
    const void* talker_noise;    /* T[noise_frames, V] or NULL */
    const void* pred_noise;      /* T[noise_frames, 15, Vp] or NULL */
    int32_t noise_frames;        /* rows in the noise rings; frame f reads row f % noise_frames */
} fq3_decode_params;

/* Arms the on-device loop state (token, position, history bitmap, counters).  Asynchronous: `p` is consumed before
 * the call returns, the buffers it points to must stay alive until the loop has finished. */
int fq3_decode_begin(fq3_ctx* ctx, const fq3_decode_params* p, void* stream);
/* Stops the loop of this context at the next frame boundary (the device state is marked done: further frames are no-ops, in a
 * lock-step batch the lane idles).  For a scheduler that abandons an utterance half way (a streaming consumer that went away):
 * without it the lane would keep decoding to its own EOS / max_new_tokens.  Asynchronous. */
int fq3_decode_cancel(fq3_ctx* ctx, void* stream);
/* Parity-test hook (teacher forcing; the shape of the reference's own relation tests, tests/test_e2e_parity.py:414-427,
 * applied decision by decision): after fq3_decode_begin, every sampler of the loop records ITS OWN id in
 * decisions[f][j] and continues with forced_codes[f][j] instead (both device int32[n_frames + 1][16]: [f][0] = the
 * first-codebook id of frame f, [f][1 + cb] = predictor codebook cb).  NULL, NULL switches it off. */
int fq3_decode_set_forced(fq3_ctx* ctx, const int32_t* forced_codes, int32_t* decisions, void* stream);
/* Enqueue n_frames iterations of the loop body; each is one hipGraph replay once
 * fq3_graph_capture() has run (talker_graph.py:109-147, predictor_graph.py:169-202), otherwise the
 * same kernels are launched directly.  Frames after EOS / limits are no-ops on device. */
int fq3_decode_frames(fq3_ctx* ctx, int n_frames, void* stream);
/* Synchronises the stream and reports: frames emitted so far, done flag (0 running, 1 finished; 2 = held: the loop has an open
 * text table -- fq3_decode_text_open -- and the next frame's text row has not been appended; it goes on once it has); copies codes
 * int64[n, 16] for frames [from, n_frames_total) into out_codes (host or device memory visible to host). */
int fq3_decode_poll(fq3_ctx* ctx, int* n_frames_total, int* done, void* stream);
int fq3_decode_codes(fq3_ctx* ctx, int from, int count, int64_t* out_codes_dev, void* stream);
/* Capture the loop body into a hipGraph (no-op if already captured). */
int fq3_graph_capture(fq3_ctx* ctx, void* stream);
int fq3_graph_reset(fq3_ctx* ctx);

/* ---- prompt builder (model.py:583-805 _build_talker_inputs_local and upstream generate_icl_prompt) -------------------
 * Every row of the talker prompt is  text_projection(text_embedding(id))  +  a codec-stream row  (either may be absent):
 * the text rows come from one batched MLP on the matrix cores, the codec rows are embedding gathers / the speaker
 * embedding / the 16-way embedding sum of one reference frame, and ONE kernel assembles all rows from a small row program
 * the host derives from the token ids (which segment goes where is control flow, not arithmetic). */
typedef struct fq3_prompt_weights {
    const void* text_embedding;   /* [text_vocab, text_hidden]   talker.get_text_embeddings(), model.py:605 */
    const void* fc1_w;            /* [text_hidden, text_hidden]  talker.text_projection.linear_fc1 */
    const void* fc1_b;            /* [text_hidden] */
    const void* fc2_w;            /* [H, text_hidden]            talker.text_projection.linear_fc2 */
    const void* fc2_b;            /* [H] */
    int32_t text_vocab, text_hidden;
} fq3_prompt_weights;
int fq3_bind_prompt_weights(fq3_ctx* ctx, const fq3_prompt_weights* w);
/* out T[n, H] = text_projection(text_embedding(ids int64[n]))  (fc1 -> SiLU -> fc2, one rounding per module output). */
int fq3_text_project(fq3_ctx* ctx, const int64_t* ids, int n, void* out, void* stream);
/* Assemble n_rows prompt rows.  prog int32[n_rows][3] = {text_row, kind, arg}: text_row indexes text_rows T[n_text, H]
 * (-1: no text part); kind 0 no codec part, 1 codec_embedding[arg], 2 the speaker embedding spk_embed T[H],
 * 3 the sum over the 16 codebook embeddings of reference frame arg (ref_codes int64[n_ref, 16], model.py:699-712).
 * out[r] = text part + codec part (one rounding), or the single part that is present, or zeros where neither is.
 * prog is read on the device, so a row cannot be refused: a row of kind 3 when ref_codes is null or n_ref <= 0, a row of
 * kind 2 when spk_embed is null, and a row of any other kind have no codec part (nothing is read for it). */
int fq3_prompt_rows(fq3_ctx* ctx, const void* text_rows, int n_text, const int32_t* prog, int n_rows,
                    const int64_t* ref_codes, int n_ref, const void* spk_embed, void* out, void* stream);

/* ---- incremental text: the loop's text table grows while it decodes --------------------------------------------------
 * In the step-by-step layout frame g adds row g of the trailing table to the talker's input, and a row is a function of its
 * token id alone, so frame g needs text token g + 1 and nothing later.  An open table lets the rows arrive while the loop runs;
 * a frame whose row has not been published yet leaves the loop untouched (fq3_decode_poll / fq3_batch_poll_wait report done = 2
 * for such a loop) and the next frame queued after the append goes on from the same state: the codes are those of the whole table.
 *
 * After fq3_decode_begin: the loop's text table becomes an open table of `capacity_rows` rows owned by the context; the
 * rows fq3_decode_begin was given (possibly none) are copied in.  FQ3_ESTATE without prompt weights or before begin. */
int fq3_decode_text_open(fq3_ctx* ctx, int capacity_rows, void* stream);
/* ids int64[n] on the device -> n more rows (text_projection(text_embedding(id))), published in stream order.
 * final != 0 closes the table (the caller's last id is tts_eos: prompt.py:125); n == 0 is allowed with final.
 * FQ3_EINVAL past the capacity (nothing is written), FQ3_ESTATE when the table is not open. */
int fq3_decode_text_append(fq3_ctx* ctx, const int64_t* ids, int n, int final, void* stream);
/* rows appended so far / whether the table is closed (host-side bookkeeping, no device round trip) */
int fq3_decode_text_rows(const fq3_ctx* ctx, int* n_rows, int* closed);
/* copies rows [from, from + count) of the table, T[count, H], to `out` on the device in stream order (tests and tools that
 * compare rows; the loop reads the table through its own state).  FQ3_EINVAL beyond the rows appended so far. */
int fq3_decode_text_read(fq3_ctx* ctx, int from, int count, void* out, void* stream);

/* ---- batched decode: B utterances in lock-step over one weight stream ------------------------------
 * No reference equivalent (the reference fixes batch = 1: talker_graph.py:46, predictor_graph.py:70; SURVEY.md
 * section 8f rank 3).  A batch borrows n_lanes (1..128) ordinary contexts that share ONE weight table, ONE config and
 * ONE max_seq_len.  Each lane is prepared with the single-stream entry points (fq3_prefill, fq3_set_generation_state,
 * fq3_decode_begin) and read back with fq3_decode_poll / fq3_decode_codes on ITS context; fq3_batch_frames replaces
 * fq3_decode_frames for all lanes at once.  Lanes that are done (EOS, limits, or never begun) idle on device and can be
 * re-armed with fq3_decode_begin between calls (continuous batching).  Every lane samples with its own policy (the one
 * its fq3_decode_begin / fq3_set_predictor_sampling set): top_p < 1 (sampling.py:57-65) is honoured per lane inside the
 * same launch.  With the VALU GEMVs ("mfma" 0, the fp32 default) a lane's ids are bit-identical to the same utterance
 * decoded alone with the same noise; the bf16 default multiplies one 16-column token tile per v_mfma_f32_16x16x32_bf16,
 * so 9..16 lanes read the weights once and issue the MFMAs of 1..8; lanes 17..32, 33..48, ... 113..128 are further token tiles
 * of the same launch over the register-resident weight fragments. */
typedef struct fq3_batch fq3_batch;
int fq3_batch_create(fq3_ctx* const* lanes, int n_lanes, fq3_batch** out);
int fq3_batch_destroy(fq3_batch* b);
int fq3_batch_size(const fq3_batch* b);
/* Enqueue n_frames lock-step iterations (hipGraph replays once fq3_batch_graph_capture() has run). */
int fq3_batch_frames(fq3_batch* b, int n_frames, void* stream);
int fq3_batch_graph_capture(fq3_batch* b, void* stream);
int fq3_batch_graph_reset(fq3_batch* b);
/* Every lane's fq3_decode_poll in one go, split in two so that a scheduler can keep the GPU fed: fq3_batch_poll_async enqueues ONE
 * gather launch + ONE small copy on `stream` (in stream order: it sees the frames queued before it) into slot 0..3;
 * fq3_batch_poll_wait blocks until that slot's copy has landed and fills n_frames_total[fq3_batch_size] / done[fq3_batch_size]
 * (either may be NULL).  Frames queued AFTER the poll run while the host waits for and digests it.  FQ3_ESTATE: nothing was queued
 * in the slot. */
int fq3_batch_poll_async(fq3_batch* b, int slot, void* stream);
int fq3_batch_poll_wait(fq3_batch* b, int slot, int* n_frames_total, int* done);
/* fq3_decode_text_append for many lanes in one call.  n_items (lane, count, final) triples on the host; ids int64[sum(count)] on the
 * device, packed in item order.  For every item: `count` more rows of that lane's open table (fq3_decode_text_open on the lane's
 * context), final != 0 closes it; count == 0 is allowed with final.  All ids are projected by ONE gather, ONE fc1 + SiLU and ONE
 * fc2 GEMM, one launch scatters the rows to the lanes' tables and one publishes the new lengths in stream order: five launches
 * whatever the number of lanes.  The rows are bit-identical to fq3_text_project of the same ids.
 * All or nothing, checked before anything is queued: FQ3_EINVAL for a lane index out of range or named twice, a negative count or
 * an item with neither ids nor final, and for an item past its lane's capacity; FQ3_ESTATE for a lane whose table is not open.
 * On error no lane's rows, row count or open flag change. */
int fq3_batch_text_append(fq3_batch* b, int n_items, const int32_t* lane, const int32_t* count, const int32_t* final_,
                          const int64_t* ids, void* stream);
/* "mfma" 0|1: batch GEMVs on the matrix cores (bf16 contexts; default 1: ids checked against the oracle by teacher
 * forcing) or on the VALU kernels (0: every lane bit-identical to the same utterance decoded alone).
 * "skinny" 0|1 (with "mfma" 1, more than 16 lanes): o_proj / down through the weight-stationary kernel of the short-prompt prefill
 * (default 1) or through the one-row-block-per-workgroup batch GEMV (0); 2 takes the weight-stationary kernel at every lane count
 * (measurement switch).
 * "norm_skinny" 0|1 (more than 32 lanes): the normalising GEMVs (qkv, gate | up, heads) as ONE normalisation launch + the
 * weight-stationary GEMM kernel (default 1) or as the per-workgroup-panel kernels of the lower lane counts (0);
 * "norm_skinny_above" n moves that lane count (measurement switch).
 * Round 5: "attn_lane" 0|1|2 -- the talker attention as ONE workgroup per (kv head, lane) that writes the final head outputs (no
 * partial slots, no merge launch): never | from "attn_lane_from" lanes on (default 64; bf16 matrix-core path) | always; "attn_lane_keys"
 * 8|16 (keys per load step); "pred_pair" 0|1 -- the predictor's two-token prefill as one pass over 2 B token rows where that is
 * bit-identical (above 32 lanes; default 1); "norm_fused" 0|1 -- the RMSNorm of qkv / gate | up / lm heads inside the
 * weight-stationary GEMM, from sum-of-squares partials the residual GEMM's epilogue leaves (measured SLOWER on MI355X: default 0).
 * Round 6: "pred_attn_group" 0|1 -- the code predictor's attention as one wave per (kv group, lane) that serves the group's q heads from
 * one read of the LIVE K / V rows (default 1; bit-identical) or as one wave per (q head, lane) over all 16 slots (0).
 * "packed_weights" 0|1 -- the weight-stationary GEMMs read the fragment-major copies fq3_bind_weights keeps of the bf16 layer matrices
 * (default 1; bit-identical) or the row-major matrices (0).
 * "groups" 0..4: LANE GROUPS (a measurement switch).  The lanes split into that many independent lock-step chains of whole 16-lane
 * tiles, each with its own frame graph, advanced concurrently on streams the library probes for a hardware queue of their own (they
 * fork from / join `stream` inside fq3_batch_frames, so the caller sees one stream as before); 0 (default) = automatic = ONE chain:
 * measured on MI355X, two concurrent chains of 32 lanes take 7.15 ms per frame where one chain of 64 takes 5.57 ms.  A lane's values
 * do not depend on the grouping.  When no stream with its own queue is found, or `stream` is being captured, the chains run one
 * after another on `stream`. */
int fq3_batch_set_option(fq3_batch* b, const char* key, int value);
/* The caller's own side streams for lane groups 1..n (n <= 3), e.g. streams it has probed against every other stream it keeps
 * busy (a vocoder stream, a prefill stream); they are borrowed, not owned.  n = 0 returns to the library's own probing. */
int fq3_batch_set_group_streams(fq3_batch* b, void* const* streams, int n);

/* ---- 12 Hz codec decoder (speech_tokenizer.decode, model.py:924) ---------------------------- */
typedef struct fq3_codec fq3_codec;
typedef struct fq3_codec_config {
    int32_t dtype;              /* FQ3_BF16: the checkpoint dtype, what the reference's Torch path runs (PCM ~8e-3 RMS from an fp32 evaluation on a
                                 * trained-vocoder-like network).  FQ3_F32: fp32 weights (a bf16 checkpoint widened exactly), activations and
                                 * v_mfma_f32_16x16x4_f32 products: ~1e-6 RMS, ~4x the time.  FQ3_BF16X2: the high-precision mode for serving --
                                 * weights stay bf16 (bound with every K column DUPLICATED: [N][taps][2 Cin]), every activation and
                                 * per-channel vector is a 32-bit word (bf16 hi | bf16 lo << 16; bind those as such), a GEMM reads the
                                 * activation tensor as a [rows][2 Cin] bf16 matrix and issues two bf16 MFMAs per K pair: <= 1e-3 PCM RMS
                                 * (north star) at about twice the bf16 time */
    int32_t codebook_size, codebook_dim, rvq_dim, num_quantizers, num_semantic;
    int32_t latent_dim, hidden, inter, n_layers, n_heads, head_dim, sliding_window;
    float rms_eps;
    int32_t n_upsample;  int32_t upsampling_ratios[4];
    int32_t n_rates;     int32_t upsample_rates[8];
    int32_t decoder_dim;
    int32_t max_frames;
} fq3_codec_config;
int fq3_codec_create(const fq3_codec_config* cfg, fq3_codec** out);
int fq3_codec_destroy(fq3_codec* c);
/* name -> device pointer binding; names are the checkpoint tensor names under "decoder." */
int fq3_codec_bind(fq3_codec* c, const char* name, const void* ptr, int64_t numel);
/* Kernel-variant switch of the codec decoder (parity tests / measurements): "fuse_units" 1 = the residual units of the
 * 96-channel decoder block (SnakeBeta -> k7 conv -> SnakeBeta -> 1x1 conv -> + skip) run as ONE launch each with the middle
 * tensor kept in LDS (the default: 7.45 vs 7.92 ms per 370-frame decode), 2 = the 192-channel block's too (measured slower:
 * 7.93 ms), 0 = two GEMM launches per unit.  All settings give bit-identical waveforms.  FQ3_BF16X2 (round 5): the 96-channel block's
 * units fuse too (the middle tensor parked in LDS as hi | lo words); measured a wash (14.46 -> 14.31 ms per 370-frame decode).
 * "glds_cap8" n (round 6, measurement hook): FQ3_BF16X2 GEMMs take the eight-wave LDS-DMA tiles up to n tiles of 128 x 64 (0 = the
 * launcher's default: whatever the grid); bit-identical.
 * The four activation workspaces follow the CALL: a batched decode needs B x elems(T) elements and grows them when short
 * (FQ3_ENOMEM when that fails: the Python host then decodes utterance by utterance). */
int fq3_codec_set_option(fq3_codec* codec, const char* key, int value);
int fq3_codec_finalize(fq3_codec* c, void* stream);
/* number of PCM samples produced for T frames (the causal transposed convs trim, so < 1920*T) */
int64_t fq3_codec_num_samples(const fq3_codec* c, int T);
/* codes int64[T,16] (device) -> pcm float32[num_samples] (device), clamped to [-1,1]. */
int fq3_codec_decode(fq3_codec* c, const int64_t* codes, int T, float* pcm, void* stream);
/* The same decode, but only PCM samples [first_sample, num_samples(T)) are produced, into pcm[0 ..): what the streaming
 * call sites keep of each re-decode (model.py:1095-1100 `audio[cut:][prev_len:]`, :1128-1133 `audio[ctx_samples:]`).
 * The decoder is causal with a bounded receptive field after its transformer, so only the rows those samples depend on are
 * recomputed; the values are bit-identical to the corresponding tail of fq3_codec_decode's output. */
int fq3_codec_decode_tail(fq3_codec* c, const int64_t* codes, int T, int64_t first_sample, float* pcm, void* stream);
/* The batched form of the vocoder interface (speech_tokenizer.decode takes audio_codes [B, T, 16], model.py:924; payload shape pinned
 * by the reference's tests/test_sample_rate.py:53-75): codes int64[B][T][16] (device), B utterances of T frames each, decoded by ONE
 * set of launches -- every tensor is [utterance][rows][C], every launch carries the utterance in a grid dimension, so the
 * latency-bound frame-level transformer and the skinny convs of short inputs fill the chip B times better.  pcm
 * float32[B][num_samples(T) - first_sample]: per utterance exactly (bit for bit) what fq3_codec_decode_tail(codes[b], T,
 * first_sample) produces.  Utterances of different lengths: pad the shorter ones with any valid ids -- the decoder is causal, a
 * prefix of the codes gives the same prefix of the waveform -- and keep num_samples(T_b) samples of each.  The workspace grows to
 * B utterances on first use (a device synchronisation; not inside a graph capture). */
int fq3_codec_decode_batch(fq3_codec* c, const int64_t* codes, int B, int T, int64_t first_sample, float* pcm, void* stream);
/* Reference-prefix state (round 6).  The ICL call sites decode `ref_codes + generated codes` and cut the reference part off
 * (model.py:919-937; every phase-1 chunk of the streaming path again, model.py:1085-1115): the frame-level front end -- RVQ sums,
 * pre_conv, the sliding-window transformer -- re-runs over the same reference frames for every chunk and every utterance of a voice.
 * fq3_codec_prefix_create runs it ONCE over ref_codes int64[ref_len][16] (device) and keeps what later rows read from the prefix: the
 * pre_conv's two context rows, every layer's post-RoPE K / V of the last sliding_window - 1 rows, the last 48 output rows (the conv
 * stack's halo).  fq3_codec_decode_batch_prefix is fq3_codec_decode_batch for codes whose first fq3_codec_prefix_frames(prefix) frames
 * of utterance b ARE that prefix's codes (prefixes: HOST array of B states of one length, B <= 128; the same state may repeat): the
 * front end computes rows [ref_len, T) only.  The waveform is bit-identical to the full decode's (the front end is causal and a row's
 * arithmetic does not depend on the row count); a first_sample that reaches further back than the cached rows silently takes the full
 * path.  A state belongs to the codec that made it and must be destroyed before it. */
typedef struct fq3_codec_prefix fq3_codec_prefix;
int fq3_codec_prefix_create(fq3_codec* c, const int64_t* ref_codes, int ref_len, fq3_codec_prefix** out, void* stream);
int fq3_codec_prefix_destroy(fq3_codec_prefix* prefix);
int fq3_codec_prefix_frames(const fq3_codec_prefix* prefix);
int fq3_codec_decode_batch_prefix(fq3_codec* c, const fq3_codec_prefix* const* prefixes, const int64_t* codes, int B, int T,
                                  int64_t first_sample, float* pcm, void* stream);
/* Rolling stream state: the prefix state moved forward with every chunk.  One state per utterance keeps what
 * later rows read of earlier ones -- the pre_conv's 2 context rows, every layer's post-RoPE K / V of the last sliding_window - 1 rows,
 * the last 48 front-end output rows.  The samples a stream has produced after ANY sequence of pushes are, bit for bit,
 * fq3_codec_decode(all codes, F)[num_samples(F0):] (F0 = the prefix it began behind, whose codes go in front): for every split of the
 * frames into pushes, for B = 1 or many, in all three precisions.  A push is the decode behind a prefix in LOCAL rows -- [0, ctx) the
 * cached rows, ctx = min(F, ctx_max), ctx_max = max(sliding_window - 1, 48), then the n_new new ones -- so its workspaces are those of
 * ctx_max + n_new frames however long the stream is.
 *   start  NULL = an utterance that begins at frame 0; else the stream begins BEHIND that prefix (ICL reference): the state is a copy,
 *          the prefix stays shared by the voice's other streams
 *   push   B <= 128 streams (HOST array) take n_new frames each: codes int64[B][n_new][16] (device) hold the NEW frames only; pcm
 *          float32[B][n_out], n_out = num_samples(F + n_new) - num_samples(F) (num_samples(0) = 0).  The lanes of one call may stand at
 *          different positions F but must share n_new and min(F, ctx_max), and a state may appear once: else FQ3_EINVAL.  Positions index
 *          the RoPE tables bound as "rope.stream_cos" / "rope.stream_sin" (fp32 [rows][head_dim / 2], rows of their own choosing; FQ3_ESTATE
 *          when not bound): a push that would pass them returns FQ3_ETOOLONG.  There is no full path to fall back to: a decoder whose
 *          conv stack reaches further back than the cached rows gets FQ3_EUNSUPPORTED.  Every such refusal leaves the states untouched.  A push
 *          that fails after its first launch leaves its streams unusable: FQ3_ESTATE until fq3_codec_stream_reset.
 * A state belongs to the codec that made it and must be destroyed before it. */
typedef struct fq3_codec_stream fq3_codec_stream;
int fq3_codec_stream_create(fq3_codec* c, const fq3_codec_prefix* start, fq3_codec_stream** out, void* stream);
int fq3_codec_stream_reset(fq3_codec_stream* s, const fq3_codec_prefix* start, void* stream);
int fq3_codec_stream_destroy(fq3_codec_stream* s);                 /* NULL -> 0 */
int fq3_codec_stream_frames(const fq3_codec_stream* s);            /* F: frames absorbed so far, the prefix included */
int fq3_codec_stream_push(fq3_codec* c, fq3_codec_stream* const* streams, int B, const int64_t* codes, int n_new,
                          float* pcm, void* stream);

/* ---- reference-audio analysis (create_voice_clone_prompt, model.py:415-463 -> upstream qwen_tts) -----------------------
 * What the reference runs once per new (ref_audio, ref_text) pair and then caches (model.py:424-463):
 *   speech_tokenizer.encode(ref_wav)  -> ref_code  int64 [T, 16]   (the 12.5 Hz tokenizer's ENCODER: SEANet conv stack,
 *       8-layer causal transformer, stride-2 conv, split residual VQ -- the Mimi architecture, transformers
 *       models/mimi/modeling_mimi.py:450-492, :782-928, :1030-1138, :1231-1268)
 *   extract_speaker_embedding(wav)    -> ref_spk_embedding [enc_dim] (log-mel front end + ECAPA-TDNN, transformers
 *       models/qwen2_5_omni/modeling_qwen2_5_omni.py:2412-2707 is the readable sibling)
 * fp32 only; either half may be left unbound.  Weight names are the checkpoint names under "encoder." / "speaker_encoder."
 * in the layouts fq3hip/refenc.py packs (documented in csrc/fq3_refenc.hip). */
typedef struct fq3_refenc fq3_refenc;
typedef struct fq3_refenc_config {
    /* speech-tokenizer encoder */
    int32_t num_filters;                     /* 64 */
    int32_t n_ratios; int32_t ratios[8];     /* strides in encoder order (4, 5, 6, 8) */
    int32_t kernel_size, last_kernel_size, residual_kernel_size, n_residual_layers, dilation_growth_rate, compress;   /* 7 3 3 1 2 2 */
    int32_t hidden, n_layers, n_heads, head_dim, inter, sliding_window;     /* 512 8 8 64 2048 250 */
    float   norm_eps;                        /* 1e-5 */
    int32_t num_quantizers, num_semantic, codebook_size, codebook_dim;      /* 16 1 2048 256 */
    int32_t max_positions;                   /* rows of the "encoder.rope.cos/sin" tables (25 Hz frames) */
    /* speaker encoder */
    int32_t mel_dim, n_fft, hop, n_bins_padded;   /* 128 1024 256 544 (n_fft/2 + 1 rounded up to a multiple of 32) */
    int32_t n_enc; int32_t enc_channels[8], enc_kernel_sizes[8], enc_dilations[8];   /* 5: 512 512 512 512 1536 / 5 3 3 3 1 / 1 2 3 4 1 */
    int32_t attn_channels, res2net_scale, se_channels, enc_dim;             /* 128 8 128 1024|2048 */
} fq3_refenc_config;
int fq3_refenc_create(const fq3_refenc_config* cfg, fq3_refenc** out);
int fq3_refenc_destroy(fq3_refenc* r);
int fq3_refenc_bind(fq3_refenc* r, const char* name, const void* ptr, int64_t numel);
int fq3_refenc_finalize(fq3_refenc* r, void* stream);
/* number of 12.5 Hz frames the encoder produces for n_samples of 24 kHz audio (MimiModel.get_encoded_length, :1270-1284) */
int64_t fq3_refenc_num_frames(const fq3_refenc* r, int64_t n_samples);
/* pcm float32[n] (device, 24 kHz mono) -> codes int64[num_frames][num_quantizers] (device) */
int fq3_refenc_encode(fq3_refenc* r, const float* pcm, int64_t n, int64_t* codes, void* stream);
/* pcm float32[n] (device, 24 kHz mono) -> embed float32[enc_dim] (device); mel (optional, may be null) receives the
 * log-mel frames float32[n / hop][mel_dim] the encoder consumed */
int fq3_refenc_speaker(fq3_refenc* r, const float* pcm, int64_t n, float* embed, float* mel, void* stream);

/* ---- audio output stage: resample and encode the vocoder's PCM before it leaves the device ----------------------------------
 * The vocoder writes float32 PCM at the model's rate (24 kHz).  This stage turns it, on the device and in ONE launch per chunk, into
 * what a client asked for: another sample rate (a streaming polyphase resampler) and another sample encoding (16-bit PCM, G.711
 * mu-law / A-law), so that only the encoded bytes cross to the host.  The result does not depend on how the stream was cut into
 * pushes: every output sample is computed from the same K input samples with the same fp32 operations in the same order.
 *
 * Design (host only, no HIP call): g = gcd(in_rate, out_rate), L = out_rate / g, M = in_rate / g, both at most 320 (else
 * FQ3_EINVAL).  The prototype is a Kaiser-windowed sinc (beta 8) of half length Z m, m = max(L, M), Z = zero_crossings (0: 16),
 * cutoff 0.96 / m of the up-sampled Nyquist, computed in double precision and scaled to sum L; K = ceil((2 Z m + 1) / L) taps per
 * output.  bank (may be NULL; `capacity` floats, at least L K) receives the L phase rows, row p at bank[p K .. p K + K).
 * Output n stands at input time n M / L (zero phase) and is
 *     y[n] = sum_k bank[(n M) mod L][k] * x[floor((n M + Z m) / L) - (K - 1) + k]     (x = 0 outside the stream),
 * accumulated in fp32 from 0.0f with fmaf over k = 0 .. K - 1.  L = M = 1 is the encoder alone: K = 1, bank = {1.0f}, y[n] = x[n]. */
int fq3_audio_out_design(int in_rate, int out_rate, int zero_crossings, int* L, int* M, int* K, float* bank, int64_t capacity);
/* Output samples that exist once the first n_in input samples of a stream have been pushed: an output is produced as soon as every
 * input sample it reads exists; final != 0: the stream ended there, and the count is ceil(n_in L / M) (the samples past the end are
 * zeros).  A function of the cumulative length alone, non-decreasing in it.  Negative: an FQ3_E* code. */
int64_t fq3_audio_out_count(int in_rate, int out_rate, int zero_crossings, int64_t n_in, int final);

enum { FQ3_PCM_F32 = 0,      /* float32, the value itself */
       FQ3_PCM_S16 = 1,      /* int16: y * 32768, clamped to [-32768, 32767], truncated toward zero */
       FQ3_PCM_MULAW = 2,    /* G.711 mu-law byte of that int16 */
       FQ3_PCM_ALAW = 3 };   /* G.711 A-law byte of that int16 */
typedef struct fq3_audio_out fq3_audio_out;
typedef struct fq3_audio_out_config { int in_rate, out_rate, format, zero_crossings; } fq3_audio_out_config;
/* One object per stream; it owns the bank and the history (the last K - 1 input samples) on the current device.  NULL or range errors
 * are answered before any HIP call. */
int fq3_audio_out_create(const fq3_audio_out_config* cfg, fq3_audio_out** out);
int fq3_audio_out_destroy(fq3_audio_out* a);                 /* NULL -> 0 */
/* a new utterance on the same object (nothing is enqueued; `stream` is where the next push will run) */
int fq3_audio_out_reset(fq3_audio_out* a, void* stream);
/* pcm: n_in device floats (n_in may be 0), the next samples of the stream; final != 0: the stream ends with them.
 * out: device buffer of capacity_samples OUTPUT samples (float / int16 / uint8 by format) at any alignment its element type allows.
 * *n_out = samples written: fq3_audio_out_count(total so far, final) minus what earlier pushes wrote, known before the launch;
 * above capacity_samples: FQ3_EINVAL and nothing is launched.  One launch on `stream`, no host synchronisation; pcm and out must stay
 * valid until the stream has run it.  After a final push: FQ3_ESTATE until fq3_audio_out_reset. */
int fq3_audio_out_push(fq3_audio_out* a, const float* pcm, int64_t n_in, int final, void* out, int64_t capacity_samples,
                       int64_t* n_out, void* stream);

/* ---- time-scale modification: the `speed` of a stream, applied to the vocoder's PCM on the device ---------------------------
 * WSOLA (waveform-similarity overlap-add with a plain cross-correlation search) in front of the audio output stage: the duration
 * changes by 1 / speed, the pitch stays.  ONE launch of ONE workgroup per push (the segments form a chain); the result does not
 * depend on how the stream was cut into pushes.
 *
 * Design (host only, no HIP call): P = speed_permille in [250, 4000], Hs = round(in_rate / 100) (a multiple of 16 in [16, 480], else
 * FQ3_EINVAL), N = 2 Hs, delta = Hs; window (may be NULL; `capacity` floats, at least N) receives the periodic Hann window of length
 * N, computed in double precision.  With x = 0 outside the stream, output segment s is samples [s Hs, (s + 1) Hs):
 *     a(s) = floor(s Hs P / 1000)        pos(s) = a(s) + d(s)        pos(-1) = -Hs        d(0) = 0
 *     s >= 1:  t[j] = x[pos(s-1) + Hs + j],   c(d) = sum_{j < N} x[a(s) + d + j] t[j],   d(s) = argmax over [-delta, delta],
 *              ties to the smallest d
 *     y[s Hs + j] = fmaf(w[j], x[pos(s) + j], w[j + Hs] * x[pos(s-1) + Hs + j])
 * c(d) is accumulated in fp32 as eight partial sums, each an fmaf chain from 0.0f over one eighth of j in ascending order, added in
 * ascending order: a fixed function of (d, j). */
int fq3_tsm_design(int in_rate, int speed_permille, int* N, int* Hs, int* delta, float* window, int64_t capacity);
/* Output samples that exist once the first n_in input samples of a stream have been pushed.  final != 0: the stream ended there and
 * the count is T = ceil(1000 n_in / P) (the last segment is cut to it).  Otherwise whole segments only: segment s >= 1 exists once
 * max(a(s), a(s-1) + Hs) + delta + N <= n_in (segment 0: Hs <= n_in), and never more than Hs floor(T / Hs) samples.  A function of the
 * cumulative length alone, non-decreasing in it, never above T; the look-ahead is about N + delta input samples.  Negative: an
 * FQ3_E* code. */
int64_t fq3_tsm_count(int in_rate, int speed_permille, int64_t n_in, int final);

typedef struct fq3_tsm fq3_tsm;
typedef struct fq3_tsm_config { int in_rate, speed_permille; } fq3_tsm_config;
/* One object per stream; it owns the window, the input history the next segment can still reach and d of the last emitted segment
 * (chosen on the device; the host never learns it) on the current device.  NULL or range errors are answered before any HIP call. */
int fq3_tsm_create(const fq3_tsm_config* cfg, fq3_tsm** out);
int fq3_tsm_destroy(fq3_tsm* t);                              /* NULL -> 0 */
/* a new utterance on the same object (nothing is enqueued) */
int fq3_tsm_reset(fq3_tsm* t, void* stream);
/* As fq3_audio_out_push, float32 in and out: *n_out = fq3_tsm_count(total so far, final) minus what earlier pushes wrote, known
 * before the launch; above capacity_samples: FQ3_EINVAL and nothing is launched; after a final push: FQ3_ESTATE until fq3_tsm_reset.
 * deltas (optional, device int32[deltas_capacity]) receives d(s) of every segment this push emitted (ceil(*n_out / Hs) of them;
 * more than deltas_capacity: FQ3_EINVAL, nothing launched). */
int fq3_tsm_push(fq3_tsm* t, const float* pcm, int64_t n_in, int final, float* out, int64_t capacity_samples,
                 int64_t* n_out, int32_t* deltas, int64_t deltas_capacity, void* stream);

/* ---- the two stages above for a GROUP of streams: all rows in ONE launch ------------------------------------------------------
 * For the lock-step batch, whose chunks leave the vocoder in groups.  Every array is a HOST array of B entries; row b is exactly
 *     fq3_audio_out_push(objs[b], pcm[b], n_in[b], final[b], out[b], capacity_samples[b], &n_out[b], stream)
 * (fq3_tsm_push_group: fq3_tsm_push with deltas = NULL), and all rows run in one launch on `stream`.
 *   Equality.        What row b writes, n_out[b] and the state objs[b] is left in are bit for bit those of the single push: the sample
 *                    is computed by the same device code.  Group and single pushes mix freely on one object; membership and order of a
 *                    group may change from push to push.
 *   All or nothing.  Every row is checked before any object changes (null pointers, negative lengths, capacity, FQ3_ESTATE after a
 *                    final push): on an error that row's code is returned, nothing is launched and no object has moved.
 *   Limits.          B == 0: returns 0, does nothing.  B < 0, B > FQ3_STAGE_GROUP_MAX, a null array, a null object or the same object
 *                    twice in one call: FQ3_EINVAL.  These are answered before any HIP call.
 *   Shared design.   fq3_audio_out_push_group: all objects have the same (in_rate, out_rate, format, zero_crossings) -- one bank, one
 *                    launch plan -- else FQ3_EINVAL.  fq3_tsm_push_group: the same in_rate (one window); speed_permille may differ per
 *                    row, it enters host-computed arguments only.
 *   Empty rows.      A row with nothing to do (n_in == 0, no outputs) is legal and costs a workgroup that exits.
 *   Asynchrony.      No host synchronisation and no copy: the rows' descriptors travel in the launch's argument block, and the counts
 *                    are known on the host before the launch.  pcm[b] and out[b] must stay valid until the stream has run it. */
#define FQ3_STAGE_GROUP_MAX 32
int fq3_audio_out_push_group(fq3_audio_out* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                             void* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream);
int fq3_tsm_push_group(fq3_tsm* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                       float* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream);

/* ---- FLAC output: lossless compression of the s16 samples on the device ------------------------------------------------------
 * Behind the s16 output stage: int16 device samples in, FLAC frames (device bytes) out; the 42-byte stream header is made on the
 * host.  Decoding the stream gives the s16 samples bit for bit.  The result does not depend on how the stream was cut into pushes.
 *
 * The stream: `fLaC`, one STREAMINFO block (block size, rate, mono, 16 bits, total samples or 0 = unknown, no MD5), then frames of B
 * samples -- only the last frame of a stream may be shorter -- with fixed-blocksize frame numbers, a CRC-8 over the header and a
 * CRC-16 over the frame.  B = block_size, any value in [16, 4608]; 0: 1152 above 16 kHz, else 576.  The rate needs a frame-header
 * code: 8, 16, 22.05, 24, 32, 44.1, 48, 88.2, 96 kHz, or any rate up to 65535 Hz (two more header bytes); else FQ3_EINVAL.
 * A frame holds one subframe, chosen per block of n samples by this rule:
 *   - all samples equal: CONSTANT;
 *   - else for every FIXED order o in 0 .. min(4, n - 1) and every partition order p in 0 .. 6 with n % 2^p == 0 and (n >> p) > o:
 *     per partition the Rice parameter k in 0 .. 14 that minimises count (1 + k) + sum(u >> k), u = (r << 1) ^ (r >> 31), lowest k
 *     on ties; cost = 16 o + 6 + sum over partitions of (4 + that minimum); the cheapest (o, p), ties to the lower o, then the lower p;
 *   - that cost >= 16 n: VERBATIM.
 * A frame is therefore never longer than 2 n + 18 bytes. */
typedef struct fq3_flac fq3_flac;
typedef struct fq3_flac_config { int sample_rate, block_size; } fq3_flac_config;      /* block_size 0: the default */
/* host only: the block size in force and the frame bound 2 * block + 18 */
int fq3_flac_design(int sample_rate, int block_size, int* block, int* max_frame_bytes);
/* host only: the 42 header bytes into out (capacity >= 42); total_samples in [0, 2^36), 0 = unknown (a stream in progress) */
int fq3_flac_header(int sample_rate, int block_size, int64_t total_samples, uint8_t* out, int64_t capacity);
/* frames that exist once n_in samples of a stream were pushed: floor(n_in / B); final != 0: ceil.  Negative: an FQ3_E* code */
int64_t fq3_flac_count(int sample_rate, int block_size, int64_t n_in, int final);
/* One object per stream; it owns the held-back tail (fewer than B samples), the frame counter and staging for 64 frames on the
 * current device.  NULL or range errors are answered before any HIP call. */
int fq3_flac_create(const fq3_flac_config* cfg, fq3_flac** out);
int fq3_flac_destroy(fq3_flac* f);                           /* NULL -> 0 */
/* a new utterance on the same object (nothing is enqueued) */
int fq3_flac_reset(fq3_flac* f, void* stream);
/* pcm: n_in device int16 (n_in may be 0), the next samples of the stream; final != 0: the stream ends with them.  out: device bytes
 * at any alignment.  *n_frames (host) = the frames this push completes, known before the launch; capacity_bytes below
 * *n_frames * max_frame_bytes: FQ3_EINVAL and nothing is launched.  The frames are written back to back from out[0];
 * *n_bytes_dev (a DEVICE int64, required) receives their total length.  Per 64 frames one launch pair on `stream` -- the frames are
 * encoded into the object's staging, one workgroup each, then gathered -- and no host synchronisation; pcm, out and n_bytes_dev must
 * stay valid until the stream has run them.  After a final push: FQ3_ESTATE until fq3_flac_reset. */
int fq3_flac_push(fq3_flac* f, const int16_t* pcm, int64_t n_in, int final, uint8_t* out, int64_t capacity_bytes,
                  int64_t* n_frames, int64_t* n_bytes_dev, void* stream);
/* The FLAC stage for a GROUP of streams, as fq3_audio_out_push_group / fq3_tsm_push_group above and with their conventions.  Every
 * array is a HOST array of B entries (n_bytes_dev: B pointers to DEVICE int64s); row b is exactly
 *     fq3_flac_push(objs[b], pcm[b], n_in[b], final[b], out[b], capacity_bytes[b], &n_frames[b], n_bytes_dev[b], stream)
 *   Launches.        Frames [64 r, 64 r + 64) of every row that has them are encoded in ONE launch and gathered in ONE more: a launch
 *                    pair per round r, and the usual chunk needs one round.  A launch no row needs is not made.
 *   Equality.        The bytes row b writes, n_frames[b], *n_bytes_dev[b] and the state objs[b] is left in are bit for bit those of
 *                    the single push: a frame is encoded by the same device code.  Group and single pushes mix freely on one object;
 *                    membership and order of a group may change from push to push.
 *   All or nothing.  Every row is checked before any object changes (null pointers, negative lengths, capacity below n_frames[b] *
 *                    max_frame_bytes, the 2^50-sample and 2^31-frame bounds, FQ3_ESTATE after a final push): on an error the code of
 *                    the first offending row is returned, the message names the row, nothing is launched and no object has moved.
 *   Limits.          B == 0: returns 0, does nothing.  B < 0, B > FQ3_STAGE_GROUP_MAX, a null array, a null object or the same object
 *                    twice in one call: FQ3_EINVAL.
 *   Shared design.   All objects have the same (sample_rate, block size), else FQ3_EINVAL.
 *                    These, and every check above, are answered before any HIP call.
 *   Empty rows.      A row that completes no frame costs no encode workgroup (one if it has a tail to copy) and one gather workgroup
 *                    that sets *n_bytes_dev[b] to 0.
 *   Asynchrony.      No host synchronisation and no copy: the rows' descriptors travel in the launches' argument blocks. */
int fq3_flac_push_group(fq3_flac* const* objs, int B, const int16_t* const* pcm, const int64_t* n_in, const int* final,
                        uint8_t* const* out, const int64_t* capacity_bytes, int64_t* n_frames, int64_t* const* n_bytes_dev,
                        void* stream);

/* ---- Segment join: the sentences of a long text become one PCM stream on the device ---------------------------------------------
 * In FRONT of the time-scale stage: the stream is a sequence of SEGMENTS (float32 at in_rate, the vocoder's waveforms of the pieces
 * of a long text).  Of every segment the leading and trailing silence is removed, and a pause of zeros is put behind it.  The result
 * is a pure function of the segments' samples and pauses; it does not depend on how they were cut into pushes.
 *
 * H = in_rate / 100 (in_rate a multiple of 100 in [8000, 48000]); 0 < threshold < 1; 0 <= lead_hops <= 16;
 * 0 <= tail_hops <= hold_hops <= 400.  A segment of n samples has hops h = 0 .. last = ceil(n / H) - 1 (only the last may be short).
 * active(h): some sample of hop h has fabsf(x) >= threshold (a NaN compares false; order-free, so cut independence is exact).
 *   - no active hop: the segment contributes nothing, and its pause is dropped as well;
 *   - else with a the first and b the last active hop and L = last - b the segment contributes its samples from
 *     max(0, a - lead_hops) H up to the end of hop last - R, R = min(max(0, L - tail_hops), hold_hops), copied bit for bit, and then
 *     pause_samples zeros (0.0f).  Internal silences are never touched.  There are no fades: every cut lies in a hop below the threshold.
 * hold_hops bounds the state: an inactive hop after an active one waits in a hold queue; when the queue exceeds hold_hops its oldest
 * hop is released (emitted); at the segment's end max(0, tail_hops - released of this run) hops of the queue go out and the rest is
 * dropped -- which gives R above.  The object owns at most (hold_hops + lead_hops + 1) H floats of history on the device (two
 * buffers of that size, used in turn), plus the phase, the queue length and the released count, written by ordinary stores. */
typedef struct fq3_join fq3_join;
typedef struct fq3_join_config { int in_rate; float threshold; int lead_hops, tail_hops, hold_hops; } fq3_join_config;
/* host only: the room a push of n_in samples followed by pause_samples zeros needs: n_in + (hold_hops + lead_hops + 1) H +
 * pause_samples; n_in in [0, 2^40], pause_samples in [0, 5 in_rate].  Negative: an FQ3_E* code. */
int64_t fq3_join_bound(const fq3_join_config* cfg, int64_t n_in, int64_t pause_samples);
/* One object per output stream.  NULL or range errors are answered before any HIP call. */
int fq3_join_create(const fq3_join_config* cfg, fq3_join** out);
int fq3_join_destroy(fq3_join* j);                           /* NULL -> 0 */
/* a new stream on the same object (nothing is enqueued) */
int fq3_join_reset(fq3_join* j, void* stream);
/* pcm: n_in device floats (n_in may be 0 with any `end`), the next samples of the current segment.  end: 0 the segment goes on, 1 it
 * ends with them and pause_samples zeros in [0, 5 in_rate] follow (unless the segment had no active hop), 2 the segment and the
 * stream end, no pause (pause_samples is read with end == 1 only).  out: device floats at any float alignment; capacity must be at
 * least fq3_join_bound(cfg, n_in, the pause in force), else FQ3_EINVAL.  *n_out_dev (a DEVICE int64, required) receives the number of
 * samples written from out[0]: it depends on the data, so only the device knows it.  ONE launch of one workgroup on `stream` (a
 * long push loops inside it), no host synchronisation; pcm, out and n_out_dev must stay valid until the stream has run it.  Every
 * error is answered before anything is launched or changed: the stream goes on as if the call had not been made.  After end == 2:
 * FQ3_ESTATE until fq3_join_reset. */
int fq3_join_push(fq3_join* j, const float* pcm, int64_t n_in, int end, int64_t pause_samples, float* out, int64_t capacity,
                  int64_t* n_out_dev, void* stream);
/* The join for a GROUP of streams, as fq3_audio_out_push_group / fq3_tsm_push_group / fq3_flac_push_group above and with their
 * conventions.  Every array is a HOST array of B entries (n_out_dev: B pointers to DEVICE int64s); row b is exactly
 *     fq3_join_push(objs[b], pcm[b], n_in[b], end[b], pause_samples[b], out[b], capacity[b], n_out_dev[b], stream)
 *   Launches.        ONE launch of B workgroups on `stream`, one per row: a push is a serial walk over its hops by one lane, and the
 *                    rows of different streams do not depend on each other, so they walk side by side.
 *   Equality.        The samples row b writes, *n_out_dev[b] and the state objs[b] is left in (on the device and on the host: the
 *                    partial-hop length, the fresh flag, which pending buffer is next) are bit for bit those of the single push: a
 *                    row runs the same device code.  Group and single pushes mix freely on one object; membership and order of a
 *                    group may change from push to push.
 *   All or nothing.  Every row is checked before any object changes (null pointers, lengths, end in 0..2, the pause range, capacity
 *                    against fq3_join_bound, FQ3_ESTATE after end == 2): on an error the code of the first offending row is
 *                    returned, the message names the row, nothing is launched and no object has moved.
 *   Limits.          B == 0: returns 0, does nothing.  B < 0, B > FQ3_STAGE_GROUP_MAX, a null array, a null object or the same object
 *                    twice in one call: FQ3_EINVAL, answered before any HIP call.
 *   No shared design. Each row's descriptor carries its own configuration: the objects may differ in rate, threshold and hops.
 *   Asynchrony.      No host synchronisation and no copy: the rows' descriptors travel in the launch's argument block. */
int fq3_join_push_group(fq3_join* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* end,
                        const int64_t* pause_samples, float* const* out, const int64_t* capacity,
                        int64_t* const* n_out_dev, void* stream);

/* ---- Loudness: an ITU-R BS.1770-4 meter (mono, integrated, gated), the gain to a target level, and a gain multiply ----------------
 * On the vocoder's float32 PCM: the MEASURE is taken in front of the join, time-scale and output stages; the gain is applied in front
 * of the time-scale and output stages -- in long form behind the join, whose silence decisions see unscaled samples.  Sample peak only (no true peak), no loudness
 * range, no momentary or short-term meter; the limiter is a stage of its own (below).  The measure does not depend on how the stream was cut into pushes: it is
 * built from integers.
 *
 * Design (host only, no HIP call): in_rate a multiple of 100 in [8000, 48000], target_lufs in [-40, -5], ceiling_db in [-20, 0],
 * max_gain_db in [0, 40], else FQ3_EINVAL.  H = in_rate / 10 (a hop of 100 ms).  K-weighting = two biquads designed in double by the
 * bilinear transform (the libebur128 construction; at 48 kHz it reproduces the standard's table):
 *   shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / in_rate), Vh = 10^(G / 20),
 *              Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;  b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0,
 *              a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1] (not divided by a0), a1 and a2 as above
 * coef64 / coef32 (each may be NULL; 10 values: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2) receive the design in double and
 * rounded to float32 -- the latter is what the device uses.  *abs_gate = floor(10^((-70 + 0.691) / 10) * 4 H * 2^40),
 * *target_power = 10^((target_lufs + 0.691) / 10), *ceiling = 10^(ceiling_db / 20), *max_gain = 10^(max_gain_db / 20) (any may be NULL).
 *
 * Filter: hop h is samples [h H, (h + 1) H).  Its outputs y come from running both biquads FROM ZERO STATE starting at sample
 * max(0, (h - 1) H); the outputs of that warm-up hop are discarded.  So a hop is a fixed function of at most 2 H samples.  A biquad is
 * transposed direct form II in fp32:  u = fmaf(b0, x, s1);  s1 = fmaf(-a1, u, fmaf(b1, x, s2));  s2 = fmaf(-a2, u, b2 * x);  the shelf
 * feeds the high-pass.
 * Hop energy: E_h = sum over the hop of (uint64) rint((double) min(y * y, 64.0f) * 2^40), y * y in fp32: integers, so the sum is exact
 * in any order.  Only whole hops count; a tail shorter than a hop is left out of the energies and still counts toward the peak.
 * Peak: max of fabsf(x) over the finite samples.  n_bad: the samples that are not finite; with n_bad > 0 the energies are unspecified.
 * Gating and gain (fq3_loud_finish, one launch of one workgroup):
 *   B_b = E_b + E_b+1 + E_b+2 + E_b+3, b = 0 .. n_hops - 4;   G1 = {b : B_b > abs_gate}, n1 members, S1 their exact integer sum
 *   S1d = (double) hi * 4294967296.0 + (double) lo with S1 = hi 2^32 + lo (one rounding: the correctly rounded double of S1)
 *   G2 = {b in G1 : (double) B_b * (double) (10 n1) > S1d}, n2 members, S2d formed likewise
 *   mean_power = S2d / ((double) n2 * (double) (4 H) * 2^40)
 *   g = sqrt(target_power / mean_power);  g = min(g, max_gain);  peak > 0: g = min(g, ceiling / (double) peak);  gain = (float) g
 * in IEEE double multiply, divide, sqrt, compare and convert only.  Fewer than 4 hops, an empty G1 or n_bad > 0: gain = 1.0f, valid = 0.
 * The host turns mean_power into LUFS: -0.691 + 10 log10(mean_power). */
typedef struct fq3_loud fq3_loud;
typedef struct fq3_loud_config { int in_rate; double target_lufs, ceiling_db, max_gain_db; int capacity_hops; } fq3_loud_config;
typedef struct fq3_loud_stats { double mean_power; float peak, gain; int32_t n_hops, n_abs, n_rel, n_bad, valid, reserved; } fq3_loud_stats;
int fq3_loud_design(int in_rate, double target_lufs, double ceiling_db, double max_gain_db, int* H, double* coef64, float* coef32,
                    uint64_t* abs_gate, double* target_power, double* ceiling, double* max_gain);
/* One object per stream; capacity_hops in [0, 2^20], 0: 4096 hops (about 410 s).  It owns at most 2 H - 1 samples of history (two
 * buffers, used in turn) and per hop the energy, the peak and the non-finite count, on the current device.  NULL or range errors are
 * answered before any HIP call. */
int fq3_loud_create(const fq3_loud_config* cfg, fq3_loud** out);
int fq3_loud_destroy(fq3_loud* l);                           /* NULL -> 0 */
/* a new stream on the same object (nothing is enqueued) */
int fq3_loud_reset(fq3_loud* l, void* stream);
/* pcm: n_in device floats at any float alignment (n_in may be 0), the next samples of the stream; final != 0: the stream ends with
 * them.  ONE launch on `stream` (none for an empty push that is not final), no host synchronisation; the hops this push completes are
 * written by ordinary stores.  More hops than the capacity: FQ3_ETOOLONG.  Every error is answered before anything is launched or
 * changed.  After a final push: FQ3_ESTATE until fq3_loud_reset. */
int fq3_loud_push(fq3_loud* l, const float* pcm, int64_t n_in, int final, void* stream);
/* Only after a final push (else FQ3_ESTATE): gating and gain into *stats_dev (DEVICE memory, 8-byte aligned).  May be repeated. */
int fq3_loud_finish(fq3_loud* l, fq3_loud_stats* stats_dev, void* stream);
/* for tests and probes: the energies of the hops completed so far to out_dev_u64 (device, room for `capacity` values; fewer than the
 * hops: FQ3_EINVAL), their number to *n_hops (host) */
int fq3_loud_hops(fq3_loud* l, uint64_t* out_dev_u64, int64_t capacity, int64_t* n_hops, void* stream);
/* out[i] = pcm[i] * *gain_dev, one fp32 multiply, i < n; out may equal pcm; any float alignment; n = 0 launches nothing.  gain_dev: a
 * DEVICE float, e.g. &stats_dev->gain. */
int fq3_loud_apply(const float* gain_dev, const float* pcm, int64_t n, float* out, void* stream);

/* ---- Limiter: a true-peak look-ahead limiter over the float32 PCM, for streams and one-shot -----------------------------------------
 * Float32 mono in, float32 out at the same rate, length-preserving, with a fixed latency of A + 6 samples.  Directly behind the gain
 * (fq3_loud_apply), in front of the time-scale and output stages.  Built from FIR and integer operations only: there is no serial
 * recursion, and the result does not depend on how the stream was cut into pushes, bit for bit.
 *
 * Design (host only, no HIP call; double precision, results rounded once to float32): in_rate in [8000, 48000], ceiling_db in
 * [-20, 0], c = (float) 10^(ceiling_db / 20); attack A = round(in_rate lookahead_ms / 1000) in [8, 480], hold
 * H = round(in_rate hold_ms / 1000) in [0, 1920] (round: halves away from zero, so 5 ms at 44 100 Hz is 221); else FQ3_EINVAL.
 * The detector is a 4x oversampler kept as three fractional-phase rows h_f[0 .. 11], f = 1, 2, 3: with d = (t - 5) - f / 4,
 * h_f[t] = sinc(d) I0(8 sqrt(1 - (d / 6)^2)) / I0(8) (a Kaiser window, beta 8, six taps each side), each row divided by its sum.
 * *ceiling receives c, rows (36 floats: h_1, h_2, h_3) the rows, *tile the default tile of the push kernel; any may be NULL.
 * The defaults callers use (5 ms, 20 ms, -1 dB) are common figures; they have NOT been tuned on real voices.
 *
 * With x = 0 outside the stream, and a non-finite sample taken as 0, emitted as 0 and counted in n_bad:
 *   u_f[n] = sum_t h_f[t] x[n - 5 + t]   from 0.0f over ascending t, every multiply and every add rounded on its own (no fma)
 *   p[n]   = max(|x[n]|, |u_1[n]|, |u_2[n]|, |u_3[n]|)
 *   q[n]   = 2^23 if p[n] <= c, else (uint32) floor((c / p[n]) * 2^23), the division correctly rounded in fp32;  outside the
 *            stream q = 2^23
 *   m[n]   = min of q[j], j in [n - A - H, n]
 *   s[n]   = sum of m[n - k], k in [0, A]      ((A + 1) 2^23 < 2^32)
 *   g[n]   = s[n] / (A + 1), integer division
 *   y[i]   = x[i] * ((float) g[i + A] * 2^-23)      one fp32 multiply; the conversion and the scaling are exact
 * Every window that enters g[i + A] contains i, so g[i + A] <= q[i] and |y[i]| <= c (1 + 2^-22) for every sample (the slack is the
 * division's rounding plus the product's).  The gain starts to fall A samples before a peak, stays down for H samples behind it and
 * comes back linearly over A + 1 samples.  Minimum, sum and division are exact integer operations: no order needs pinning. */
typedef struct fq3_limit fq3_limit;
/* tile: output samples per workgroup, 0 = the default, else a multiple of 256 in [256, 4096]; the result does not depend on it */
typedef struct fq3_limit_config { int in_rate; double ceiling_db, lookahead_ms, hold_ms; int tile; } fq3_limit_config;
/* true_peak: the largest p of the stream so far;  min_gain_q23: the smallest g applied (2^23: none below 1);  n_limited: output
 * samples with g < 2^23;  n_bad: non-finite samples among those emitted.  Accumulated with integer atomic max / add (the bit pattern
 * of a non-negative float orders as an integer), so they do not depend on any order either. */
typedef struct fq3_limit_report { float true_peak; uint32_t min_gain_q23; int64_t n_limited, n_bad; } fq3_limit_report;
int fq3_limit_design(int in_rate, double ceiling_db, double lookahead_ms, double hold_ms, int* A, int* H, float* ceiling, float* rows,
                     int* tile);
/* Output samples that exist once the first n_in samples of a stream were pushed: final ? n_in : max(0, n_in - A - 6) -- y[i] reaches
 * x[i + A + 6].  n_in in [0, 2^31].  A function of the cumulative length alone.  Negative: an FQ3_E* code. */
int64_t fq3_limit_count(int in_rate, double lookahead_ms, int64_t n_in, int final);
/* One object per stream; it owns the last 2 A + H + 11 input samples (two buffers, used in turn) and the accumulators behind
 * fq3_limit_stats on the current device.  NULL or range errors are answered before any HIP call. */
int fq3_limit_create(const fq3_limit_config* cfg, fq3_limit** out);
int fq3_limit_destroy(fq3_limit* l);                         /* NULL -> 0 */
/* a new stream on the same object: the accumulators are cleared on `stream` */
int fq3_limit_reset(fq3_limit* l, void* stream);
/* pcm: n_in device floats at any float alignment (n_in may be 0, at most 2^31), the next samples of the stream; final != 0: the
 * stream ends with them and the held-back samples come out (a final push with n_in = 0 emits the tail; a stream shorter than the
 * latency is legal).  *n_out (host) = fq3_limit_count(in_rate, lookahead_ms, total so far, final) minus what earlier pushes wrote, known before the launch;
 * above capacity_samples: FQ3_EINVAL and nothing is launched or changed.  out: device floats at any float alignment, not overlapping
 * pcm.  ONE launch on `stream` (none for an empty push that is not final), no host synchronisation; pcm and out must stay valid until
 * the stream has run it.  After a final push: FQ3_ESTATE until fq3_limit_reset. */
int fq3_limit_push(fq3_limit* l, const float* pcm, int64_t n_in, int final, float* out, int64_t capacity_samples, int64_t* n_out,
                   void* stream);
/* the accumulators of the pushes enqueued so far into *stats_dev (DEVICE memory, 8-byte aligned); one launch of one thread */
int fq3_limit_stats(fq3_limit* l, fq3_limit_report* stats_dev, void* stream);

/* ---- Leveller: a causal BS.1770 gain for a stream that has not ended ------------------------------------------------------------------
 * Float32 mono in, float32 out at the same rate: length-preserving, ZERO latency, and independent of how the stream was cut into
 * pushes, of the alignment and of the launch geometry, bit for bit.  Behind the fixed gain (fq3_loud_apply), in front of the limiter.
 * The gain of a sample is built from the loudness meter's hop integers of the hops that ENDED before the sample's own hop began, so it
 * converges to the gain one-shot normalisation (fq3_loud_finish) would have applied to the whole stream.  The stage does NOT limit: a
 * hop louder than everything before it can pass the ceiling -- the limiter is the stage behind it for that.
 *
 * Design constants: in_rate a multiple of 100 in [8000, 48000], H = in_rate / 10;  d = fq3_loud_design(in_rate, target_lufs,
 * ceiling_db, max_gain_db) (the same call, the same ranges);  g0 = (float) 10^(initial_gain_db / 20), computed once on the host in
 * double and rounded once, initial_gain_db in [-60, 40];  k = smooth_hops in [1, 64];  m = min_blocks in [1, 64];  else FQ3_EINVAL.
 * The defaults callers use (-16 LUFS, -1 dBFS, +20 dB, 0 dB, k = 10, m = 8) have NOT been tuned on real voices.
 *
 * Per-hop measures: for every whole hop h of the stream, E_h, peak_h and bad_h are what fq3_loud_push produces for the same samples
 * (the per-hop restart from zero state, the 2^40 quantum and the clip at 64 included): the same integers, bit for bit.
 * Target: T(h), h >= 0, is the gain of the fq3_loud_finish computation run over the PREFIX E[0 .. h) with peak = max(peak_j, j < h)
 * and n_bad = sum(bad_j, j < h) -- the same split sums, doubles, relative gate and min(sqrt(T / mean_power), Gmax, C / peak) -- when
 * that prefix is valid (at least one block passes both gates, no non-finite sample) AND its n_abs >= m; otherwise T(h) = g0.
 * T(h) = g0 for h < 0.  (m keeps the first blocks behind leading silence, which hold more silence than sound and read low, from
 * setting the gain.)
 * Smoothing: S(h) = (float) ((sum over i = h - k + 1 .. h, ascending, of (double) T(i)) / (double) k), so S(-1) = g0.
 * Output: sample n lies in hop h = floor(n / H) at offset j = n - h H:
 *   y[n] = x[n] * fmaf(S(h) - S(h - 1), (float) j / (float) H, S(h - 1))
 * in IEEE float32 (the division correctly rounded), nothing contracted except where written.  A sample of hop h needs only hops < h,
 * which are complete when it arrives.  A non-finite sample passes through (NaN in, NaN out); from the next hop on T = g0.
 * Cost: the target of hop h walks its prefix twice, so a push that enters N hops behind h0 costs about N (h0 + N / 2) block sums:
 * nothing for a stream fed chunk by chunk, but quadratic in ONE push -- about 5 * 10^11 for a single push of 2^20 hops.  Feed audio
 * of more than a few thousand hops in pieces. */
typedef struct fq3_level fq3_level;
/* capacity_hops in [0, 2^20], 0: 4096 hops (about 410 s) */
typedef struct fq3_level_config {
    int in_rate; double target_lufs, ceiling_db, max_gain_db, initial_gain_db; int smooth_hops, min_blocks, capacity_hops;
} fq3_level_config;
/* of the newest hop h = n_hops the stream has entered: target_gain = T(h), smooth_gain = S(h); n_abs / n_rel / n_bad / mean_power:
 * of the prefix E[0 .. h); valid: T(h) is the prefix's measured gain (0: it is g0) */
typedef struct fq3_level_report { double mean_power; float target_gain, smooth_gain; int32_t n_hops, n_abs, n_rel, n_bad, valid, reserved; } fq3_level_report;
/* One object per stream: a loudness meter (fq3_loud_create) plus T per hop, on the current device.  NULL or range errors are answered
 * before any HIP call. */
int fq3_level_create(const fq3_level_config* cfg, fq3_level** out);
int fq3_level_destroy(fq3_level* l);                         /* NULL -> 0 */
/* a new stream on the same object (nothing is enqueued) */
int fq3_level_reset(fq3_level* l, void* stream);
/* g0 = (float) 10^(initial_gain_db / 20) for the stream that begins: legal between create / reset and the first sample (afterwards
 * FQ3_ESTATE), initial_gain_db in [-60, 40] (else FQ3_EINVAL); host only, nothing is enqueued.  It is how ONE kept object serves
 * streams that start from different gains (a voice's last measured one): reset, set, push.  A reset alone keeps the last g0. */
int fq3_level_set_initial_gain(fq3_level* l, double initial_gain_db);
/* pcm: n_in device floats at any float alignment (n_in may be 0), the next samples of the stream; final != 0: the stream ends with
 * them.  out receives exactly n_in samples and may equal pcm (it may not overlap it otherwise).  At most THREE launches on `stream`
 * (the meter's, the targets of the hops the push enters, the multiply; none for an empty push), no host synchronisation.  More hops
 * than the capacity: FQ3_ETOOLONG.  Every error is answered before anything is launched or changed.  After a final push: FQ3_ESTATE
 * until fq3_level_reset. */
int fq3_level_push(fq3_level* l, const float* pcm, int64_t n_in, int final, float* out, void* stream);
/* the state behind the pushes enqueued so far into *stats_dev (DEVICE memory, 8-byte aligned); one launch of one thread.  Before the
 * first sample: T = S = g0, everything else 0. */
int fq3_level_stats(fq3_level* l, fq3_level_report* stats_dev, void* stream);
/* for tests and probes: the hop integers of the n whole hops so far (energy: uint64, peak: float, bad: int32; n values each) and
 * T(0 .. n) (n + 1 floats) to device buffers with room for `capacity` hops (capacity + 1 floats of T; fewer than the hops:
 * FQ3_EINVAL; a NULL buffer is skipped), n to *n_hops (host) */
int fq3_level_trace(fq3_level* l, uint64_t* energy_dev, float* peak_dev, int32_t* bad_dev, float* target_dev, int64_t capacity,
                    int64_t* n_hops, void* stream);

/* ---- the leveller and the limiter for a GROUP of streams: one launch per stage step, whatever the number of rows ------------------
 * For the lock-step batch, as fq3_audio_out_push_group / fq3_tsm_push_group above and with their conventions.  Every array is a HOST
 * array of B entries; row b is exactly
 *     fq3_level_push(objs[b], pcm[b], n_in[b], final[b], out[b], stream)
 *     fq3_limit_push(objs[b], pcm[b], n_in[b], final[b], out[b], capacity_samples[b], &n_out[b], stream)
 *   Equality.        What row b writes, n_out[b] and the state objs[b] is left in -- the meter's hop integers and history, T, the
 *                    stats slot, the limiter's accumulators -- are bit for bit those of the single push: the same device code computes
 *                    them.  Group and single pushes mix freely on one object; membership and order may change from call to call.
 *   Launches.        fq3_leveller_push_group: at most THREE for the whole call (the meters', the targets', the multiplies');
 *                    fq3_limit_push_group: at most ONE.  A launch no row needs is not made.  No host synchronisation and no copy: the
 *                    rows' descriptors travel in the launch's argument block.  pcm[b] and out[b] must stay valid until the stream
 *                    has run the call.
 *   All or nothing.  Every row is checked before any object changes, a leveller's meter included; the checks are the single push's
 *                    own (FQ3_ESTATE after a final push, FQ3_ETOOLONG beyond the hop capacity, FQ3_EINVAL for bad input or capacity).
 *                    On an error the first failing row's code is returned, nothing is launched and no object has moved.
 *   Limits.          B == 0: returns 0, does nothing.  B < 0, B > FQ3_STAGE_GROUP_MAX, a null array, a null object or the same object
 *                    twice in one call: FQ3_EINVAL.  These are answered before any HIP call.
 *   Shared design.   fq3_leveller_push_group: every config field but initial_gain_db and capacity_hops is the same (g0 travels per row);
 *                    fq3_limit_push_group: the same in_rate, ceiling_db, lookahead_ms, hold_ms and tile.  Else FQ3_EINVAL.
 *   Empty rows.      Legal, and they cost workgroups that exit.  A leveller row with n_in == 0 only ends its stream when final; a
 *                    limiter row with n_in == 0 does nothing unless final, and then emits its held-back A + 6 samples (fewer when the
 *                    stream was shorter).  out[b] == pcm[b] stays legal for the leveller; the limiter stays out of place.
 *   Name.            The leveller's entry is fq3_leveller_push_group: the fq3_level_* family above is one stream's interface and stays
 *                    the seven calls it was. */
int fq3_leveller_push_group(fq3_level* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                         float* const* out, void* stream);
int fq3_limit_push_group(fq3_limit* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                         float* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream);

/* ---- Seeded sampling noise: the samplers' Exp(1) variates from a counter-based generator on the device -------------------------
 * The samplers divide by host-provided noise (fq3_sample's noise vector, the rings of fq3_decode_begin).  These calls fill such
 * buffers as a PURE FUNCTION of (seed, emitted-frame index, slot, vocabulary index): no state, no dependence on lane, batch
 * composition, ring size or how the calls are cut.  The contract -- a seed printed today gives the same noise after any later change:
 *   generator   Philox4x32-10: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
 *   key         (seed & 0xffffffff, seed >> 32)
 *   counter     (v >> 2, frame, slot, 0); vocabulary index v takes output word v & 3
 *   frame       the emitted-frame index (the loop state's `frame`): talker and predictor samplers of a frame read ring row
 *               frame % noise_frames
 *   slot        0: the talker's row; 1 + cb: predictor codebook cb in 0 .. G-2; 0xFFFFFFFF with frame 0: the first token after the prefill
 *   variate     k = word >> 9; u = (2 k + 1) 2^-24; e = -ln(u) in fp64, rounded once to fp32 (nearest even) and, in a bf16 context,
 *               once more to bf16.  Range [5.96e-8, 16.64]: strictly positive and finite in both storage types.
 * Known answers:
 *   Philox   counter 0,0,0,0 key 0,0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8;  counter and key all ffffffff -> 408f276d 41c83b0e
 *            a20bc7c6 6d5451fd;  counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   seed 1234, frame 0, slot 0, v = 0..7:  words 2090b348 da7cf0ab 4401906f cbca470e 9eeede35 1cbe137c fa277093 147edd50;  fp32 variates
 *            2.0619323 0.15844612 1.3255798 0.22808668 0.47669414 2.1868014 0.02310045 2.524969 = bits 4003f6b3 3e223fb3 3fa9ac99
 *            3e698f8e 3ef41141 400bf48e 3cbd3d25 40219918
 *   seed 1234, first token (slot 0xFFFFFFFF, frame 0), v = 0..3:  words ab2cfba4 d35d7331 f3a5f4c3 79a03acc;  fp32 variates 0.4024869
 *            0.19159077 0.04945178 0.7442275 = bits 3ece12c3 3e44305f 3d4a8df2 3f3e85b2 */
typedef struct fq3_noise_ring {
    void* talker;               /* T[ring_frames][V] or NULL */
    void* pred;                 /* T[ring_frames][G-1][Vp] or NULL */
    uint64_t seed;
    uint32_t first_frame;       /* emitted-frame index of the first row written */
    int32_t n_frames;           /* rows written: 0 .. ring_frames */
} fq3_noise_ring;
/* Writes, for every i < n and j < rings[i].n_frames, ring row (first_frame + j) % ring_frames of rings[i] with the noise of frame
 * first_frame + j; no other row is touched.  T, V, G and Vp come from ctx's config (ctx is not otherwise used: the rings may belong
 * to any contexts of that shape).  One launch per 32 rings.  All or nothing, checked before anything is queued: FQ3_EINVAL for a NULL
 * ctx or one without a config, NULL rings with n > 0, n < 0, ring_frames < 1, n_frames outside [0, ring_frames], a misaligned ring. */
int fq3_noise_fill(fq3_ctx* ctx, const fq3_noise_ring* rings, int n, int ring_frames, void* stream);
/* out: T[V], the first-token row (slot 0xFFFFFFFF, frame 0) */
int fq3_noise_first(fq3_ctx* ctx, uint64_t seed, void* out, void* stream);
/* Conformance hook: the raw Philox words of one row, out[v] = word v & 3 of counter (v >> 2, frame, slot, 0), for any V >= 1
 * (device uint32[V]).  Needs no context. */
int fq3_noise_words(uint64_t seed, uint32_t frame, uint32_t slot, int V, uint32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FQ3HIP_H */
