// Conformance probe of the kernels that decide which row, which frame, which lane and whether the decode loop goes on: the frame
// prologue and the embedding sum (csrc/decode_kernels.cuh, csrc/batch_kernels.cuh), the prompt builder's row kernels and the open text
// table (csrc/prompt_kernels.cuh), the batch poll and text append, the block table, the paged KV copies and the loop's arming
// (csrc/state_kernels.cuh).  A shared library with a C ABI that launches exactly ONE named kernel on caller-owned device buffers, with
// the launch geometry of its call site in fq3_api.hip / fq3_batch.hip / fq3_prompt.hip / fq3_prefill.hip, and waits for it, so that
// tests/test_gpu_state_reference.py can compare every byte with the model of tests/_state_ref.py.  It includes the product headers (no
// kernel code of its own) and never links into libfq3hip.so.
//
// A kind runs only where `admits` accepts the arguments: whatever would make the kernel address outside the buffers the arguments
// describe is refused with kRefused and nothing is launched -- a token outside the seen / codec_emb rows or a frame beyond the codes
// buffer (frame_begin; the probe reads the DecodeState(s) back to know them), a code id outside its table (embed_sum clamps nothing),
// H no multiple of 8 for the 8-wide kernels, copy widths that are no multiple of 16 bytes, a block-table entry outside the pool, more
// than kMaxLanes lanes or items, a prompt row of kind 3 with a null ref_codes or of kind 2 with a null spk.
//
// Arguments per kind (StateArgs: p = device pointers, tab = tables of device pointers, iv / iv2 = integers, n = sizes, f = floats):
//   FRAME_BEGIN          p: st, past_hidden, codec_emb, pred_in, codes, seen, ph_hold            n: H, G, V (codec_emb rows = seen bytes), frames
//   FRAME_BEGIN_BATCH    p: codec_emb, pred_in   tab[0..4]: st, codes, seen, past_hidden, ph_hold of the lanes   n: H, G, V, frames, B
//   EMBED_SUM            p: st, codes, cos, sin, rope_now, x     tab[0]: the 16 tables           n: H, rope_len, rope_delta, V0, V1, frames, text_rows
//   EMBED_SUM_BATCH      p: x, cos, sin, rope_now   tab[0]: st, tab[1]: codes, tab[2]: the 16 tables   n: H, rope_len, V0, V1, frames, text_rows, B
//   RMSNORM              p: x, w, y                                                               n: K            f: eps
//   COPY                 p: dst, src                                                              n: n
//   TEXT_GATHER          p: ids, table, out                                                       n: n, Ht, vocab
//   PROMPT_ROWS          p: text_rows, prog, ref_codes, spk, out   tab[0]: the 16 tables          n: n_text, n_rows, n_ref, vocab0, vocab_rest, H
//   TEXT_OPEN            p: st, table, rows                                                       n: words, table_words
//   TEXT_PUBLISH         p: st                                                                    n: rows, final
//   POLL_GATHER          p: out                  tab[0]: st of the lanes                          n: B
//   TEXT_SCATTER         p: y                    tab[0]: dst of the items   iv: first[n_items + 1]   iv2: rows each dst holds   n: n_items, row_vec, N
//   TEXT_PUBLISH_LANES                           tab[0]: st of the items    iv: rows   iv2: closes   n: n_items
//   KV_TABLE_WRITE       p: table                iv: vals                                         n: first, count, table_len
//   KV_IMPORT / _EXPORT  p: cache, table, dense                                                   n: blk_stride, n_kv, L, pool_blocks, table_len
//   KV_ADOPT             p: dst_table, src_table   tab[0]: dst, tab[1]: src tensors               n: n_which, nb, blk_elems, dst_blocks, src_blocks, table_len
//   DECODE_ARM           p: st, seen, past_hidden, ph_src   host: the initial DecodeState         n: seen_bytes, ph_words, seen_cap, ph_cap_words
//   DECODE_SET_FORCED    p: tf, forced, decisions
//   DECODE_CANCEL        p: st
//   CODES_TO_I64         p: src, dst                                                              n: n
//   TALKER_STEP          p: st, logits, seen     (sample_talker_kernel, greedy only: the state must say t_do_sample = 0)   n: V, G
#include "../../faster-qwen3-tts_amd/csrc/state_kernels.cuh"
#include "../../faster-qwen3-tts_amd/csrc/prompt_kernels.cuh"
#include <cstddef>
#include <cstdint>
#include <vector>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;

enum Kind {
    K_FRAME_BEGIN = 0, K_FRAME_BEGIN_BATCH, K_EMBED_SUM, K_EMBED_SUM_BATCH, K_RMSNORM, K_COPY, K_TEXT_GATHER, K_PROMPT_ROWS,
    K_KV_IMPORT, K_KV_EXPORT, K_KV_ADOPT, K_TALKER_STEP,                                     // up to here: bf16 and fp32
    K_TEXT_OPEN, K_TEXT_PUBLISH, K_POLL_GATHER, K_TEXT_SCATTER, K_TEXT_PUBLISH_LANES, K_KV_TABLE_WRITE, K_DECODE_ARM,
    K_DECODE_SET_FORCED, K_DECODE_CANCEL, K_CODES_TO_I64,                                    // from K_TEXT_OPEN on: no storage type
    K_COUNT
};
enum Te { TE_BF16 = 0, TE_F32 = 2 };

int g_last_inst = -1;
constexpr bool typed(int kind) { return kind < K_TEXT_OPEN; }
constexpr int inst_id(int kind, int te) { return kind * 2 + ((typed(kind) && te) ? 1 : 0); }

}  // namespace

extern "C" {

struct StateArgs {
    void* p[8];
    void* tab[5][128];
    int iv[132];
    int iv2[128];
    long n[8];
    float f[2];
    const void* host;
};

int state_probe_version() { return kProbeVersion; }
int state_probe_kinds() { return K_COUNT; }
int state_probe_refused_code() { return kRefused; }
int state_probe_last_inst() { return g_last_inst; }
// the instantiations this library holds: every kind, the typed ones in bf16 and fp32
int state_probe_insts(int* out, int cap) {
    int n = 0;
    for (int k = 0; k < K_COUNT; ++k)
        for (int te = 0; te <= (typed(k) ? TE_F32 : 0); te += 2) { if (n < cap) out[n] = inst_id(k, te); ++n; }
    return n;
}

// struct layouts for the ctypes mirrors: groups of [sizeof, offsets of the fields in declaration order] -- DecodeState, TeacherForcing,
// LaneTab, StateArgs -- then kMaxLanes, kMaxVocab, kKeysPerTile, kHeadDim; returns the number of values
int state_probe_layout(long* out, int cap) {
#define D(f) (long)offsetof(DecodeState, f)
#define F(f) (long)offsetof(TeacherForcing, f)
#define L(f) (long)offsetof(LaneTab, f)
#define P(f) (long)offsetof(StateArgs, f)
    const long v[] = {(long)sizeof(DecodeState),
                      D(token), D(frame), D(pos), D(gen_step), D(done), D(text_open), D(min_new), D(max_new), D(trailing_len), D(noise_frames),
                      D(eos_id), D(max_seq), D(sup_lo), D(sup_hi), D(t_temperature), D(t_top_k), D(t_top_p), D(t_do_sample), D(t_rep_penalty),
                      D(p_temperature), D(p_top_k), D(p_top_p), D(p_do_sample), D(trailing_text), D(tts_pad), D(talker_noise), D(pred_noise),
                      D(past_hidden_init), D(n_pad), D(rope_delta),
                      (long)sizeof(TeacherForcing), F(forced), F(decisions),
                      (long)sizeof(LaneTab), L(st), L(codes), L(seen), L(past_hidden), L(ph_hold),
                      (long)sizeof(StateArgs), P(p), P(tab), P(iv), P(iv2), P(n), P(f), P(host),
                      (long)kMaxLanes, (long)kMaxVocab, (long)kKeysPerTile, (long)kHeadDim};
#undef D
#undef F
#undef L
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
bool have(const StateArgs& a, int k) {
    for (int i = 0; i < k; ++i) if (!a.p[i]) return false;
    return true;
}
bool tab_ok(const StateArgs& a, int t, int k) {
    for (int i = 0; i < k; ++i) if (!a.tab[t][i]) return false;
    return true;
}
bool fits(long v) { return v >= 0 && v < (1L << 30); }
template <typename U>
bool fetch(std::vector<U>& h, const void* dev, size_t count) {
    h.resize(count);
    return count == 0 || hipMemcpy(h.data(), dev, count * sizeof(U), hipMemcpyDeviceToHost) == hipSuccess;
}
bool fetch_state(DecodeState& st, const void* dev) { return dev && hipMemcpy(&st, dev, sizeof st, hipMemcpyDeviceToHost) == hipSuccess; }

// one lane of frame_begin: its state against V rows of codec_emb / bytes of seen and `frames` frames of codes
bool frame_begin_ok(const void* st_dev, const void* codes, const void* seen, const void* ph, const void* hold, long V, long frames) {
    DecodeState st;
    if (!fetch_state(st, st_dev) || !codes || !seen || !ph || !hold) return false;
    if (st.done == 1) return true;
    if (st.token != st.eos_id && (st.token < 0 || st.token >= V)) return false;
    return st.frame >= st.max_new || (st.frame >= 0 && st.frame < frames);
}

// one lane of embed_sum: frame inside codes, the frame's 16 ids inside their tables, the text row inside the table the state names
bool embed_sum_ok(const void* st_dev, const void* codes, long H, long V0, long V1, long frames, long text_rows, size_t esz) {
    DecodeState st;
    if (!fetch_state(st, st_dev) || !codes) return false;
    if (st.done != 0 || st.pos >= st.max_seq - 1) return true;
    if (st.frame < 0 || st.frame >= frames || st.gen_step < 0) return false;
    std::vector<int> ids;
    if (!fetch(ids, reinterpret_cast<const int*>(codes) + (size_t)st.frame * 16, 16)) return false;
    for (int g = 0; g < 16; ++g) if (ids[g] < 0 || ids[g] >= (g == 0 ? V0 : V1)) return false;
    if (st.gen_step < st.trailing_len) return st.trailing_text && st.trailing_len <= text_rows && aligned(st.trailing_text, 16);
    return st.tts_pad && aligned(st.tts_pad, 16);
}

bool table_in(const void* dev, long count, long table_len, long blocks) {
    std::vector<int> t;
    if (count > table_len || !fetch(t, dev, (size_t)count)) return false;
    for (int v : t) if (v < 0 || v >= blocks) return false;
    return true;
}

bool admits(int kind, int te, const StateArgs& a) {
    if (kind < 0 || kind >= K_COUNT || (te != TE_BF16 && te != TE_F32)) return false;
    const long* n = a.n;
    for (int i = 0; i < 8; ++i) if (!fits(n[i]) && !(kind == K_EMBED_SUM && i == 2)) return false;
    const size_t esz = te == TE_BF16 ? 2 : 4;
    switch (kind) {
        case K_FRAME_BEGIN:
            return have(a, 7) && n[0] >= 1 && n[1] >= 1 && n[2] >= 1 && n[3] >= 1 && frame_begin_ok(a.p[0], a.p[4], a.p[5], a.p[1], a.p[6], n[2], n[3]);
        case K_FRAME_BEGIN_BATCH: {
            if (!have(a, 2) || n[0] < 1 || n[1] < 1 || n[2] < 1 || n[3] < 1 || n[4] < 1 || n[4] > kMaxLanes) return false;
            for (int l = 0; l < n[4]; ++l)
                if (!frame_begin_ok(a.tab[0][l], a.tab[1][l], a.tab[2][l], a.tab[3][l], a.tab[4][l], n[2], n[3])) return false;
            return true;
        }
        case K_EMBED_SUM:
            return have(a, 6) && tab_ok(a, 0, 16) && n[0] >= 8 && n[0] % 8 == 0 && n[1] >= 1 && n[2] > -(1L << 30) && n[2] < (1L << 30) &&
                   aligned(a.p[5], 16) && embed_sum_ok(a.p[0], a.p[1], n[0], n[3], n[4], n[5], n[6], esz);
        case K_EMBED_SUM_BATCH: {
            if (!have(a, 4) || !tab_ok(a, 2, 16) || n[0] < 8 || n[0] % 8 || n[1] < 1 || n[6] < 1 || n[6] > kMaxLanes || !aligned(a.p[0], 16)) return false;
            for (int l = 0; l < n[6]; ++l)
                if (!embed_sum_ok(a.tab[0][l], a.tab[1][l], n[0], n[2], n[3], n[4], n[5], esz)) return false;
            return true;
        }
        case K_RMSNORM: return have(a, 3) && n[0] >= 1;
        case K_COPY: return have(a, 2) && n[0] >= 1;
        case K_TEXT_GATHER:
            return have(a, 3) && n[0] >= 1 && n[1] >= 8 && n[1] % 8 == 0 && n[2] >= 1 && aligned(a.p[1], 16) && aligned(a.p[2], 16);
        case K_PROMPT_ROWS: {
            const long n_text = n[0], n_rows = n[1], n_ref = n[2], H = n[5];
            if (!a.p[1] || !a.p[4] || !tab_ok(a, 0, 16) || n_rows < 1 || n[3] < 1 || n[4] < 1 || H < 8 || H % 8) return false;
            if ((n_text > 0 && !a.p[0]) || (n_ref > 0 && !a.p[2])) return false;
            std::vector<int> prog;
            if (!fetch(prog, a.p[1], (size_t)n_rows * 3)) return false;
            for (long r = 0; r < n_rows; ++r) {
                if (prog[r * 3 + 1] == 3 && !a.p[2]) return false;       // (a fixed kernel reads nothing here; an unfixed one would)
                if (prog[r * 3 + 1] == 2 && !a.p[3]) return false;
            }
            return true;
        }
        case K_KV_IMPORT: case K_KV_EXPORT: {
            const long blk_stride = n[0], n_kv = n[1], L = n[2], blocks = n[3], table_len = n[4];
            return have(a, 3) && n_kv >= 1 && L >= 1 && blocks >= 1 && blk_stride >= n_kv * kKeysPerTile * kHeadDim && (blk_stride * esz) % 16 == 0 &&
                   aligned(a.p[0], 16) && aligned(a.p[2], 16) && table_in(a.p[1], (L + kKeysPerTile - 1) / kKeysPerTile, table_len, blocks);
        }
        case K_KV_ADOPT: {
            const long n_which = n[0], nb = n[1], blk_elems = n[2];
            if (!have(a, 2) || n_which < 1 || n_which > 128 || nb < 1 || blk_elems < 1 || (blk_elems * esz) % 16) return false;
            for (int w = 0; w < n_which; ++w) if (!a.tab[0][w] || !a.tab[1][w] || !aligned(a.tab[0][w], 16) || !aligned(a.tab[1][w], 16)) return false;
            return table_in(a.p[0], nb, n[5], n[3]) && table_in(a.p[1], nb, n[5], n[4]);
        }
        case K_TALKER_STEP: {
            DecodeState st;
            if (!have(a, 3) || n[0] < 1 || n[0] > kMaxVocab || n[1] < 1 || !fetch_state(st, a.p[0])) return false;
            return st.t_do_sample == 0;
        }
        case K_TEXT_OPEN: return have(a, 3) && n[0] <= n[1];
        case K_TEXT_PUBLISH: case K_DECODE_CANCEL: return have(a, 1);
        case K_POLL_GATHER: return have(a, 1) && n[0] >= 1 && n[0] <= kMaxLanes && tab_ok(a, 0, (int)n[0]);
        case K_TEXT_SCATTER: {
            const long items = n[0], row_vec = n[1], N = n[2];
            if (!have(a, 1) || items < 1 || items > kMaxLanes || row_vec < 1 || N < 1 || a.iv[0] != 0 || a.iv[items] != N) return false;
            for (int i = 0; i < items; ++i) {
                const int cnt = a.iv[i + 1] - a.iv[i];
                if (cnt < 0 || cnt > a.iv2[i] || (cnt > 0 && (!a.tab[0][i] || !aligned(a.tab[0][i], 16)))) return false;
            }
            return aligned(a.p[0], 16);
        }
        case K_TEXT_PUBLISH_LANES: return n[0] >= 0 && n[0] <= kMaxLanes && tab_ok(a, 0, (int)n[0]);
        case K_KV_TABLE_WRITE: return have(a, 1) && n[1] <= 128 && n[0] + n[1] <= n[2];
        case K_DECODE_ARM: return have(a, 4) && a.host && n[0] % 4 == 0 && n[0] <= n[2] && n[1] <= n[3];
        case K_DECODE_SET_FORCED: return a.p[0] != nullptr;
        case K_CODES_TO_I64: return have(a, 2) && n[0] >= 1;
    }
    return false;
}

dim3 el(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

int finish(hipStream_t s) {
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);
    return rc ? rc : rs;
}

// a device copy of a by-address launch argument for the duration of one launch
template <typename U>
struct DevCopy {
    U* d = nullptr;
    int make(const U& h) {
        if (hipMalloc((void**)&d, sizeof(U)) != hipSuccess) return (int)hipGetLastError();
        return (int)hipMemcpy(d, &h, sizeof(U), hipMemcpyHostToDevice);
    }
    ~DevCopy() { if (d) (void)hipFree(d); }
};

EmbTables emb_tables(const StateArgs& a, int t) {
    EmbTables tabs{};
    for (int i = 0; i < 16; ++i) tabs.t[i] = a.tab[t][i];
    return tabs;
}

template <typename T>
int run_typed(int kind, const StateArgs& a, hipStream_t s) {
    const long* n = a.n;
    const dim3 one(1), b256(256);
    switch (kind) {
        case K_FRAME_BEGIN:
            frame_begin_launch<T>((DecodeState*)a.p[0], (const T*)a.p[2], (const T*)a.p[1], (T*)a.p[6], (T*)a.p[3], (int*)a.p[4], (unsigned char*)a.p[5],
                                  (int)n[0], (int)n[1], s);
            break;
        case K_FRAME_BEGIN_BATCH: case K_EMBED_SUM_BATCH: {
            const bool fb = kind == K_FRAME_BEGIN_BATCH;
            const int B = (int)(fb ? n[4] : n[6]);
            LaneTab t{};
            for (int l = 0; l < B; ++l) {
                t.st[l] = (DecodeState*)a.tab[0][l]; t.codes[l] = (int*)a.tab[1][l];
                if (fb) { t.seen[l] = (unsigned char*)a.tab[2][l]; t.past_hidden[l] = a.tab[3][l]; t.ph_hold[l] = a.tab[4][l]; }
            }
            DevCopy<LaneTab> dt;
            if (int r = dt.make(t)) return r;
            if (fb)
                hipLaunchKernelGGL((frame_begin_batch_kernel<T>), dim3(B), b256, 0, s, dt.d, (const T*)a.p[0], (T*)a.p[1], (int)n[0], (int)n[1]);
            else
                hipLaunchKernelGGL((embed_sum_batch_kernel<T, 16>), dim3(B), b256, 0, s, dt.d, emb_tables(a, 2), (T*)a.p[0], (int)n[0], (const float*)a.p[1],
                                   (const float*)a.p[2], (int)n[1], (float*)a.p[3]);
            return finish(s);                         // (the table is freed after the wait)
        }
        case K_EMBED_SUM:
            embed_sum_launch<T, 16>((DecodeState*)a.p[0], emb_tables(a, 0), (const int*)a.p[1], (T*)a.p[5], (int)n[0], (const float*)a.p[2],
                                    (const float*)a.p[3], (int)n[1], (int)n[2], (float*)a.p[4], s);
            break;
        case K_RMSNORM:
            hipLaunchKernelGGL((rmsnorm_kernel<T>), one, b256, 0, s, (const T*)a.p[0], (const T*)a.p[1], (T*)a.p[2], (int)n[0], a.f[0]);
            break;
        case K_COPY:
            hipLaunchKernelGGL((copy_kernel<T>), el((size_t)n[0]), b256, 0, s, (T*)a.p[0], (const T*)a.p[1], (int)n[0]);
            break;
        case K_TEXT_GATHER:
            hipLaunchKernelGGL((text_gather_kernel<T>), dim3((unsigned)n[0]), b256, 0, s, (const int64_t*)a.p[0], (const T*)a.p[1], (T*)a.p[2], (int)n[0],
                               (int)n[1], (int)n[2]);
            break;
        case K_PROMPT_ROWS: {
            RowTables tabs{};
            for (int i = 0; i < 16; ++i) tabs.t[i] = a.tab[0][i];
            hipLaunchKernelGGL((prompt_rows_kernel<T>), dim3((unsigned)n[1]), b256, 0, s, (const T*)a.p[0], a.p[0] ? (int)n[0] : 0, (const int*)a.p[1],
                               (const int64_t*)a.p[2], a.p[2] ? (int)n[2] : 0, (const T*)a.p[3], tabs, (int)n[3], (int)n[4], (T*)a.p[4], (int)n[5]);
            break;
        }
        case K_KV_IMPORT: case K_KV_EXPORT: {
            const int nk = (int)n[1], L = (int)n[2], cnt = nk * L * (kHeadDim * (int)sizeof(T) / 16);
            if (kind == K_KV_IMPORT)
                hipLaunchKernelGGL((kv_paged_copy_kernel<T, true>), el((size_t)cnt), b256, 0, s, (T*)a.p[0], (const int*)a.p[1], (int)n[0], (T*)a.p[2], nk, L);
            else
                hipLaunchKernelGGL((kv_paged_copy_kernel<T, false>), el((size_t)cnt), b256, 0, s, (T*)a.p[0], (const int*)a.p[1], (int)n[0], (T*)a.p[2], nk, L);
            break;
        }
        case K_KV_ADOPT: {
            KvAdoptTab t{};
            for (int w = 0; w < n[0]; ++w) { t.dst[w] = a.tab[0][w]; t.src[w] = a.tab[1][w]; }
            hipLaunchKernelGGL((kv_adopt_kernel<T>), dim3((unsigned)n[0], (unsigned)n[1]), b256, 0, s, t, (const int*)a.p[0], (const int*)a.p[1], (int)n[2]);
            break;
        }
        case K_TALKER_STEP:
            hipLaunchKernelGGL((sample_talker_kernel<T>), one, b256, 0, s, (DecodeState*)a.p[0], (const T*)a.p[1], (int)n[0], (const unsigned char*)a.p[2],
                               (int)n[1], (const TeacherForcing*)nullptr);
            break;
        default: return kRefused;
    }
    return finish(s);
}

int run_plain(int kind, const StateArgs& a, hipStream_t s) {
    const long* n = a.n;
    const dim3 one(1);
    switch (kind) {
        case K_TEXT_OPEN:
            hipLaunchKernelGGL(text_open_kernel, one, dim3(256), 0, s, (DecodeState*)a.p[0], (uint32_t*)a.p[1], (const uint32_t*)a.p[2], (int)n[0]);
            break;
        case K_TEXT_PUBLISH:
            hipLaunchKernelGGL(text_publish_kernel, one, one, 0, s, (DecodeState*)a.p[0], (int)n[0], n[1] ? 1 : 0);
            break;
        case K_POLL_GATHER: {
            LaneSt t{};
            for (int l = 0; l < n[0]; ++l) t.st[l] = (DecodeState*)a.tab[0][l];
            hipLaunchKernelGGL(poll_gather_kernel, one, dim3(kMaxLanes), 0, s, t, (int)n[0], (int*)a.p[0]);
            break;
        }
        case K_TEXT_SCATTER: {
            AppendDst d{};
            for (int i = 0; i < n[0]; ++i) { d.dst[i] = a.tab[0][i]; d.first[i] = a.iv[i]; }
            d.first[n[0]] = a.iv[n[0]];
            hipLaunchKernelGGL(text_scatter_kernel, dim3((unsigned)n[2]), dim3(256), 0, s, d, (int)n[0], (const u32x4*)a.p[0], (int)n[1]);
            break;
        }
        case K_TEXT_PUBLISH_LANES: {
            AppendPub p{};
            for (int i = 0; i < n[0]; ++i) { p.st[i] = (DecodeState*)a.tab[0][i]; p.rows[i] = a.iv[i]; p.closes[i] = a.iv2[i] ? 1 : 0; }
            hipLaunchKernelGGL(text_publish_lanes_kernel, one, dim3(kMaxLanes), 0, s, p, (int)n[0]);
            break;
        }
        case K_KV_TABLE_WRITE: {
            KvTableVals t{};
            for (int i = 0; i < n[1]; ++i) t.v[i] = a.iv[i];
            hipLaunchKernelGGL(kv_table_write_kernel, one, dim3(128), 0, s, (int*)a.p[0], t, (int)n[0], (int)n[1]);
            break;
        }
        case K_DECODE_ARM:
            hipLaunchKernelGGL(decode_arm_kernel, one, dim3(256), 0, s, (DecodeState*)a.p[0], *reinterpret_cast<const DecodeState*>(a.host),
                               (unsigned char*)a.p[1], (int)n[0], (uint32_t*)a.p[2], (const uint32_t*)a.p[3], (int)n[1]);
            break;
        case K_DECODE_SET_FORCED:
            hipLaunchKernelGGL(decode_set_forced_kernel, one, one, 0, s, (TeacherForcing*)a.p[0], (const int*)a.p[1], (int*)a.p[2]);
            break;
        case K_DECODE_CANCEL:
            hipLaunchKernelGGL(decode_cancel_kernel, one, one, 0, s, (DecodeState*)a.p[0]);
            break;
        case K_CODES_TO_I64:
            hipLaunchKernelGGL(codes_to_i64_kernel, el((size_t)n[0]), dim3(256), 0, s, (const int*)a.p[0], (int64_t*)a.p[1], (int)n[0]);
            break;
        default: return kRefused;
    }
    return finish(s);
}

}  // namespace

extern "C" {

// 1 = the kind accepts these arguments in storage type te (0 bf16, 2 fp32; ignored by the kinds without one)
int state_probe_admits(int kind, int te, const StateArgs* a) { return a && admits(kind, te, *a) ? 1 : 0; }

// launch exactly kernel `kind` and wait for it; returns the HIP error of the launch or the wait, or kRefused (nothing launched)
int state_probe_run(int kind, int te, const StateArgs* a, hipStream_t s) {
    if (!a || !admits(kind, te, *a)) return kRefused;
    g_last_inst = inst_id(kind, te);
    if (!typed(kind)) return run_plain(kind, *a, s);
    return te == TE_F32 ? run_typed<float>(kind, *a, s) : run_typed<bf16_t>(kind, *a, s);
}

}  // extern "C"

