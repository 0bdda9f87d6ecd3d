// Conformance probe of the row kernels that run between the GEMM, attention and sampler launches: the vocoder's glue
// (csrc/codec_kernels.cuh), the prefill's vector RMSNorm (csrc/prefill_kernels.cuh) and the analysers' glue (csrc/refenc_kernels.cuh).
// A shared library with a C ABI that launches exactly ONE named kernel on caller-owned device buffers, with the launch geometry of its
// call site in fq3_codec.hip / fq3_refenc.hip / fq3_prefill.hip, so that tests/test_gpu_rows_reference.py can compare every kernel,
// element by element, with the float64 reference of tests/_rows_ref.py.  It includes the product headers (no kernel code of its own)
// and never links into libfq3hip.so.
//
// A kind runs only where `admits` accepts the arguments: whatever would make the kernel read or write outside the caller's buffers
// (a code id outside the codebook, a RoPE position beyond the table, an output conv whose C is no multiple of 8, copy widths or
// offsets that are no multiple of 16 bytes, a codebook size without an instantiation) is refused with kRefused and nothing is launched.
//
// Arguments per kind (RowsArgs: p = device pointers, n = integers, f = floats, tab = device pointer table, pos = positions):
//   RVQ_GATHER / RVQ_GATHER_NEW   p: codes, first, rest     tab: books[nq]     n: nq, n_first, dim, Tn, row_lo, NS, book_rows
//                                 hc: the codes once more on the HOST (NS * Tn * nq ids; _NEW: NS * (Tn - row_lo) * nq)
//   PREFIX_ROWS                   p: dst                    tab: src[NS]       n: src_off, src_ld, dst_seg, dst_ld, dst_row0, dst_col0, n_rows, n_cols, NS, dst_rows, src_elems
//   KEEP_ROWS                     p: src                    tab: dst[NS]       n: src_seg, src_ld, src_row0, src_col0, dst_off, dst_ld, n_rows, n_cols, NS, src_rows, dst_elems
//   RMSNORM_ROWS                  p: x, w, y                                   n: row_lo, rows, C, NS           f: eps
//   RMSNORM_VEC2 / _VEC4          p: x, w, y   (through the rmsnorm_rows dispatcher; C must be 1024 / 2048)   n: rows, C   f: eps
//   LAYERNORM_ROWS                p: x, w, b, y                                n: row_lo, rows, C, NS           f: eps
//   DWCONV7                       p: x, w, b, y                                n: row_lo, rows, C, NS
//   SILU_MUL                      p: gu, y                                     n: rows, I
//   ROPE_ROWS_POS                 p: qkv, cos, sin          pos: base[NS]      n: rows, QD, HD, row_lo, NS, table_rows
//   ROPE_ROWS                     p: qkv, cos, sin                             n: rows, QD, HD, row_lo, NS, table_rows
//   FINAL_CONV                    p: x, w, b, pcm                              n: t_lo, rows, C, NS
//   SNAKE_CONSTS                  p: alpha, beta, a, ib                        n: C
//   CONV_IN                       p: x, w, b, y, e                             n: n, C, K
//   PAD_ROWS                      p: src1, src2 (or null), dst                 n: ld1, ld2, ldd, T, C, pad_l, rows_out, mode
//   CODEBOOK_PREPARE              p: embed_sum, usage, emb, embT               n: K, D                          f: eps
//   RVQ_ENCODE_<VEC>_<PER>        p: proj, codes            tab: emb[nq], then embT[nq] from tab[32]      n: nq, n_sem, K, D, T
//   DFT_MAG                       p: spec, mag                                 n: F, NB
//   COL_STATS                     p: x, logits (or null), mean (or null), std (or null)     n: ldx, ldl, T, C   f: eps
//   SE_SCALE                      p: x, gate, res, y                           n: ldx, ldr, ldy, T, C
#include "../../faster-qwen3-tts_amd/csrc/prefill_kernels.cuh"
#include "../../faster-qwen3-tts_amd/csrc/refenc_kernels.cuh"
#include <cstddef>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;

enum Kind {
    K_RVQ_GATHER = 0, K_RVQ_GATHER_NEW, K_PREFIX_ROWS, K_KEEP_ROWS, K_RMSNORM_ROWS, K_RMSNORM_VEC2, K_RMSNORM_VEC4, K_LAYERNORM_ROWS,
    K_DWCONV7, K_SILU_MUL, K_ROPE_ROWS_POS, K_ROPE_ROWS, K_FINAL_CONV, K_SNAKE_CONSTS,                 // the vocoder: bf16, bf16 x 2, fp32
    K_CONV_IN, K_PAD_ROWS, K_CODEBOOK_PREPARE, K_RVQ_ENC_1_1, K_RVQ_ENC_1_2, K_RVQ_ENC_4_1, K_RVQ_ENC_4_2, K_RVQ_ENC_4_4,
    K_DFT_MAG, K_COL_STATS, K_SE_SCALE,                                                              // the analysers: fp32 only
    K_COUNT
};
enum Te { TE_BF16 = 0, TE_BFS = 1, TE_F32 = 2 };

}  // namespace

extern "C" {

struct RowsArgs {
    void* p[8];
    void* tab[128];
    int pos[128];
    long n[16];
    float f[4];
    const long long* hc;
};

int rows_probe_version() { return kProbeVersion; }
int rows_probe_kinds() { return K_COUNT; }
int rows_probe_refused_code() { return kRefused; }

// struct layout for the ctypes mirror: [sizeof RowsArgs, offsets of the fields in declaration order]; returns the number of values
int rows_probe_layout(long* out, int cap) {
#define P(f) (long)offsetof(RowsArgs, f)
    const long v[] = {(long)sizeof(RowsArgs), P(p), P(tab), P(pos), P(n), P(f), P(hc)};
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

// samples per workgroup final_conv_kernel gets for C channels in storage type te, and its dynamic LDS bytes (the host's own helper)
int rows_probe_final_spw(int C, int te, long* lds_bytes) {
    size_t shm = 0;
    const int spw = final_conv_spw(C, te == TE_BF16 ? 2 : 4, &shm);
    if (lds_bytes) *lds_bytes = (long)shm;
    return spw;
}

}  // extern "C"

namespace {

int esz_of(int te) { return te == TE_BF16 ? 2 : 4; }
bool mult16(long elems, int esz) { return elems >= 0 && (elems * esz) % 16 == 0; }
int enc_k(int kind) {
    switch (kind) {
        case K_RVQ_ENC_1_1: return 256;
        case K_RVQ_ENC_1_2: return 512;
        case K_RVQ_ENC_4_1: return 1024;
        case K_RVQ_ENC_4_2: return 2048;
        case K_RVQ_ENC_4_4: return 4096;
    }
    return 0;
}
bool have(const RowsArgs& a, int k) {
    for (int i = 0; i < k; ++i) if (!a.p[i]) return false;
    return true;
}
bool tab_ok(const RowsArgs& a, int lo, int k) {
    for (int i = lo; i < lo + k; ++i) if (!a.tab[i]) return false;
    return true;
}
bool fits_int(long v) { return v >= 0 && v < (1L << 30); }

bool admits(int kind, int te, const RowsArgs& a) {
    if (kind < 0 || kind >= K_COUNT || te < TE_BF16 || te > TE_F32) return false;
    if (kind >= K_CONV_IN && te != TE_F32) return false;
    const long* n = a.n;
    for (int i = 0; i < 16; ++i) if (!fits_int(n[i])) return false;
    const int esz = esz_of(te);
    switch (kind) {
        case K_RVQ_GATHER: case K_RVQ_GATHER_NEW: {
            const long nq = n[0], n_first = n[1], dim = n[2], Tn = n[3], row_lo = n[4], NS = n[5], book_rows = n[6];
            if (!have(a, 3) || !a.hc || nq < 1 || nq > 32 || n_first < 0 || n_first > nq || dim < 1 || Tn < 1 || row_lo < 0 || row_lo >= Tn ||
                NS < 1 || NS > 65535 || book_rows < 1 || !tab_ok(a, 0, (int)nq)) return false;
            const long ids = NS * (kind == K_RVQ_GATHER ? Tn : Tn - row_lo) * nq;
            for (long i = 0; i < ids; ++i) if (a.hc[i] < 0 || a.hc[i] >= book_rows) return false;
            return true;
        }
        case K_PREFIX_ROWS: {
            const long src_off = n[0], src_ld = n[1], dst_seg = n[2], dst_ld = n[3], dst_row0 = n[4], dst_col0 = n[5], n_rows = n[6], n_cols = n[7],
                       NS = n[8], dst_rows = n[9];
            return have(a, 1) && NS >= 1 && NS <= 128 && tab_ok(a, 0, (int)NS) && n_rows >= 1 && n_cols >= 1 && mult16(n_cols, esz) &&
                   mult16(src_off, esz) && mult16(src_ld, esz) && mult16(dst_seg, esz) && mult16(dst_ld, esz) && mult16(dst_col0, esz) &&
                   n_cols <= src_ld && dst_col0 + n_cols <= dst_ld && dst_row0 + n_rows <= dst_rows && dst_rows * dst_ld <= dst_seg &&
                   src_off + (n_rows - 1) * src_ld + n_cols <= n[10];
        }
        case K_KEEP_ROWS: {
            const long src_seg = n[0], src_ld = n[1], src_row0 = n[2], src_col0 = n[3], dst_off = n[4], dst_ld = n[5], n_rows = n[6], n_cols = n[7],
                       NS = n[8], src_rows = n[9];
            return have(a, 1) && NS >= 1 && NS <= 128 && tab_ok(a, 0, (int)NS) && n_rows >= 1 && n_cols >= 1 && mult16(n_cols, esz) &&
                   mult16(src_seg, esz) && mult16(src_ld, esz) && mult16(src_col0, esz) && mult16(dst_off, esz) && mult16(dst_ld, esz) &&
                   n_cols <= dst_ld && src_col0 + n_cols <= src_ld && src_row0 + n_rows <= src_rows && src_rows * src_ld <= src_seg &&
                   dst_off + (n_rows - 1) * dst_ld + n_cols <= n[10];
        }
        case K_RMSNORM_ROWS:
            return have(a, 3) && n[1] >= 1 && n[0] < n[1] && n[2] >= 1 && n[3] >= 1 && n[3] <= 65535;
        case K_RMSNORM_VEC2: case K_RMSNORM_VEC4:
            return have(a, 3) && n[0] >= 1 && n[1] == (kind == K_RMSNORM_VEC2 ? 1024 : 2048);
        case K_LAYERNORM_ROWS: case K_DWCONV7:
            return have(a, 4) && n[1] >= 1 && n[0] < n[1] && n[2] >= 1 && n[3] >= 1 && n[3] <= 65535;
        case K_SILU_MUL:
            return have(a, 2) && n[0] >= 1 && n[1] >= 1;
        case K_ROPE_ROWS_POS: case K_ROPE_ROWS: {
            const long rows = n[0], QD = n[1], HD = n[2], row_lo = n[3], NS = n[4], table_rows = n[5];
            if (!have(a, 3) || rows < 1 || row_lo < 0 || row_lo >= rows || HD < 2 || HD % 2 || QD < HD || QD % HD || NS < 1 || NS > 128) return false;
            if (kind == K_ROPE_ROWS) return rows <= table_rows;
            for (int u = 0; u < NS; ++u) if (a.pos[u] < 0 || (long)a.pos[u] + (rows - row_lo) > table_rows) return false;
            return true;
        }
        case K_FINAL_CONV: {
            const long t_lo = n[0], rows = n[1], C = n[2], NS = n[3];
            size_t shm = 0;
            return have(a, 4) && rows >= 1 && t_lo < rows && C >= 8 && C % 8 == 0 && NS >= 1 && NS <= 65535 && final_conv_spw((int)C, esz, &shm) != 0;
        }
        case K_SNAKE_CONSTS:
            return have(a, 4) && n[0] >= 1;
        case K_CONV_IN:
            return have(a, 5) && n[0] >= 1 && n[1] >= 1 && n[2] >= 1;
        case K_PAD_ROWS: {
            const long ld1 = n[0], ld2 = n[1], ldd = n[2], T = n[3], C = n[4], rows_out = n[6], mode = n[7];
            return a.p[0] && a.p[2] && T >= 1 && C >= 1 && ld1 >= C && ldd >= C && (!a.p[1] || ld2 >= C) && rows_out >= 1 && (mode == 0 || mode == 1);
        }
        case K_CODEBOOK_PREPARE:
            return have(a, 4) && n[0] >= 1 && n[1] >= 1;
        case K_RVQ_ENC_1_1: case K_RVQ_ENC_1_2: case K_RVQ_ENC_4_1: case K_RVQ_ENC_4_2: case K_RVQ_ENC_4_4: {
            const long nq = n[0], n_sem = n[1], K = n[2], D = n[3], T = n[4];
            return have(a, 2) && nq >= 1 && nq <= 32 && n_sem >= 0 && n_sem <= nq && K == enc_k(kind) && D >= 1 && D <= 8192 && T >= 1 &&
                   tab_ok(a, 0, (int)nq) && tab_ok(a, 32, (int)nq);
        }
        case K_DFT_MAG:
            return have(a, 2) && n[0] >= 1 && n[1] >= 1;
        case K_COL_STATS: {
            const long ldx = n[0], ldl = n[1], T = n[2], C = n[3];
            return a.p[0] && (a.p[2] || a.p[3]) && T >= 1 && C >= 1 && ldx >= C && (!a.p[1] || ldl >= C);
        }
        case K_SE_SCALE:
            return have(a, 4) && n[0] >= n[4] && n[1] >= n[4] && n[2] >= n[4] && n[3] >= 1 && n[4] >= 1;
    }
    return false;
}

dim3 el(size_t n, int NS = 1) { return dim3((unsigned)((n + 255) / 256), (unsigned)NS); }

template <typename T>
int run_codec(int kind, const RowsArgs& a, hipStream_t s) {
    const long* n = a.n;
    const dim3 b256(256);
    switch (kind) {
        case K_RVQ_GATHER: case K_RVQ_GATHER_NEW: {
            RvqArgs ra{};
            ra.nq = (int)n[0]; ra.n_first = (int)n[1]; ra.dim = (int)n[2];
            for (int j = 0; j < ra.nq; ++j) ra.books[j] = a.tab[j];
            const int Tn = (int)n[3], f0 = (int)n[4], NS = (int)n[5];
            if (kind == K_RVQ_GATHER_NEW) hipLaunchKernelGGL((rvq_gather_new_kernel<T>), dim3(Tn - f0, NS), b256, 0, s, ra, (const int64_t*)a.p[0], (T*)a.p[1], (T*)a.p[2], Tn, f0);
            else hipLaunchKernelGGL((rvq_gather_kernel<T>), dim3(Tn - f0, NS), b256, 0, s, ra, (const int64_t*)a.p[0], (T*)a.p[1], (T*)a.p[2], Tn, f0);
            break;
        }
        case K_PREFIX_ROWS: {
            constexpr int EPC = 16 / (int)sizeof(T);
            PrefixSrc src{};
            const int NS = (int)n[8], n_rows = (int)n[6], n_cols = (int)n[7];
            for (int u = 0; u < NS; ++u) src.p[u] = a.tab[u];
            hipLaunchKernelGGL((prefix_rows_kernel<T>), dim3((n_rows * (n_cols / EPC) + 255) / 256, NS), b256, 0, s, src, (size_t)n[0], (int)n[1], (T*)a.p[0],
                               (size_t)n[2], (int)n[3], (int)n[4], (int)n[5], n_rows, n_cols);
            break;
        }
        case K_KEEP_ROWS: {
            constexpr int EPC = 16 / (int)sizeof(T);
            StreamDst dst{};
            const int NS = (int)n[8], n_rows = (int)n[6], n_cols = (int)n[7];
            for (int u = 0; u < NS; ++u) dst.p[u] = a.tab[u];
            hipLaunchKernelGGL((keep_rows_kernel<T>), dim3((n_rows * (n_cols / EPC) + 255) / 256, NS), b256, 0, s, (const T*)a.p[0], (size_t)n[0], (int)n[1],
                               (int)n[2], (int)n[3], dst, (size_t)n[4], (int)n[5], n_rows, n_cols);
            break;
        }
        case K_RMSNORM_ROWS: {
            const int f0 = (int)n[0], Tn = (int)n[1], NS = (int)n[3];
            const dim3 rows4((Tn - f0 + 3) / 4, NS);
            hipLaunchKernelGGL((rmsnorm_rows_kernel<T>), rows4, b256, 0, s, (const T*)a.p[0], (const T*)a.p[1], (T*)a.p[2], f0, Tn, (int)n[2], a.f[0]);
            break;
        }
        case K_RMSNORM_VEC2: case K_RMSNORM_VEC4:
            rmsnorm_rows<T>((const T*)a.p[0], (const T*)a.p[1], (T*)a.p[2], (int)n[0], (int)n[1], a.f[0], s);
            break;
        case K_LAYERNORM_ROWS: {
            const int lo = (int)n[0], R = (int)n[1], NS = (int)n[3];
            hipLaunchKernelGGL((layernorm_rows_kernel<T>), dim3((R - lo + 3) / 4, NS), b256, 0, s, (const T*)a.p[0], (const T*)a.p[1], (const T*)a.p[2], (T*)a.p[3],
                               lo, R, (int)n[2], a.f[0]);
            break;
        }
        case K_DWCONV7: {
            const int lo = (int)n[0], R = (int)n[1], Lc = (int)n[2], NS = (int)n[3];
            hipLaunchKernelGGL((dwconv7_kernel<T>), el((size_t)(R - lo) * Lc, NS), b256, 0, s, (const T*)a.p[0], (const T*)a.p[1], (const T*)a.p[2], (T*)a.p[3], lo, R, Lc);
            break;
        }
        case K_SILU_MUL: {
            const int M = (int)n[0], I = (int)n[1];
            hipLaunchKernelGGL((silu_mul_kernel<T>), dim3((unsigned)(((size_t)M * I + 255) / 256)), b256, 0, s, (const T*)a.p[0], (T*)a.p[1], M, I);
            break;
        }
        case K_ROPE_ROWS_POS: case K_ROPE_ROWS: {
            const int Tn = (int)n[0], QD = (int)n[1], HD = (int)n[2], f0 = (int)n[3], NS = (int)n[4];
            const dim3 grid = el((size_t)(Tn - f0) * 2 * (QD / HD) * (HD / 2), NS);
            if (kind == K_ROPE_ROWS) hipLaunchKernelGGL((rope_rows_kernel<T>), grid, b256, 0, s, (T*)a.p[0], (const float*)a.p[1], (const float*)a.p[2], Tn, QD, HD, f0);
            else {
                StreamPos pos{};
                for (int u = 0; u < NS; ++u) pos.p[u] = a.pos[u];
                hipLaunchKernelGGL((rope_rows_pos_kernel<T>), grid, b256, 0, s, (T*)a.p[0], (const float*)a.p[1], (const float*)a.p[2], Tn, QD, HD, f0, pos);
            }
            break;
        }
        case K_FINAL_CONV: {
            const int lo = (int)n[0], R = (int)n[1], C = (int)n[2], NS = (int)n[3];
            size_t shm = 0;
            const int spw = final_conv_spw(C, (int)sizeof(T), &shm);
            if (spw == 0 || !lds_limit_at_least<final_conv_kernel<T>>(shm)) return kRefused;
            hipLaunchKernelGGL(final_conv_kernel<T>, dim3((R - lo + spw - 1) / spw, NS), b256, shm, s, (const T*)a.p[0], (const T*)a.p[1], (const T*)a.p[2],
                               (float*)a.p[3], lo, R, C, spw);
            break;
        }
        case K_SNAKE_CONSTS: {
            const int C = (int)n[0];
            hipLaunchKernelGGL((snake_consts_kernel<T>), dim3((C + 255) / 256), b256, 0, s, (const T*)a.p[0], (const T*)a.p[1], (T*)a.p[2], (T*)a.p[3], C);
            break;
        }
        default: return kRefused;
    }
    return (int)hipGetLastError();
}

int run_analyser(int kind, const RowsArgs& a, hipStream_t s) {
    const long* n = a.n;
    const dim3 b256(256);
    auto F = [&](int i) { return (const float*)a.p[i]; };
    auto O = [&](int i) { return (float*)a.p[i]; };
    switch (kind) {
        case K_CONV_IN:
            hipLaunchKernelGGL(conv_in_kernel, el((size_t)n[0] * n[1]), b256, 0, s, F(0), F(1), F(2), O(3), O(4), (long)n[0], (int)n[1], (int)n[2]);
            break;
        case K_PAD_ROWS:
            hipLaunchKernelGGL(pad_rows_kernel, el((size_t)n[6] * n[4]), b256, 0, s, F(0), (int)n[0], F(1), (int)n[1], O(2), (int)n[2], (int)n[3], (int)n[4],
                               (int)n[5], (int)n[6], (int)n[7]);
            break;
        case K_CODEBOOK_PREPARE: {
            const int K = (int)n[0], D = (int)n[1];
            hipLaunchKernelGGL(codebook_prepare_kernel, dim3((K * D + 255) / 256), b256, 0, s, F(0), F(1), O(2), O(3), K, D, a.f[0]);
            break;
        }
        case K_RVQ_ENC_1_1: case K_RVQ_ENC_1_2: case K_RVQ_ENC_4_1: case K_RVQ_ENC_4_2: case K_RVQ_ENC_4_4: {
            RvqEncArgs ra{};
            ra.nq = (int)n[0]; ra.n_sem = (int)n[1]; ra.K = (int)n[2]; ra.D = (int)n[3];
            for (int lv = 0; lv < ra.nq; ++lv) { ra.emb[lv] = (const float*)a.tab[lv]; ra.embT[lv] = (const float*)a.tab[32 + lv]; }
            const int T5 = (int)n[4], D = ra.D;
            int64_t* codes = (int64_t*)a.p[1];
            const float* Dd = F(0);
#define ROWS_RVQ(V, P) hipLaunchKernelGGL((rvq_encode_kernel<V, P>), dim3(T5, 2), dim3(256), D * sizeof(float), s, ra, (const float*)Dd, codes)
            switch (ra.K) {
                case 256: ROWS_RVQ(1, 1); break;
                case 512: ROWS_RVQ(1, 2); break;
                case 1024: ROWS_RVQ(4, 1); break;
                case 2048: ROWS_RVQ(4, 2); break;
                default: ROWS_RVQ(4, 4); break;
            }
#undef ROWS_RVQ
            break;
        }
        case K_DFT_MAG:
            hipLaunchKernelGGL(dft_mag_kernel, el((size_t)n[0] * n[1]), b256, 0, s, F(0), O(1), (long)n[0], (int)n[1]);
            break;
        case K_COL_STATS: {
            const int Cb = (int)n[3];
            hipLaunchKernelGGL(col_stats_kernel, dim3((Cb + 63) / 64), dim3(64 * kStatSlices), 0, s, F(0), (int)n[0], F(1), (int)n[1], O(2), O(3), (int)n[2], Cb, a.f[0]);
            break;
        }
        case K_SE_SCALE:
            hipLaunchKernelGGL(se_scale_kernel, el((size_t)n[3] * n[4]), b256, 0, s, F(0), (int)n[0], F(1), F(2), (int)n[1], O(3), (int)n[2], (int)n[3], (int)n[4]);
            break;
        default: return kRefused;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// 1 = the kind accepts these arguments in storage type te (0 bf16, 1 bf16 x 2, 2 fp32)
int rows_probe_admits(int kind, int te, const RowsArgs* a) { return a && admits(kind, te, *a) ? 1 : 0; }

// launch exactly kernel `kind`; returns hipGetLastError() after the launch, or kRefused (nothing launched)
int rows_probe_run(int kind, int te, const RowsArgs* a, hipStream_t s) {
    if (!a || !admits(kind, te, *a)) return kRefused;
    if (kind >= K_CONV_IN) return run_analyser(kind, *a, s);
    if (te == TE_BFS) return run_codec<bfs_t>(kind, *a, s);
    if (te == TE_F32) return run_codec<float>(kind, *a, s);
    return run_codec<bf16_t>(kind, *a, s);
}

}  // extern "C"
