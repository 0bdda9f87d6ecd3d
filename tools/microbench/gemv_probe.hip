// Conformance probe of the decode GEMV kernels (csrc/decode_kernels.cuh: gemv_kernel; csrc/batch_kernels.cuh: gemv_batch_kernel,
// rmsnorm_batch_kernel, gemv_batch_mfma_norm_kernel, gemv_batch_mfma_plain_kernel): a shared library with a C ABI that launches exactly
// ONE named instantiation on caller-owned device buffers, so that tests/test_gpu_gemv_reference.py can compare each of them, element by
// element, with the float64 reference of tests/_gemv_ref.py.  It includes the product headers (no GEMV arithmetic of its own), takes
// grid, rows per wave, tokens per LDS pass and LDS bytes from the launchers' own helpers in those headers, and never links into
// libfq3hip.so.
//
// Built instantiations = what fq3_api.hip / fq3_batch.hip can launch (built_gemv / built_batch / built_norm / built_plain below; the
// PRO_COMBINE prologue stages K <= kCombineMaxK = 2048, so its 6- and 12-chunk forms are not built here).  Anything that would make a
// kernel read or write outside the buffers the arguments describe is refused with kRefused and nothing is launched.
#include "../../faster-qwen3-tts_amd/csrc/batch_kernels.cuh"
#include "../../faster-qwen3-tts_amd/csrc/skinny_gemm.cuh"
#include <cstddef>
#include <vector>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;
constexpr int kLdsRefused = 100001;      // the device refused the dynamic LDS the launch needs

enum Kind {
    K_GEMV = 0,         // gemv_kernel<T, NCH, PRO, EPI, NT, M, R>: M = B (1 or 2), NT = nt, R by the launcher's rule under the cap `rows`
    K_BATCH,            // gemv_batch_kernel<T, NCH, PRO, EPI>, `group` tokens per LDS pass (0: the launcher's choice)
    K_RMSNORM,          // rmsnorm_batch_kernel<2 | 4> (bf16)
    K_MFMA_NORM,        // gemv_batch_mfma_norm_kernel<K / 128, EPI, nt, dual> (bf16)
    K_MFMA_PLAIN,       // gemv_batch_mfma_plain_kernel<KSTEPS, NW, EPI, nt> (bf16)
    K_COUNT
};
enum Te { TE_BF16 = 0, TE_F32 = 2 };          // the storage-type codes of the GEMM probe

int g_last_inst = -1;                          // id of the instantiation the last successful run launched

// ---- what is built ---------------------------------------------------------------------------------------------------------------
// (PRO, EPI) pairs: 0 NORM+STORE, 1 NORM+SWIGLU, 2 PLAIN+STORE, 3 PLAIN+RESIDUAL, 4 COMBINE+RESIDUAL
constexpr int kPairs = 5;
constexpr int pair_pro(int pe) { return pe < 2 ? PRO_NORM : (pe < 4 ? PRO_PLAIN : PRO_COMBINE); }
constexpr int pair_epi(int pe) { return (pe == 0 || pe == 2) ? EPI_STORE : (pe == 1 ? EPI_SWIGLU : EPI_RESIDUAL); }
int pair_of(int pro, int epi) {
    for (int pe = 0; pe < kPairs; ++pe) if (pair_pro(pe) == pro && pair_epi(pe) == epi) return pe;
    return -1;
}
constexpr int kNch[5] = {1, 2, 4, 6, 12};
constexpr int nch_index(int nch) { return nch == 1 ? 0 : nch == 2 ? 1 : nch == 4 ? 2 : nch == 6 ? 3 : 4; }
// chunks per lane at most: the launchers' own cap (gemv_most_chunks), and for the merge prologue what K <= kCombineMaxK leaves of it
constexpr int most_nch(int pro, int m) { return pro == PRO_COMBINE ? (kCombineMaxK + 511) / 512 : gemv_most_chunks(pro, m); }
constexpr int max_rows(int nch, int epi) { return nch >= 12 ? 1 : (nch >= 6 ? (epi == EPI_SWIGLU ? 1 : 2) : 2); }      // = MaxRows<NCH, EPI>::v
constexpr bool built_gemv(int pe, int nch, bool nt, int m, int r) {
    return nch <= most_nch(pair_pro(pe), m) && (m == 1 || (m == 2 && !nt)) && r >= 1 && r <= max_rows(nch, pair_epi(pe));
}
constexpr int gemv_id(int te, int pe, int nch, bool nt, int m, int r) {
    return (((((te ? 1 : 0) * kPairs + pe) * 5 + nch_index(nch)) * 2 + (nt ? 1 : 0)) * 2 + (m - 1)) * 2 + (r - 1);
}
constexpr bool built_batch(int pe, int nch) { return pe < 4 && nch <= most_nch(pair_pro(pe), 1); }
constexpr int batch_id(int te, int pe, int nch) { return ((te ? 1 : 0) * 4 + pe) * 5 + nch_index(nch); }
// norm kernel: KSTEPS 2, 4, 8, 16; EPI STORE / SWIGLU; NT 1..4, 0; DUAL for KSTEPS <= 8 and NT != 1
constexpr int ks_index(int ks) { return ks == 2 ? 0 : ks == 4 ? 1 : ks == 8 ? 2 : 3; }
constexpr bool built_norm(int ks, int nt, bool dual) { return !dual || (ks <= 8 && nt != 1); }
constexpr int norm_id(int ks, int epi, int nt, bool dual) { return ((ks_index(ks) * 2 + (epi == EPI_SWIGLU ? 1 : 0)) * 5 + nt) * 2 + (dual ? 1 : 0); }
constexpr int kPlainK[8] = {256, 512, 768, 1024, 2048, 3072, 4096, 6144};
int plain_k_index(int K) {
    for (int i = 0; i < 8; ++i) if (kPlainK[i] == K) return i;
    return -1;
}
int plain_id(int K, int epi, int nt) { return (plain_k_index(K) * 2 + (epi == EPI_RESIDUAL ? 1 : 0)) * 5 + nt; }

int count_built(int kind) {
    int n = 0;
    switch (kind) {
        case K_GEMV:
            for (int pe = 0; pe < kPairs; ++pe) for (int nch : kNch) for (int nt = 0; nt < 2; ++nt) for (int m = 1; m <= 2; ++m)
                for (int r = 1; r <= 2; ++r) n += built_gemv(pe, nch, nt != 0, m, r) ? 2 : 0;                  // x 2 storage types
            return n;
        case K_BATCH:
            for (int pe = 0; pe < 4; ++pe) for (int nch : kNch) n += built_batch(pe, nch) ? 2 : 0;
            return n;
        case K_RMSNORM: return 2;
        case K_MFMA_NORM:
            for (int ks : {2, 4, 8, 16}) for (int nt = 0; nt < 5; ++nt) for (int d = 0; d < 2; ++d) n += built_norm(ks, nt, d != 0) ? 2 : 0;      // x 2 epilogues
            return n;
        case K_MFMA_PLAIN: return 8 * 2 * 5;
    }
    return 0;
}

}  // namespace

extern "C" {

// Everything one probe launch needs.  Device pointers; T = the storage type of the call.
//   W [N (+ up_off for SWIGLU)][K] row-major; Wp: its fragment-major copy (gemv_probe_pack; the matrix-core kinds only) or null
//   x [B][x_stride], y [B][y_stride], res [B][res_stride] (may alias y); norm_w [K], bias [N] or null
//   xn_out: null, or the base of [B][xn_stride] rows that receive the prologue result (K_GEMV: token 0 only; the batch kinds: the probe
//   builds the device pointer table base + t * xn_stride itself); K_RMSNORM writes y [B][y_stride] with K values per row
//   part: PRO_COMBINE, [B][part_stride] floats of [K / 128 / rep][8][rep][132] partial slots
struct GemvProbeArgs {
    int N, K, B;
    int pro, epi;
    int nt;                         // K_GEMV: non-temporal weight loads (0 / 1); matrix-core kinds: the NT template argument (1..4, 0 = runtime count)
    int rows;                       // K_GEMV: cap on rows per wave (the launcher's rmax; 0 = none)
    int group;                      // K_BATCH: tokens per LDS pass (0 = the launcher's choice)
    int dual;                       // K_MFMA_NORM: the two-panel form
    int ntiles;                     // matrix-core kinds with nt = 0: the runtime tile count
    int up_off;                     // SWIGLU: first "up" row
    int n_part, rep;                // PRO_COMBINE
    int x_stride, y_stride, res_stride, xn_stride;
    long part_stride;
    float eps;
    const void* W; const void* Wp; const void* x; const void* norm_w; const void* bias;
    void* y; const void* res; void* xn_out; const float* part;
};

int gemv_probe_version() { return kProbeVersion; }
int gemv_probe_kinds() { return K_COUNT; }
int gemv_probe_refused_code() { return kRefused; }
// instantiations built for `kind`, and the id (unique within a kind) of the one the last successful gemv_probe_run launched
int gemv_probe_built(int kind) { return count_built(kind); }
int gemv_probe_last_inst() { return g_last_inst; }
// chunks per lane the probe builds at most for prologue `pro` and m tokens per pass (the ctypes side mirrors it)
int gemv_probe_most_chunks(int pro, int m) { return most_nch(pro, m); }

// struct layout for the ctypes mirror: [sizeof GemvProbeArgs, offsets of its fields in declaration order, kMaxLanes, kTokTile,
// kGroupLanes, kCombineMaxK, kMaxWorkers, kPartStride]; returns the number of values written
int gemv_probe_layout(long* out, int cap) {
#define P(f) (long)offsetof(GemvProbeArgs, f)
    const long v[] = {(long)sizeof(GemvProbeArgs),
                      P(N), P(K), P(B), P(pro), P(epi), P(nt), P(rows), P(group), P(dual), P(ntiles), P(up_off), P(n_part), P(rep),
                      P(x_stride), P(y_stride), P(res_stride), P(xn_stride), P(part_stride), P(eps), P(W), P(Wp), P(x), P(norm_w), P(bias),
                      P(y), P(res), P(xn_out), P(part),
                      (long)kMaxLanes, (long)kTokTile, (long)kGroupLanes, (long)kCombineMaxK, (long)kMaxWorkers, (long)kPartStride};
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

template <typename T> int group_max_for(int K) { return batch_group_max<T>((K + 511) / 512); }

bool admits(int kind, int te, const GemvProbeArgs& p) {
    if ((te != TE_BF16 && te != TE_F32) || kind < 0 || kind >= K_COUNT) return false;
    const int esz = te == TE_BF16 ? 2 : 4;
    if (p.K < 8 || p.K % 8 || p.N < 1 || p.N > (1 << 24) || p.B < 1 || !p.y) return false;
    if (!p.x && !(kind == K_GEMV && p.pro == PRO_COMBINE)) return false;
    if (p.xn_out && p.xn_stride < p.K) return false;
    if (kind == K_RMSNORM) {
        return te == TE_BF16 && p.K <= 2048 && p.B <= (1 << 16) && p.norm_w && p.x_stride >= p.K && p.y_stride >= p.K;
    }
    const int pe = pair_of(p.pro, p.epi);
    if (pe < 0 || !p.W) return false;
    const int pro = p.pro, epi = p.epi;
    if (pro == PRO_NORM && !p.norm_w) return false;
    if (epi == EPI_RESIDUAL && !p.res) return false;
    if (epi == EPI_SWIGLU && p.up_off < p.N) return false;
    const bool strided = kind != K_GEMV || p.B > 1;              // one token: no row follows another
    if (strided) {
        if (pro != PRO_COMBINE && p.x_stride < p.K) return false;
        if (p.y_stride < p.N || (epi == EPI_RESIDUAL && p.res_stride < p.N)) return false;
    }
    if (kind == K_GEMV) {
        if (p.B > 2 || (p.nt != 0 && p.nt != 1) || (p.B == 2 && p.nt) || p.rows < 0 || p.rows > 2 || p.Wp) return false;
        if (!gemv_chunks(p.K, most_nch(pro, p.B))) return false;
        if (pro == PRO_COMBINE) {
            if (p.K > kCombineMaxK || p.K % kHeadDim || !p.part || p.n_part < 1 || p.n_part > kMaxWorkers) return false;
            if ((p.rep != 1 && p.rep != 2 && p.rep != 4) || (p.K / kHeadDim) % p.rep) return false;
            if (p.B == 2 && p.part_stride < (long)(p.K / kHeadDim) * kMaxWorkers * kPartStride) return false;
        }
        return true;
    }
    if (pro == PRO_COMBINE || p.B > kMaxLanes) return false;
    if (kind == K_BATCH) {
        if (p.Wp || !gemv_chunks(p.K, most_nch(pro, 1)) || p.group < 0) return false;
        const int gmax = te == TE_BF16 ? group_max_for<bf16_t>(p.K) : group_max_for<float>(p.K);
        if (p.group > gmax || p.group > p.B) return false;
        if (p.group && (size_t)p.group * p.K * esz > kBatchGemvLdsBudget) return false;
        return true;
    }
    // the matrix-core kinds
    if (te != TE_BF16 || p.nt < 0 || p.nt > 4) return false;
    const int need = (p.B + kTokTile - 1) / kTokTile;
    if (p.nt ? p.nt != need : p.ntiles != need) return false;
    if (p.Wp && (p.N % 16 || p.K % 32 || (epi == EPI_SWIGLU && p.up_off % 16))) return false;
    if (kind == K_MFMA_NORM) {
        if (pro != PRO_NORM || !one_of<256, 512, 1024, 2048>(p.K)) return false;
        if (p.dual != 0 && p.dual != 1) return false;
        if (p.dual && (!built_norm(p.K / 128, p.nt, true) || p.B <= kTokTile)) return false;        // a second tile's tokens are loaded up front
        return true;
    }
    return pro == PRO_PLAIN && plain_k_index(p.K) >= 0 && !p.dual;
}

int finish(hipStream_t s) {
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);
    return rc ? rc : rs;
}

// ---- gemv_kernel -----------------------------------------------------------------------------------------------------------------
template <typename T, int PE, int NCH, bool NT, int M>
int launch_one_gemv(const GemvArgs& a, int rmax, int te, hipStream_t s) {
    constexpr int PRO = pair_pro(PE), EPI = pair_epi(PE);
    static_assert(max_rows(NCH, EPI) == MaxRows<NCH, EPI>::v, "max_rows mirrors MaxRows");
    const int R = gemv_rows_per_wave<NCH, EPI>(a.N, rmax);
    const int grid = gemv_grid(a.N, R);
    const size_t shm = gemv_lds_bytes<PRO, M>(a.K);
    g_last_inst = gemv_id(te, PE, NCH, NT, M, R);
    if constexpr (MaxRows<NCH, EPI>::v >= 2) {
        if (R == 2) { gemv_launch<T, NCH, PRO, EPI, NT, M, 2>(a, grid, shm, s); return 0; }
    }
    gemv_launch<T, NCH, PRO, EPI, NT, M, 1>(a, grid, shm, s);
    return 0;
}

template <typename T>
int run_gemv(const GemvProbeArgs& p, int te, hipStream_t s) {
    GemvArgs a{};
    a.W = p.W; a.N = p.N; a.K = p.K; a.x = p.x; a.norm_w = p.norm_w; a.eps = p.eps; a.bias = p.bias; a.y = p.y; a.res = p.res;
    a.xn_out = p.xn_out; a.up_off = p.up_off; a.part = p.part; a.n_part = p.n_part; a.rep = p.rep;
    if (p.B == 2) {
        a.x2 = p.x ? reinterpret_cast<const T*>(p.x) + p.x_stride : nullptr;
        a.y2 = reinterpret_cast<T*>(p.y) + p.y_stride;
        a.res2 = p.res ? reinterpret_cast<const T*>(p.res) + p.res_stride : nullptr;
        a.part_stride2 = (size_t)p.part_stride;
    }
    const int pe = pair_of(p.pro, p.epi), M = p.B;
    const int n = gemv_chunks(p.K, most_nch(p.pro, M));
    int rc = kRefused;
    with_value<0, 1, 2, 3, 4>(pe, [&](auto pev) {
        constexpr int PE = decltype(pev)::value;
        with_value<1, 2, 4, 6, 12>(n, [&](auto nchv) {
            constexpr int NCH = decltype(nchv)::value;
            if constexpr (built_gemv(PE, NCH, false, 1, 1)) {
                if (M == 1) rc = p.nt ? launch_one_gemv<T, PE, NCH, true, 1>(a, p.rows, te, s) : launch_one_gemv<T, PE, NCH, false, 1>(a, p.rows, te, s);
            }
            if constexpr (built_gemv(PE, NCH, false, 2, 1)) {
                if (M == 2) rc = launch_one_gemv<T, PE, NCH, false, 2>(a, p.rows, te, s);
            }
        });
    });
    return rc ? rc : finish(s);
}

// ---- the batch kinds ---------------------------------------------------------------------------------------------------------------
// the per-token xn_out pointer table: base + t * stride, in device memory for the duration of the launch
struct PtrTable {
    void** dev = nullptr;
    int make(void* base, int B, size_t stride_bytes) {
        if (!base) return 0;
        std::vector<void*> h(B);
        for (int t = 0; t < B; ++t) h[t] = reinterpret_cast<char*>(base) + (size_t)t * stride_bytes;
        if (hipMalloc(&dev, sizeof(void*) * B) != hipSuccess) return (int)hipGetLastError();
        if (hipMemcpy(dev, h.data(), sizeof(void*) * B, hipMemcpyHostToDevice) != hipSuccess) return (int)hipGetLastError();
        return 0;
    }
    ~PtrTable() { if (dev) (void)hipFree(dev); }
};

BatchGemvArgs batch_args(const GemvProbeArgs& p, void* const* table) {
    BatchGemvArgs a{};
    a.W = p.W; a.N = p.N; a.K = p.K; a.B = p.B; a.x = p.x; a.x_stride = p.x_stride; a.norm_w = p.norm_w; a.eps = p.eps; a.bias = p.bias;
    a.y = p.y; a.y_stride = p.y_stride; a.res = p.res; a.res_stride = p.res_stride; a.up_off = p.up_off; a.xn_out = table;
    a.ntiles = (p.B + kTokTile - 1) / kTokTile; a.Wp = p.Wp;
    return a;
}

template <typename T>
int run_batch(const GemvProbeArgs& p, int te, hipStream_t s) {
    PtrTable tab;
    if (int r = tab.make(p.xn_out, p.B, (size_t)p.xn_stride * sizeof(T))) return r;
    BatchGemvArgs a = batch_args(p, tab.dev);
    a.Wp = nullptr;
    const int esz = (int)sizeof(T);
    a.group = p.group ? p.group : batch_gemv_group<T>(a.B, a.K, esz);
    const size_t shm = (size_t)a.group * a.K * esz;
    if (shm > kBatchGemvLdsBudget) return kRefused;
    const int grid = (a.N + 3) / 4;
    const int pe = pair_of(p.pro, p.epi);
    const int n = gemv_chunks(a.K, most_nch(p.pro, 1));
    int rc = kRefused;
    with_value<0, 1, 2, 3>(pe, [&](auto pev) {
        constexpr int PE = decltype(pev)::value;
        with_value<1, 2, 4, 6, 12>(n, [&](auto nchv) {
            constexpr int NCH = decltype(nchv)::value;
            if constexpr (built_batch(PE, NCH)) {
                constexpr auto kern = gemv_batch_kernel<T, NCH, pair_pro(PE), pair_epi(PE)>;
                if (!lds_limit_at_least<kern>(shm)) { rc = kLdsRefused; return; }
                g_last_inst = batch_id(te, PE, NCH);
                hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shm, s, a);
                rc = 0;
            }
        });
    });
    return rc ? rc : finish(s);
}

int run_rmsnorm(const GemvProbeArgs& p, hipStream_t s) {
    PtrTable tab;
    if (int r = tab.make(p.xn_out, p.B, (size_t)p.xn_stride * sizeof(bf16_t))) return r;
    const dim3 grid((p.B + 3) / 4);
    const bf16_t* x = reinterpret_cast<const bf16_t*>(p.x);
    const bf16_t* w = reinterpret_cast<const bf16_t*>(p.norm_w);
    bf16_t* y = reinterpret_cast<bf16_t*>(p.y);
    g_last_inst = p.K <= 1024 ? 0 : 1;
    if (p.K <= 1024) hipLaunchKernelGGL((rmsnorm_batch_kernel<2>), grid, dim3(256), 0, s, x, p.x_stride, w, p.eps, p.K, p.B, y, p.y_stride, tab.dev);
    else hipLaunchKernelGGL((rmsnorm_batch_kernel<4>), grid, dim3(256), 0, s, x, p.x_stride, w, p.eps, p.K, p.B, y, p.y_stride, tab.dev);
    return finish(s);
}

template <int EPI>
int run_mfma_norm(const GemvProbeArgs& p, hipStream_t s) {
    PtrTable tab;
    if (int r = tab.make(p.xn_out, p.B, (size_t)p.xn_stride * sizeof(bf16_t))) return r;
    const BatchGemvArgs a = batch_args(p, tab.dev);
    const int grid = (a.N + 15) / 16;
    constexpr int NR = EPI == EPI_SWIGLU ? 2 : 1;
    const size_t shm = norm_panel_lds(a.K, NR, p.dual ? 2 : 1);
    int rc = kRefused;
    with_value<2, 4, 8, 16>(a.K / 128, [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        with_value<1, 2, 3, 4, 0>(p.nt, [&](auto ntv) {
            constexpr int NT = decltype(ntv)::value;
            auto go = [&](auto dualv) {
                constexpr bool DUAL = decltype(dualv)::value != 0;
                if constexpr (built_norm(KS, NT, DUAL)) {
                    constexpr auto kern = gemv_batch_mfma_norm_kernel<KS, EPI, NT, DUAL>;
                    if (!lds_limit_at_least<kern>(shm)) { rc = kLdsRefused; return; }
                    g_last_inst = norm_id(KS, EPI, NT, DUAL);
                    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shm, s, a);
                    rc = 0;
                }
            };
            if (p.dual) go(std::integral_constant<int, 1>{}); else go(std::integral_constant<int, 0>{});
        });
    });
    return rc ? rc : finish(s);
}

template <int EPI>
int run_mfma_plain(const GemvProbeArgs& p, hipStream_t s) {
    const BatchGemvArgs a = batch_args(p, nullptr);
    with_value<256, 512, 768, 1024, 2048, 3072, 4096, 6144>(a.K, [&](auto k) {
        constexpr int NW = plain_mfma_nw(decltype(k)::value), KS = plain_mfma_ksteps(decltype(k)::value);
        with_value<1, 2, 3, 4, 0>(p.nt, [&](auto nt) {
            hipLaunchKernelGGL((gemv_batch_mfma_plain_kernel<KS, NW, EPI, decltype(nt)::value>), dim3((a.N + 15) / 16), dim3(64 * NW), 0, s, a);
        });
    });
    g_last_inst = plain_id(a.K, EPI, p.nt);
    return finish(s);
}

}  // namespace

extern "C" {

// 1 = these arguments stay inside the buffers they describe for kind `kind` in storage type te (0 bf16, 2 fp32)
int gemv_probe_admits(int kind, int te, const GemvProbeArgs* p) { return p && admits(kind, te, *p) ? 1 : 0; }

// launch exactly one instantiation and wait for it; returns the HIP error of the launch or the wait, kLdsRefused, or kRefused (nothing
// launched)
int gemv_probe_run(int kind, int te, const GemvProbeArgs* p, hipStream_t s) {
    if (!p || !admits(kind, te, *p)) return kRefused;
    switch (kind) {
        case K_GEMV: return te == TE_F32 ? run_gemv<float>(*p, te, s) : run_gemv<bf16_t>(*p, te, s);
        case K_BATCH: return te == TE_F32 ? run_batch<float>(*p, te, s) : run_batch<bf16_t>(*p, te, s);
        case K_RMSNORM: return run_rmsnorm(*p, s);
        case K_MFMA_NORM: return p->epi == EPI_SWIGLU ? run_mfma_norm<EPI_SWIGLU>(*p, s) : run_mfma_norm<EPI_STORE>(*p, s);
        case K_MFMA_PLAIN: return p->epi == EPI_RESIDUAL ? run_mfma_plain<EPI_RESIDUAL>(*p, s) : run_mfma_plain<EPI_STORE>(*p, s);
    }
    return kRefused;
}

// fragment-major copy (the product's skinny_pack, kind 0: 16-row blocks) of a bf16 [N][K] weight
int gemv_probe_pack(const void* W, void* P, int N, int K, hipStream_t s) {
    if (!W || !P || N <= 0 || N % 16 || K <= 0 || K % 32) return kRefused;
    skinny_pack(reinterpret_cast<const bf16_t*>(W), reinterpret_cast<bf16_t*>(P), N, K, 0, s);
    return finish(s);
}

}  // extern "C"
