// Conformance probe of the implicit-GEMM kernel families (csrc/codec_kernels.cuh, csrc/skinny_gemm.cuh): a shared library with a C ABI
// that launches exactly ONE named family on caller-owned device buffers, so that tests/test_gpu_gemm_reference.py can compare every
// family, element by element, with the float64 reference of tests/_gemm_ref.py.  It includes the product headers the way
// gemm_bench.hip does (no kernel code of its own) and never links into libfq3hip.so.
//
// A family runs only where its guard admits the shape (the conditions gemm_launch / gemm_swiglu_halves / resunit_launch check
// before they pick it); anything else is refused with kRefused and nothing is launched.
#include "../../faster-qwen3-tts_amd/csrc/codec_kernels.cuh"
#include <cstddef>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;

enum Family {
    F_CONV_64x32 = 0, F_CONV_64x64, F_CONV_128x32, F_CONV_128x64, F_CONV_128x96,     // register-prefetch conv_gemm_kernel tiles
    F_SPLITK,                                                                        // conv_gemm_kernel<64, 32, 8> with ksplit + splitk_reduce_kernel
    F_GLDS4_128x64_S2,                                                               // LDS-DMA tile by four waves
    F_GLDS8_64x128_S3, F_GLDS8_64x64_S3, F_GLDS8_128x64_S3, F_GLDS8_128x64_S2,     // ... by eight waves
    F_CHAIN_8x8, F_CHAIN_16x4,                                                       // chain GEMM
    F_BIG_TR_PAIR, F_BIG_PAIR, F_BIG_TR_RING, F_BIG_RING, F_BIG_TR_128, F_BIG_128,  // 256-row ring tiles
    F_SKINNY,                                                                        // SK_STORE / SK_RESIDUAL (by res), NORM by ssq
    F_SKINNY_SWIGLU,                                                                 // SK_SWIGLU (NORM by ssq)
    F_SWIGLU_HALVES,                                                                 // gemm_swiglu_halves<bf16_t>
    F_RESUNIT,                                                                       // resunit_launch<T>
    F_LAUNCH,                                                                        // gemm_launch<T>: the product dispatcher
    F_COUNT
};
enum Te { TE_BF16 = 0, TE_BFS = 1, TE_F32 = 2 };

}  // namespace

extern "C" {

// Everything one probe launch needs.  g: the GEMM (conv1 of a residual unit), in the storage type's own units (bfs_t: as gemm_launch<bfs_t>
// takes them; the probe doubles lda / Cin / a_seg for the tile families as gemm_launch<bfs_t> does).
struct ProbeArgs {
    GemmArgs g;
    GemmArgs g2;                    // F_RESUNIT: conv2
    void* y;                        // F_SWIGLU_HALVES / F_SKINNY_SWIGLU: the [M][N / 2] output
    int rb_force;                   // skinny: weight-row blocks per wave (0 = the launcher's choice)
    int mt;                         // skinny: workgroups per row group (0 = the launcher's choice)
    float* ssq_out; int ssq_ld;     // skinny SK_RESIDUAL: per-16-column sums of squares of the stored values
    const float* ssq; const void* gain; float eps;     // skinny NORM consumer
};

int gemm_probe_version() { return kProbeVersion; }
int gemm_probe_families() { return F_COUNT; }
int gemm_probe_refused_code() { return kRefused; }

// struct layout for the ctypes mirror: [sizeof GemmArgs, sizeof ProbeArgs, offsets of GemmArgs' fields in declaration order,
// offsets of ProbeArgs' fields after g]; returns the number of values written
int gemm_probe_layout(long* out, int cap) {
#define O(f) (long)offsetof(GemmArgs, f)
#define P(f) (long)offsetof(ProbeArgs, f)
    const long v[] = {(long)sizeof(GemmArgs), (long)sizeof(ProbeArgs),
                      O(A), O(lda), O(M), O(a_rows), O(m_lo), O(n_taps), O(tap_off), O(Cin), O(W), O(N), O(bias), O(bias_mod), O(scale),
                      O(res), O(ldr), O(Y), O(ldy), O(act), O(sn_a), O(sn_ib), O(Y2), O(act2), O(ws), O(ws_floats), O(ksplit), O(n_seg),
                      O(a_seg), O(y_seg), O(r_seg), O(glds_min_wgs), O(big_pair), O(Wp), O(Wi), O(no_skinny), O(glds_cap8), O(chain),
                      O(glds_waves), O(xcd_map), O(epi_legacy),
                      P(g2), P(y), P(rb_force), P(mt), P(ssq_out), P(ssq_ld), P(ssq), P(gain), P(eps)};
#undef O
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

// ---- guards: the conditions under which the product would pick the family -----------------------------------------------
bool plain_ok(const GemmArgs& a) { return a.act == 0 && !a.scale && !a.res && !a.Y2; }
// the arguments a tile family sees for storage type te (gemm_launch<bfs_t>: the [rows][2 C] bf16 image against K-duplicated weights)
GemmArgs kernel_units(const GemmArgs& a, int te) {
    GemmArgs b = a;
    if (te == TE_BFS) { b.lda = 2 * a.lda; b.Cin = 2 * a.Cin; b.a_seg = 2 * a.a_seg; b.ws = nullptr; }
    return b;
}
bool skinny_common_ok(const ProbeArgs& p, int te) {
    const GemmArgs& a = p.g;
    return te == TE_BF16 && a.n_taps == 1 && a.tap_off[0] == 0 && a.m_lo == 0 && a.n_seg <= 1 && a.M >= 1 && a.M <= kSkinnyMaxRows &&
           a.a_rows >= a.M && a.act == 0 && !a.bias && !a.scale && !a.Y2 && skinny_k_ok(a.Cin) && a.N % 32 == 0 && a.lda % 8 == 0 &&
           (!a.Wp || skinny_pack_ok(a.N, a.Cin)) && p.mt >= 0;
}
bool skinny_rb_ok(int rb, int N, int K) {
    const int groups1 = N / 16;
    if (rb == 0 || rb == 1) return true;
    if (rb == 2) return K <= 3072 && groups1 % 2 == 0;
    if (rb == 3) return K <= 2048 && groups1 % 3 == 0;
    return false;
}

bool admits(int fam, int te, const ProbeArgs& p) {
    const GemmArgs& a0 = p.g;
    if (te < TE_BF16 || te > TE_F32 || fam < 0 || fam >= F_COUNT) return false;
    if (!a0.W || a0.M < 0 || a0.m_lo < 0 || a0.N <= 0 || a0.Cin <= 0 || a0.n_taps < 1 || a0.n_taps > kMaxTaps || a0.bias_mod <= 0) return false;
    if (a0.n_seg > 1 && fam != F_LAUNCH && (a0.ws || a0.ksplit > 1)) return false;
    const GemmArgs a = kernel_units(a0, te);
    const bool tile_te = te == TE_BF16 || te == TE_BFS;          // the bf16-operand families: bf16 or bf16 x 2 outputs
    const bool out = a.Y || a.Y2;
    switch (fam) {
        case F_CONV_64x64:
            if (te == TE_F32) return out && a.act != 2;          // the fp32 parity tile (no SwiGLU pairs in fp32 callers)
            return out && (a.act != 2 || a.Y);
        case F_CONV_128x64:
            return tile_te && out && (a.act != 2 || a.Y);
        case F_CONV_64x32: case F_CONV_128x32: case F_CONV_128x96:
            return tile_te && out && a.act != 2;                 // TN = 1 / 3: no gate | up column pairs in one wave
        case F_SPLITK:
            // gemm_launch_te: bf16 only, one tap, no SwiGLU, and the reduce pass's epilogue (acts 0 / 1 / 3, SnakeBeta second output)
            return te == TE_BF16 && out && a.n_taps == 1 && a.n_seg <= 1 && a.ws && a.ksplit >= 2 && a.ksplit <= 8 &&
                   a.Cin % (a.ksplit * 32) == 0 && (long)a.ksplit * (a.M - a.m_lo) * a.N <= a.ws_floats &&
                   (a.act == 0 || a.act == 1 || a.act == 3) && (!a.Y2 || a.act2 == 0);
        case F_GLDS4_128x64_S2:
            return tile_te && out && a.N % 64 == 0 && a.Cin % 64 == 0 && (a.act != 2 || a.Y) && a.ksplit <= 1;
        case F_GLDS8_64x128_S3:
            if (a.N % 128) return false;
            [[fallthrough]];
        case F_GLDS8_64x64_S3: case F_GLDS8_128x64_S3: case F_GLDS8_128x64_S2:
            return tile_te && out && a.N % 64 == 0 && a.Cin % 64 == 0 && a.act != 2 && a.ksplit <= 1 && !a.epi_legacy;
        case F_CHAIN_8x8: case F_CHAIN_16x4:
            return tile_te && out && chain_ok(a);
        case F_BIG_TR_PAIR: case F_BIG_TR_RING: case F_BIG_TR_128:
            // register-layout (transposed) epilogue: plain bf16 outputs, bias at most (SwiGLU only through gemm_swiglu_halves), and only
            // at the widths gemm_launch sends there (big_go: N % 256 == 0; the 256 x 128 tile: N % 128 == 0)
            if (te != TE_BF16 || !a.Y || !plain_ok(a) || a.Cin % 32) return false;
            if (fam == F_BIG_TR_PAIR) return a.Cin % 64 == 0 && a.N % kBigBN == 0;
            if (fam == F_BIG_TR_128) return a.N % 128 == 0;
            return a.N % kBigBN == 0;
        case F_BIG_PAIR: case F_BIG_RING: case F_BIG_128:
            if (!tile_te || !out || a.act == 2 || a.Cin % 32) return false;
            if (fam == F_BIG_PAIR) return a.Cin % 64 == 0;
            if (fam == F_BIG_128) return a.N % 128 == 0;
            return true;
        case F_SKINNY:
            if (!skinny_common_ok(p, te) || !a.Y || a.ldy % 4 || (a.res && a.ldr % 4) || !skinny_rb_ok(p.rb_force, a.N, a.Cin)) return false;
            if (p.ssq_out && (!a.res || p.ssq_ld < a.N / 16)) return false;
            if (p.ssq) return !a.res && p.gain && skinny_norm_ok(a.Cin, a.M);
            return true;
        case F_SKINNY_SWIGLU:
            if (!skinny_common_ok(p, te) || !p.y || a.res || (a.N / 2) % 8 || p.ssq_out || !skinny_rb_ok(p.rb_force, a.N, a.Cin)) return false;
            if (p.ssq) return p.gain && skinny_norm_ok(a.Cin, a.M);
            return true;
        case F_SWIGLU_HALVES:
            return te != TE_BFS && a0.Y && p.y && a0.act == 0 && a0.N % 2 == 0 && !a0.Y2 && !p.ssq && !p.ssq_out;
        case F_RESUNIT:
            if (te == TE_F32) return false;
            if (te == TE_BFS) return resunit_ok<bfs_t>(a0, p.g2);
            return resunit_ok<bf16_t>(a0, p.g2);
        case F_LAUNCH:
            return out && (te != TE_F32 || a.act != 2);
    }
    return false;
}

// ---- launches -----------------------------------------------------------------------------------------------------------
template <typename TE>
void run_tile(int fam, const GemmArgs& a, hipStream_t s) {
    switch (fam) {
        case F_CONV_64x32:  gemm_go<bf16_t, 64, 32, TE>(a, s); break;
        case F_CONV_64x64:  gemm_go<bf16_t, 64, 64, TE>(a, s); break;
        case F_CONV_128x32: gemm_go<bf16_t, 128, 32, TE>(a, s); break;
        case F_CONV_128x64: gemm_go<bf16_t, 128, 64, TE>(a, s); break;
        case F_CONV_128x96: gemm_go<bf16_t, 128, 96, TE>(a, s); break;
        case F_GLDS4_128x64_S2: glds_go<64, 2, TE>(a, s); break;
        case F_GLDS8_64x128_S3: glds_go<128, 3, TE, 512, 64>(a, s); break;
        case F_GLDS8_64x64_S3:  glds_go<64, 3, TE, 512, 64>(a, s); break;
        case F_GLDS8_128x64_S3: glds_go<64, 3, TE, 512>(a, s); break;
        case F_GLDS8_128x64_S2: glds_go<64, 2, TE, 512>(a, s); break;
        case F_CHAIN_8x8:  chain_go<8, 8, TE>(a, s); break;
        case F_CHAIN_16x4: chain_go<16, 4, TE>(a, s); break;
        case F_BIG_PAIR: { GemmArgs b = a; b.big_pair = 0; big_go_t<false, kBigBN, TE>(b, s); break; }
        case F_BIG_RING: { GemmArgs b = a; b.big_pair = -1; big_go_t<false, kBigBN, TE>(b, s); break; }
        case F_BIG_128:  big_go_t<false, 128, TE>(a, s); break;
        default: break;
    }
}

int run(int fam, int te, const ProbeArgs& p, hipStream_t s) {
    const GemmArgs a = kernel_units(p.g, te);
    const int rows = a.M - a.m_lo;
    switch (fam) {
        case F_SPLITK: {
            if (rows <= 0) break;
            hipLaunchKernelGGL((conv_gemm_kernel<bf16_t, 64, 32, 8>), dim3((a.N + 31) / 32, (rows + 63) / 64, a.ksplit), dim3(256), 0, s, a);
            hipLaunchKernelGGL((splitk_reduce_kernel<bf16_t>), dim3((unsigned)(((size_t)rows * a.N + 255) / 256)), dim3(256), 0, s, a);
            break;
        }
        case F_BIG_TR_PAIR: { GemmArgs b = a; b.big_pair = 0; big_go_t<true, kBigBN>(b, s); break; }
        case F_BIG_TR_RING: { GemmArgs b = a; b.big_pair = -1; big_go_t<true, kBigBN>(b, s); break; }
        case F_BIG_TR_128:  big_go_t<true, 128>(a, s); break;
        case F_SKINNY: case F_SKINNY_SWIGLU: {
            SkinnyArgs k{};
            k.X = reinterpret_cast<const bf16_t*>(a.A); k.ldx = a.lda; k.M = a.M; k.W = reinterpret_cast<const bf16_t*>(a.W); k.N = a.N;
            k.res = reinterpret_cast<const bf16_t*>(a.res); k.ldr = a.ldr; k.Y = reinterpret_cast<bf16_t*>(a.Y); k.ldy = a.ldy;
            k.Wp = reinterpret_cast<const bf16_t*>(a.Wp); k.mt = p.mt;
            k.ssq_out = p.ssq_out; k.ssq_ld = p.ssq_ld; k.ssq = p.ssq; k.gain = reinterpret_cast<const bf16_t*>(p.gain); k.eps = p.eps;
            if (fam == F_SKINNY_SWIGLU) { k.Y = reinterpret_cast<bf16_t*>(p.y); k.ldy = a.N / 2; skinny_launch<SK_SWIGLU>(k, a.Cin, s, p.rb_force); }
            else if (a.res) skinny_launch<SK_RESIDUAL>(k, a.Cin, s, p.rb_force);
            else skinny_launch<SK_STORE>(k, a.Cin, s, p.rb_force);
            break;
        }
        case F_SWIGLU_HALVES:
            if (te == TE_F32) gemm_swiglu_halves<float>(p.g, p.y, s); else gemm_swiglu_halves<bf16_t>(p.g, p.y, s);
            break;
        case F_RESUNIT:
            if (te == TE_BFS) (void)resunit_launch<bfs_t>(p.g, p.g2, s); else (void)resunit_launch<bf16_t>(p.g, p.g2, s);
            break;
        case F_LAUNCH:
            if (te == TE_BFS) gemm_launch<bfs_t>(p.g, s); else if (te == TE_F32) gemm_launch<float>(p.g, s); else gemm_launch<bf16_t>(p.g, s);
            break;
        default:
            if (rows <= 0) break;
            if (te == TE_F32) gemm_go<float, 64, 64>(a, s);
            else if (te == TE_BFS) run_tile<bfs_t>(fam, a, s);
            else run_tile<bf16_t>(fam, a, s);
            break;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// 1 = the family's guard admits these arguments in storage type te (0 bf16, 1 bf16 x 2, 2 fp32)
int gemm_probe_admits(int fam, int te, const ProbeArgs* p) { return p && admits(fam, te, *p) ? 1 : 0; }

// launch exactly family `fam`; returns hipGetLastError() after the launch(es), or kRefused (nothing launched)
int gemm_probe_run(int fam, int te, const ProbeArgs* p, hipStream_t s) {
    if (!p || !admits(fam, te, *p)) return kRefused;
    return run(fam, te, *p, s);
}

// fragment-major (swiglu_I >= 0) or 16-row-interleaved row-major (swiglu_I < 0) copy of a bf16 [N][K] weight (fq3_api.hip's kinds)
int gemm_probe_pack(const void* W, void* P, int N, int K, int swiglu_I, hipStream_t s) {
    if (!W || !P || N <= 0 || K <= 0 || K % 8) return kRefused;
    if (swiglu_I >= 0 && !skinny_pack_ok(N, K)) return kRefused;
    if (swiglu_I < 0 && (N % 32 || -swiglu_I * 2 != N)) return kRefused;
    skinny_pack(reinterpret_cast<const bf16_t*>(W), reinterpret_cast<bf16_t*>(P), N, K, swiglu_I, s);
    return (int)hipGetLastError();
}

}  // extern "C"
