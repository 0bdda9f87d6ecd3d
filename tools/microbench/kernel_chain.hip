// Kernel-tuning harness (measurement tool, not product code): replays chains of the PRODUCT decode kernels
// (csrc/decode_kernels.cuh, csrc/sampler_wave.cuh) from a hipGraph, one kernel type per chain, at the 0.6B
// shapes, and prints wall time per launch.  Dependencies are the graph's stream-order edges; weights rotate over
// 5 copies so that no launch finds its matrix hot in L2.  No torch, no Python: ~10 s of GPU time per run.
// "entry" (only when named, ~60 s): the frame's kernels behind a by-value struct against their preloaded leading arguments.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <functional>
#include <algorithm>
#include <utility>
#include "../../faster-qwen3-tts_amd/csrc/decode_kernels.cuh"
#include "../../faster-qwen3-tts_amd/csrc/sampler.cuh"
#include "../../faster-qwen3-tts_amd/csrc/sampler_wave.cuh"
#include "../../faster-qwen3-tts_amd/csrc/batch_kernels.cuh"
using namespace fq3;

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)

static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); u += 0x7fff + ((u >> 16) & 1); return (unsigned short)(u >> 16); }
static void* dev_bf16(size_t n, float scale, float offset = 0.f) {
    std::vector<unsigned short> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = f2bf(offset + scale * ((rand() & 0xffff) / 32768.f - 1.f));
    void* d; CHK(hipMalloc(&d, n * 2)); CHK(hipMemcpy(d, h.data(), n * 2, hipMemcpyHostToDevice));
    return d;
}
static void* dev_f32(size_t n, float scale) {
    std::vector<float> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = scale * ((rand() & 0xffff) / 32768.f - 1.f);
    void* d; CHK(hipMalloc(&d, n * 4)); CHK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
    return d;
}

static hipStream_t st;
static hipEvent_t e0, e1;
static int g_reps = 20;

static double chain(const char* name, int n, const std::function<void(int)>& launch) {
    hipGraph_t g; hipGraphExec_t ge;
    CHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    for (int i = 0; i < n; ++i) launch(i);
    CHK(hipStreamEndCapture(st, &g)); CHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    for (int w = 0; w < 3; ++w) CHK(hipGraphLaunch(ge, st));
    CHK(hipStreamSynchronize(st));
    float ms = 0;
    CHK(hipEventRecord(e0, st));
    for (int r = 0; r < g_reps; ++r) CHK(hipGraphLaunch(ge, st));
    CHK(hipEventRecord(e1, st)); CHK(hipEventSynchronize(e1)); CHK(hipEventElapsedTime(&ms, e0, e1));
    CHK(hipGetLastError());
    const double us = 1e3 * ms / g_reps / n;
    printf("%-64s %7.3f us/launch   (%d launches: %.3f ms)\n", name, us, n, ms / g_reps);
    CHK(hipGraphExecDestroy(ge)); CHK(hipGraphDestroy(g));
    return us;
}

template <int NCH, int PRO, int EPI, bool NT>
static void gemv(const GemvArgs& a, int R) {
    const int grid = (a.N + 4 * R - 1) / (4 * R);
    const size_t shm = PRO == PRO_COMBINE ? (size_t)a.K * sizeof(float) : 0;
    if constexpr (MaxRows<NCH, EPI>::v >= 2) {
        if (R == 2) { gemv_launch<bf16_t, NCH, PRO, EPI, NT, 1, 2>(a, grid, shm, st); return; }
    }
    if (R != 1) { fprintf(stderr, "R=%d not built for NCH=%d\n", R, NCH); exit(2); }
    gemv_launch<bf16_t, NCH, PRO, EPI, NT, 1, 1>(a, grid, shm, st);
}

// ---- kernel entry (mode "entry"): the same bodies behind the entry every kernel of the frame had before the
// leading-argument split -- ONE by-value struct, which is never preloaded, so the wave starts by reading its kernarg segment with
// scalar loads -- against the product kernels, whose leading arguments arrive in SGPRs at wave launch.  Same arithmetic: the
// outputs of the two forms are compared bit for bit before anything is timed.
template <int NCH, int PRO, int EPI, int R>
__global__ __launch_bounds__(256) void gemv_struct_kernel(GemvArgs a) { gemv_body<bf16_t, NCH, PRO, EPI, false, 1, R>(a); }
__global__ __launch_bounds__(64) void attn_pred_struct_kernel(AttnArgs a) { attn_pred_body<bf16_t>(a); }
struct SamplePredArgs {
    const DecodeState* st; const bf16_t* logits; int V, cb; SampleCfg c_imm; const bf16_t* noise_imm; int* codes; int G;
    int64_t* out64; const bf16_t* next_emb; bf16_t* next_in; int H;
};
__global__ __launch_bounds__(256) void sample_pred_struct_kernel(SamplePredArgs a) {
    sample_pred_wave_body<bf16_t, 1>(a.st, a.logits, a.V, a.cb, a.c_imm, a.noise_imm, a.codes, a.G, a.out64, a.next_emb, a.next_in, a.H, nullptr);
}
template <int NCH, int PRO, int EPI>
static void gemv_struct(const GemvArgs& a, int R) {
    const int grid = (a.N + 4 * R - 1) / (4 * R);
    if constexpr (MaxRows<NCH, EPI>::v >= 2) {
        if (R == 2) { hipLaunchKernelGGL((gemv_struct_kernel<NCH, PRO, EPI, 2>), dim3(grid), dim3(256), 0, st, a); return; }
    }
    if (R != 1) { fprintf(stderr, "R=%d not built for NCH=%d\n", R, NCH); exit(2); }
    hipLaunchKernelGGL((gemv_struct_kernel<NCH, PRO, EPI, 1>), dim3(grid), dim3(256), 0, st, a);
}

// A / B of two chains: both graphs are built once and replayed in alternating rounds (so that clock and neighbour drift hits both),
// each round long enough to time (~0.15 s), >= 2 s of replays per side; the figure is the median round.
static hipGraphExec_t capture(int n, const std::function<void(int)>& launch) {
    hipGraph_t g; hipGraphExec_t ge;
    CHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    for (int i = 0; i < n; ++i) launch(i);
    CHK(hipStreamEndCapture(st, &g)); CHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    CHK(hipGraphDestroy(g));
    return ge;
}
static double replay_us(hipGraphExec_t ge, int reps, int n) {
    float ms = 0;
    CHK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) CHK(hipGraphLaunch(ge, st));
    CHK(hipEventRecord(e1, st)); CHK(hipEventSynchronize(e1)); CHK(hipEventElapsedTime(&ms, e0, e1));
    CHK(hipGetLastError());
    return 1e3 * ms / reps / n;
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
// returns {struct entry, preloaded entry} in us per launch; with one side only (b empty) times a alone
static std::pair<double, double> chain_ab(const char* name, int n, const std::function<void(int)>& a, const std::function<void(int)>& b) {
    hipGraphExec_t ga = capture(n, a), gb = b ? capture(n, b) : nullptr;
    for (int w = 0; w < 3; ++w) { CHK(hipGraphLaunch(ga, st)); if (gb) CHK(hipGraphLaunch(gb, st)); }
    CHK(hipStreamSynchronize(st));
    const double one = replay_us(ga, 10, n) * n;                    // us per replay
    const int reps = (int)fmax(10.0, 150e3 / one), rounds = 15;     // 15 rounds x 0.15 s = 2.25 s per side
    std::vector<double> ta, tb;
    for (int r = 0; r < rounds; ++r) { ta.push_back(replay_us(ga, reps, n)); if (gb) tb.push_back(replay_us(gb, reps, n)); }
    const double ma = median(ta), mb = gb ? median(tb) : 0.0;
    if (gb) printf("%-58s struct %7.3f  preloaded %7.3f us/launch  %+7.3f  (min %.3f / %.3f, %d x %d replays of %d)\n", name, ma, mb, mb - ma,
                   *std::min_element(ta.begin(), ta.end()), *std::min_element(tb.begin(), tb.end()), rounds, reps, n);
    else printf("%-58s        %7.3f us/launch  (min %.3f, %d x %d replays of %d)\n", name, ma, *std::min_element(ta.begin(), ta.end()), rounds, reps, n);
    CHK(hipGraphExecDestroy(ga)); if (gb) CHK(hipGraphExecDestroy(gb));
    return {ma, mb};
}

// ---- self-checks: cheap CPU references so that a 15-second harness run also catches logic errors ---------------
static float bf2f(unsigned short v) { unsigned u = (unsigned)v << 16; float f; memcpy(&f, &u, 4); return f; }
static float rbf(float f) { return bf2f(f2bf(f)); }
static std::vector<float> fetch_bf16(const void* d, size_t n) {
    std::vector<unsigned short> h(n); CHK(hipMemcpy(h.data(), d, n * 2, hipMemcpyDeviceToHost));
    std::vector<float> f(n); for (size_t i = 0; i < n; ++i) f[i] = bf2f(h[i]); return f;
}
static std::vector<float> fetch_f32(const void* d, size_t n) { std::vector<float> f(n); CHK(hipMemcpy(f.data(), d, n * 4, hipMemcpyDeviceToHost)); return f; }
static int g_fail = 0;
static void report(const char* what, double err, double tol) {
    printf("check %-52s max err %.3e (tol %.1e) %s\n", what, err, tol, err <= tol ? "ok" : "FAIL");
    if (!(err <= tol)) ++g_fail;
}
__global__ void lane_ops_kernel(float* out) {
    const int lane = threadIdx.x;
    const float v = (float)(lane * lane % 37) + 0.25f * lane;
    out[lane] = wave_sum(v); out[64 + lane] = wave_max(v); out[128 + lane] = row16_sum(v); out[192 + lane] = row16_max(v);
    out[256 + lane] = row16_xor8(v); out[320 + lane] = xrow_sum(v); out[384 + lane] = xrow_max(v); out[448 + lane] = v;
}
static void check_lane_ops() {
    float* d; CHK(hipMalloc(&d, 512 * 4));
    hipLaunchKernelGGL(lane_ops_kernel, dim3(1), dim3(64), 0, st, d); CHK(hipStreamSynchronize(st));
    auto o = fetch_f32(d, 512); const float* v = &o[448];
    double e = 0;
    float tot = 0, mx = -1e30f; for (int i = 0; i < 64; ++i) { tot += v[i]; mx = fmaxf(mx, v[i]); }
    for (int l = 0; l < 64; ++l) {
        float rs = 0, rm = -1e30f, xs = 0, xm = -1e30f;
        for (int i = 0; i < 16; ++i) { rs += v[(l & 48) + i]; rm = fmaxf(rm, v[(l & 48) + i]); }
        for (int r = 0; r < 4; ++r) { xs += v[(l & 15) + 16 * r]; xm = fmaxf(xm, v[(l & 15) + 16 * r]); }
        e = fmax(e, fabs(o[l] - tot)); e = fmax(e, fabs(o[64 + l] - mx)); e = fmax(e, fabs(o[128 + l] - rs)); e = fmax(e, fabs(o[192 + l] - rm));
        e = fmax(e, fabs(o[256 + l] - v[l ^ 8])); e = fmax(e, fabs(o[320 + l] - xs)); e = fmax(e, fabs(o[384 + l] - xm));
    }
    report("DPP / permlane-swap lane reductions", e, 1e-3);
}

// (combine_batch_kernel -- the split-KV merge as its own launch -- now lives in csrc/batch_kernels.cuh: shipped in round 2)

// ---- candidate (round 3, measured here): the code predictor's attention INSIDE its qkv GEMV by
// "last arriver": every workgroup of the GEMV releases its 8 output rows (agent-scope release: L2 write-back, the 8 XCDs do
// not share an L2), takes a ticket on the counter of the kv group its rows belong to (2 q heads + k + v = 512 rows = 64
// workgroups), and the workgroup that draws the last ticket acquires and runs the group's two one-wave attention bodies.
// Replaces the attn_pred_kernel launch (16 workgroups x 1 wave) of every predictor layer pass.
template <typename T>
__global__ __launch_bounds__(256) void qkv_attn_fused_kernel(GemvArgs a, AttnArgs at, unsigned* counters, int q_rows, int kv_rows) {
    gemv_body<T, 2, PRO_NORM, EPI_STORE, false, 1, 2>(a);
    const int row0 = blockIdx.x * 8;
    int g;
    if (row0 < q_rows) g = row0 / (at.rep * kHeadDim);
    else if (row0 < q_rows + kv_rows) g = (row0 - q_rows) / kHeadDim;
    else g = (row0 - q_rows - kv_rows) / kHeadDim;
    const unsigned per_group = (unsigned)((at.rep + 2) * kHeadDim / 8);
    __shared__ int s_last;
    __syncthreads();                                   // every wave's rows are stored (workgroup scope) before thread 0 releases them
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(&counters[g], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == per_group - 1;
        if (s_last) __hip_atomic_store(&counters[g], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch
    }
    __syncthreads();
    if (!s_last) return;
    const int wave = threadIdx.x >> 6;
    if (wave < at.rep) attn_pred_body<T>(at, g * at.rep + wave);
}
// the same GEMV with the release + ticket but NO attention: what the synchronisation alone adds to the launch
template <typename T>
__global__ __launch_bounds__(256) void qkv_ticket_only_kernel(GemvArgs a, unsigned* counters) {
    gemv_body<T, 2, PRO_NORM, EPI_STORE, false, 1, 2>(a);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(&counters[blockIdx.x >> 6], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 63u) __hip_atomic_store(&counters[blockIdx.x >> 6], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__global__ void empty_kernel(const float* p) { if (p == nullptr) __builtin_trap(); }

// ---- candidate (round 5, the round-4 review's "one bounded single-stream experiment"): the code predictor's attention recomputed
// redundantly inside its o_proj GEMV.  Every one of the 256 workgroups (here 16 waves: one per q head) runs the one-wave attention body
// of all 16 heads into LDS (<= 17 keys: ~70 KB of L2 reads per workgroup), one barrier, then the GEMV over the LDS vector (a row's K
// split over four waves, partial sums through LDS).  Replaces the attn_pred_kernel launch (16 workgroups x 1 wave, 2.75 us in a
// chain) in front of every predictor o_proj: 75 of the frame's 554 launches -- if the prologue costs less than that launch.
template <typename T>
__global__ __launch_bounds__(1024) void oproj_attn_fused_kernel(GemvArgs g, AttnArgs at) {
    __shared__ __attribute__((aligned(16))) T xs[2048];
    __shared__ float part[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row = blockIdx.x * 4 + (wave >> 2), kq = wave & 3;
    Raw8<T> wr;
    ldraw<false>(wr, reinterpret_cast<const T*>(g.W) + (size_t)row * g.K + kq * 512 + lane * 8);        // the weights first: the long pole
    const float resv = DT<T>::ld(reinterpret_cast<const T*>(g.res) + blockIdx.x * 4 + (tid & 3));
    at.out = xs;                                       // (a generic pointer into LDS: the body's stores become flat stores)
    attn_pred_body<T>(at, wave);                       // head = wave; the group's first head appends K / V (every workgroup: same values)
    __syncthreads();
    Raw8<T> xr;
    xr.v = *reinterpret_cast<const u32x4*>(xs + kq * 512 + lane * 8);
    float x[8];
    unpack(xr, x);
    float sacc = dot8<T>(wr, x, 0.f);
    sacc = wave_sum(sacc);
    if (lane == 0) part[wave] = sacc;
    __syncthreads();
    if (tid < 4) {
        const float t = ((part[tid * 4] + part[tid * 4 + 1]) + part[tid * 4 + 2]) + part[tid * 4 + 3];
        DT<T>::st(reinterpret_cast<T*>(g.y) + blockIdx.x * 4 + tid, DT<T>::rnd(t) + resv);
    }
}

int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : "";
    g_reps = argc > 2 ? atoi(argv[2]) : 20;
    auto want = [&](const char* tag) { return only[0] == 0 || strstr(tag, only) != nullptr || strcmp(only, "all") == 0; };
    srand(7);
    CHK(hipStreamCreate(&st)); CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    const int H = 1024, I = 3072, QD = 2048, KVD = 1024, NQKV = QD + 2 * KVD, Vp = 2048, Vt = 3072, NKV = 8;
    const int NL = 5;
    void *Wqkv[NL], *Wo[NL], *Wgu[NL], *Wdn[NL], *Whead[NL], *WheadT;
    for (int l = 0; l < NL; ++l) {
        Wqkv[l] = dev_bf16((size_t)NQKV * H, 1.f / sqrtf((float)H));
        Wo[l] = dev_bf16((size_t)H * QD, 1.f / sqrtf((float)QD));
        Wgu[l] = dev_bf16((size_t)2 * I * H, 1.f / sqrtf((float)H));
        Wdn[l] = dev_bf16((size_t)H * I, 1.f / sqrtf((float)I));
        Whead[l] = dev_bf16((size_t)Vp * H, 1.f / sqrtf((float)H));
    }
    WheadT = dev_bf16((size_t)Vt * H, 1.f / sqrtf((float)H));
    void* norm_w = dev_bf16(H, 0.05f, 1.f);
    void* hd_w = dev_bf16(128, 0.05f, 1.f);
    void* bufA = dev_bf16(8192, 1.f);
    void* bufB = dev_bf16(8192, 1.f);
    void* qkv = dev_bf16(NQKV, 1.f);
    void* act = dev_bf16(I, 1.f);
    void* attn_out = dev_bf16(QD, 1.f);
    float* cosr = (float*)dev_f32(128, 1.f);
    const int pred_seq = 17, talk_seq = 2048;
    void* pk = dev_bf16((size_t)NKV * pred_seq * 128, 1.f);
    void* pv = dev_bf16((size_t)NKV * pred_seq * 128, 1.f);
    void* tk[NL]; void* tv[NL];
    for (int l = 0; l < NL; ++l) { tk[l] = dev_bf16((size_t)NKV * talk_seq * 128, 1.f); tv[l] = dev_bf16((size_t)NKV * talk_seq * 128, 1.f); }
    float* part = (float*)dev_f32((size_t)NKV * kMaxWorkers * 2 * kPartStride, 0.5f);
    void* logits = dev_bf16(Vt, 3.f);
    void* noise = dev_bf16((size_t)16 * Vt, 0.4f, 0.6f);
    void* emb = dev_bf16((size_t)Vp * H, 1.f);
    int* codes; CHK(hipMalloc(&codes, 16384 * 16 * 4)); CHK(hipMemset(codes, 0, 16384 * 16 * 4));
    unsigned char* seen; CHK(hipMalloc(&seen, kMaxVocab)); CHK(hipMemset(seen, 0, kMaxVocab));
    int64_t* out64; CHK(hipMalloc(&out64, 64 * 8));
    int* pos_dev; CHK(hipMalloc(&pos_dev, 4)); { int p = 300; CHK(hipMemcpy(pos_dev, &p, 4, hipMemcpyHostToDevice)); }
    // a frozen DecodeState for the talker sampler (done = 0; frame never advances in this harness is fine for timing)
    DecodeState hs{}; hs.token = 5; hs.frame = 0; hs.pos = 300; hs.done = 0; hs.min_new = 2; hs.max_new = 4000; hs.noise_frames = 1;
    hs.eos_id = 2150; hs.max_seq = talk_seq; hs.sup_lo = Vt - 1024; hs.sup_hi = Vt; hs.t_temperature = 0.9f; hs.t_top_k = 50; hs.t_top_p = 1.f;
    hs.t_do_sample = 1; hs.t_rep_penalty = 1.05f; hs.p_temperature = 0.9f; hs.p_top_k = 50; hs.p_top_p = 1.f; hs.p_do_sample = 1;
    hs.talker_noise = noise; hs.pred_noise = noise;
    DecodeState* st_dev; CHK(hipMalloc(&st_dev, sizeof hs)); CHK(hipMemcpy(st_dev, &hs, sizeof hs, hipMemcpyHostToDevice));

    const int N = 320;
    printf("# chain of %d dependent launches per line, %d graph replays; MI355X, 0.6B predictor/talker shapes, bf16\n", N, g_reps);
    if (want("empty")) chain("empty kernel (1 wave)", N, [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, st, cosr); });

    auto qkv_args = [&](int i) { GemvArgs g{}; g.eps = 1e-6f; g.W = Wqkv[i % NL]; g.N = NQKV; g.K = H; g.x = (i & 1) ? bufB : bufA; g.norm_w = norm_w; g.y = qkv; return g; };
    auto o_args = [&](int i, int n_part) { GemvArgs g{}; g.W = Wo[i % NL]; g.N = H; g.K = QD; g.y = (i & 1) ? bufA : bufB; g.res = (i & 1) ? bufB : bufA; g.rep = 2; g.part = part; g.n_part = n_part; return g; };
    auto gu_args = [&](int i) { GemvArgs g{}; g.eps = 1e-6f; g.W = Wgu[i % NL]; g.N = I; g.K = H; g.x = (i & 1) ? bufB : bufA; g.norm_w = norm_w; g.y = act; g.up_off = I; return g; };
    auto dn_args = [&](int i) { GemvArgs g{}; g.W = Wdn[i % NL]; g.N = H; g.K = I; g.x = act; g.y = (i & 1) ? bufA : bufB; g.res = (i & 1) ? bufB : bufA; return g; };
    auto head_args = [&](int i) { GemvArgs g{}; g.eps = 1e-6f; g.W = Whead[i % NL]; g.N = Vp; g.K = H; g.x = (i & 1) ? bufB : bufA; g.norm_w = norm_w; g.y = logits; return g; };
    auto pattn_args = [&](int pos) { AttnArgs a{}; a.qkv = qkv; a.q_norm_w = hd_w; a.k_norm_w = hd_w; a.eps = 1e-6f; a.cos_row = cosr; a.sin_row = cosr + 64;
        a.kcache = pk; a.vcache = pv; a.max_seq = pred_seq; a.pos_ptr = nullptr; a.pos_imm = pos; a.n_pad = 0; a.n_kv = NKV; a.part = part; a.scale = 0.0883883f; a.rep = 2; a.out = attn_out; return a; };
    auto tattn_args = [&](int i) { AttnArgs a = pattn_args(0); a.kcache = tk[i % NL]; a.vcache = tv[i % NL]; a.max_seq = talk_seq; a.pos_ptr = pos_dev; return a; };
    SampleCfg pc{}; pc.temperature = 0.9f; pc.top_k = 50; pc.top_p = 1.f; pc.do_sample = 1; pc.rep_penalty = 1.f; pc.sup_lo = 0; pc.sup_hi = 0; pc.keep_id = -1; pc.sup_extra = -1;


    if (want("check")) {
        check_lane_ops();
        // qkv: y = W . (norm_w * rnd(x * rs)) -- compare rows against a double-precision reference
        auto Wh = fetch_bf16(Wqkv[0], (size_t)NQKV * H); auto xh = fetch_bf16(bufA, H); auto nh = fetch_bf16(norm_w, H);
        std::vector<float> xn(H); { double ss = 0; for (int i = 0; i < H; ++i) ss += (double)xh[i] * xh[i]; const float rs = 1.f / sqrtf((float)(ss / H) + 1e-6f);
            for (int i = 0; i < H; ++i) xn[i] = rbf(nh[i] * rbf(xh[i] * rs)); }
        for (int R = 1; R <= 2; ++R) {
            gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(0), R); CHK(hipStreamSynchronize(st));
            auto y = fetch_bf16(qkv, NQKV); double e = 0;
            for (int r = 0; r < NQKV; ++r) { double acc = 0; for (int i = 0; i < H; ++i) acc += (double)Wh[(size_t)r * H + i] * xn[i]; e = fmax(e, fabs(y[r] - acc) / (1.0 + fabs(acc))); }
            report(R == 1 ? "gemv NORM/STORE R=1 (qkv)" : "gemv NORM/STORE R=2 (qkv)", e, 1e-2);
        }
        {   // gate_up + SwiGLU
            auto Wg = fetch_bf16(Wgu[0], (size_t)2 * I * H);
            gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(0), 2); CHK(hipStreamSynchronize(st));
            auto y = fetch_bf16(act, I); double e = 0;
            for (int r = 0; r < I; ++r) { double g = 0, u = 0; for (int i = 0; i < H; ++i) { g += (double)Wg[(size_t)r * H + i] * xn[i]; u += (double)Wg[(size_t)(r + I) * H + i] * xn[i]; }
                const float gg = rbf((float)g), uu = rbf((float)u); const double ref = rbf(gg / (1.f + expf(-gg))) * uu; e = fmax(e, fabs(y[r] - ref) / (1.0 + fabs(ref))); }
            report("gemv NORM/SWIGLU R=2 (gate_up)", e, 1e-2);
        }
        {   // down + residual (in place on bufB <- bufA residual)
            auto Wd = fetch_bf16(Wdn[0], (size_t)H * I); auto ah = fetch_bf16(act, I); auto rh = fetch_bf16(bufA, H);
            gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(0), 1); CHK(hipStreamSynchronize(st));
            auto y = fetch_bf16(bufB, H); double e = 0;
            for (int r = 0; r < H; ++r) { double acc = 0; for (int i = 0; i < I; ++i) acc += (double)Wd[(size_t)r * I + i] * ah[i]; const double ref = rbf((float)acc) + rh[r]; e = fmax(e, fabs(y[r] - ref) / (1.0 + fabs(ref))); }
            report("gemv PLAIN/RESIDUAL R=1 (down)", e, 1e-2);
            CHK(hipMemcpy(bufB, bufA, 8192 * 2, hipMemcpyDeviceToDevice));
        }
        {   // predictor attention, pos 8, against fp32 reference with the same rounding points
            attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st); CHK(hipStreamSynchronize(st));
            auto qh = fetch_bf16(qkv, NQKV); auto wn = fetch_bf16(hd_w, 128); auto cs = fetch_f32(cosr, 128);
            auto kh = fetch_bf16(pk, (size_t)NKV * pred_seq * 128), vh = fetch_bf16(pv, (size_t)NKV * pred_seq * 128); auto out = fetch_bf16(attn_out, QD);
            auto norm_rope = [&](const float* x, float* o) { double ss = 0; for (int d = 0; d < 128; ++d) ss += (double)x[d] * x[d]; const float rs = 1.f / sqrtf((float)(ss / 128) + 1e-6f);
                float n[128]; for (int d = 0; d < 128; ++d) n[d] = rbf(wn[d] * rbf(x[d] * rs));
                for (int d = 0; d < 128; ++d) { const float rot = d < 64 ? -n[d + 64] : n[d - 64]; o[d] = rbf(rbf(n[d] * cs[d & 63]) + rbf(rot * cs[64 + (d & 63)])); } };
            double e = 0;
            for (int h = 0; h < 16; ++h) { const int g = h / 2; float q[128], kn[128];
                norm_rope(&qh[(size_t)h * 128], q); norm_rope(&qh[QD + (size_t)g * 128], kn);
                double sc[9], mx = -1e30; for (int k = 0; k < 9; ++k) { const float* kk = k < 8 ? &kh[((size_t)g * pred_seq + k) * 128] : kn; double a2 = 0; for (int d = 0; d < 128; ++d) a2 += (double)q[d] * kk[d]; sc[k] = a2 * 0.0883883; mx = fmax(mx, sc[k]); }
                double l = 0; for (int k = 0; k < 9; ++k) { sc[k] = exp(sc[k] - mx); l += sc[k]; }
                for (int d = 0; d < 128; ++d) { double o = 0; for (int k = 0; k < 9; ++k) o += sc[k] * (k < 8 ? vh[((size_t)g * pred_seq + k) * 128 + d] : qh[QD + KVD + (size_t)g * 128 + d]); o /= l;
                    e = fmax(e, fabs(out[(size_t)h * 128 + d] - o) / (1.0 + fabs(o))); } }
            report("attn_pred_kernel pos 8 (16 heads)", e, 2e-2);
            // the group's first head must have appended K (normed + roped) and V at slot 8
            auto k2 = fetch_bf16(pk, (size_t)NKV * pred_seq * 128); float kn[128]; norm_rope(&qh[QD], kn); double e2 = 0;
            for (int d = 0; d < 128; ++d) e2 = fmax(e2, fabs(k2[(size_t)8 * 128 + d] - kn[d]));
            report("attn_pred_kernel KV append (group 0)", e2, 2e-2);
        }
        {   // talker attention + COMBINE o_proj against PLAIN o_proj fed by the reference merge is covered by pytest; here: finite + sane
            attn_decode_launch<bf16_t, 2, false>(tattn_args(0), 8, st); 
            gemv<4, PRO_COMBINE, EPI_RESIDUAL, false>(o_args(0, 8), 1); CHK(hipStreamSynchronize(st));
            auto y = fetch_bf16(bufB, H); double s2 = 0; int bad = 0; for (float v : y) { if (!(fabs(v) < 1e4)) ++bad; s2 += (double)v * v; }
            report("attn_decode + COMBINE o_proj finite", bad, 0.5);
            CHK(hipMemcpy(bufB, bufA, 8192 * 2, hipMemcpyDeviceToDevice));
        }
        if (g_fail) { printf("SELF-CHECK FAILURES: %d\n", g_fail); }
    }
    if (want("qkv")) {
        chain("qkv   gemv<2,NORM,STORE>      N=4096 K=1024 R=2 grid 512", N, [&](int i) { gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(i), 2); });
        chain("qkv   gemv<2,NORM,STORE>      N=4096 K=1024 R=1 grid 1024", N, [&](int i) { gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(i), 1); });
        chain("qkv   gemv<2,NORM,STORE> NT   N=4096 K=1024 R=2 grid 512", N, [&](int i) { gemv<2, PRO_NORM, EPI_STORE, true>(qkv_args(i), 2); });
        chain("qkv   gemv<2,PLAIN,STORE>     N=4096 K=1024 R=2 grid 512 (no norm)", N, [&](int i) { gemv<2, PRO_PLAIN, EPI_STORE, false>(qkv_args(i), 2); });
    }
    if (want("pattn")) {
        chain("pattn attn_pred_kernel        16 x 64 thr, pos 8 (final output)", N, [&](int) { attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st); });
        chain("pattn attn_decode_kernel<2>    8 x 256 thr, pos 8 (1 worker)", N, [&](int) { attn_decode_launch<bf16_t, 2, false>(pattn_args(8), 1, st); });
    }
    if (want("tattn")) {
        chain("tattn attn_decode_kernel<2>    8x8 x 256 thr, pos 300 (device pos), contiguous cache", N, [&](int i) { attn_decode_launch<bf16_t, 2, false>(tattn_args(i), 8, st); });
        // the product's form: the same buffers read as a pool of 64-key blocks through a (shuffled) block table
        const int nblk = talk_seq / 64;
        std::vector<int> tab(nblk);
        for (int i = 0; i < nblk; ++i) tab[i] = (i * 7 + 3) % nblk;              // a permutation when nblk is not a multiple of 7
        int* tab_dev = nullptr;
        CHK(hipMalloc(&tab_dev, nblk * sizeof(int)));
        CHK(hipMemcpy(tab_dev, tab.data(), nblk * sizeof(int), hipMemcpyHostToDevice));
        chain("tattn attn_decode_kernel<2>    8x8 x 256 thr, pos 300 (device pos), PAGED (block table)", N, [&](int i) {
            AttnArgs a = tattn_args(i); a.table = tab_dev; a.blk_stride = NKV * 64 * 128;
            attn_decode_launch<bf16_t, 2, true>(a, 8, st); });
    }
    if (want("oproj")) {
        chain("oproj gemv<4,COMBINE,RESID>   N=1024 K=2048 R=1 grid 256, 1 part", N, [&](int i) { gemv<4, PRO_COMBINE, EPI_RESIDUAL, false>(o_args(i, 1), 1); });
        chain("oproj gemv<4,COMBINE,RESID>   N=1024 K=2048 R=1 grid 256, 8 parts", N, [&](int i) { gemv<4, PRO_COMBINE, EPI_RESIDUAL, false>(o_args(i, 8), 1); });
        chain("oproj gemv<4,PLAIN,RESID>     N=1024 K=2048 R=1 grid 256 (no combine)", N, [&](int i) { GemvArgs g = o_args(i, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); });
    }
    if (want("oattn")) {
        // correctness first: fused == attn_pred_kernel + PLAIN o_proj up to the fp32 order of the K split
        GemvArgs g0 = o_args(0, 1); g0.x = attn_out;
        attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st);
        gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g0, 1); CHK(hipStreamSynchronize(st));
        auto y_ref = fetch_bf16(g0.y, H);
        CHK(hipMemset(g0.y, 0, H * 2));
        hipLaunchKernelGGL((oproj_attn_fused_kernel<bf16_t>), dim3(H / 4), dim3(1024), 0, st, g0, pattn_args(8)); CHK(hipStreamSynchronize(st));
        auto y_f = fetch_bf16(g0.y, H);
        double e = 0; for (int r = 0; r < H; ++r) e = fmax(e, fabs(y_f[r] - y_ref[r]) / (1.0 + fabs(y_ref[r])));
        report("o_proj with the attention recomputed in every workgroup ~ attn + o_proj", e, 2e-2);
        CHK(hipMemcpy(bufB, bufA, 8192 * 2, hipMemcpyDeviceToDevice));
        const double t_pair = chain("oattn attn_pred_kernel + gemv<4,PLAIN,RESID> (the product: 2 launches per step, 160 steps)", N, [&](int i) {
            if (i & 1) { GemvArgs g = o_args(i / 2, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); }
            else attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st); });
        const double t_fused = chain("oattn o_proj with the attention inside (256 WG x 1024 thr: 1 launch per step)", N, [&](int i) {
            GemvArgs g = o_args(i, 1); g.x = attn_out;
            hipLaunchKernelGGL((oproj_attn_fused_kernel<bf16_t>), dim3(H / 4), dim3(1024), 0, st, g, pattn_args(8)); });
        printf("   -> per predictor layer: pair %.2f us, fused %.2f us: %+.2f us (x 75 launches per frame = %+.1f us of ~2060)\n", 2 * t_pair, t_fused, t_fused - 2 * t_pair,
               75 * (t_fused - 2 * t_pair));
    }
    if (want("gateup")) {
        chain("gateup gemv<2,NORM,SWIGLU>    N=3072 K=1024 R=2 grid 384", N, [&](int i) { gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(i), 2); });
        chain("gateup gemv<2,NORM,SWIGLU>    N=3072 K=1024 R=1 grid 768", N, [&](int i) { gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(i), 1); });
    }
    if (want("down")) {
        chain("down  gemv<6,PLAIN,RESID>     N=1024 K=3072 R=1 grid 256", N, [&](int i) { gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(i), 1); });
    }
    if (want("head")) {
        chain("head  gemv<2,NORM,STORE>      N=2048 K=1024 R=2 grid 256", N, [&](int i) { gemv<2, PRO_NORM, EPI_STORE, false>(head_args(i), 2); });
        chain("head  gemv<2,NORM,STORE>      N=2048 K=1024 R=1 grid 512", N, [&](int i) { gemv<2, PRO_NORM, EPI_STORE, false>(head_args(i), 1); });
    }
    if (want("sample")) {
        chain("sample sample_pred_wave_kernel<1>  V=2048 top_k=50 (immediate cfg)", N, [&](int i) {
            sample_pred_wave_launch<bf16_t, 1>((const DecodeState*)nullptr, (const bf16_t*)logits, Vp, i % 15, pc,
                                               (const bf16_t*)noise, (int*)nullptr, 16, out64, (const bf16_t*)emb, (bf16_t*)bufA, H, (const TeacherForcing*)nullptr, st); });
        chain("sample sample_pred_wave_kernel<1>  V=2048 (device state)", N, [&](int i) {
            sample_pred_wave_launch<bf16_t, 1>((const DecodeState*)st_dev, (const bf16_t*)logits, Vp, i % 15, pc,
                                               (const bf16_t*)nullptr, codes, 16, (int64_t*)nullptr, (const bf16_t*)emb, (bf16_t*)bufA, H, (const TeacherForcing*)nullptr, st); });
        chain("sample sample_talker_wave_kernel<2> V=3072 top_k=50 rep 1.05", N, [&](int) {
            sample_talker_wave_launch<bf16_t, 2>(st_dev, (const bf16_t*)logits, Vt, (const unsigned char*)seen, 16, (const TeacherForcing*)nullptr, st); });
        CHK(hipMemcpy(st_dev, &hs, sizeof hs, hipMemcpyHostToDevice));
    }
    if (want("layer")) {
        chain("layer  predictor layer x64 (qkv, attn_pred, o plain, gate_up, down)", N, [&](int j) {
            const int i = j / 5;
            switch (j % 5) {
                case 0: gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(i), 2); break;
                case 1: attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st); break;
                case 2: { GemvArgs g = o_args(i, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); } break;
                case 3: gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(i + 1), 2); break;
                default: gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(i + 1), 1); break;
            }
        });
    }

    // ---- kernel entry: by-value struct (scalar loads of the kernarg segment in front of everything) against preloaded leading arguments.
    // Named only ("entry"): ~60 s of replays.  Build with KERNARG_PRELOAD=0 to see both columns read their arguments with scalar loads.
    if (strcmp(only, "entry") == 0) {
        const bf16_t* lg = (const bf16_t*)logits; const bf16_t* embp = (const bf16_t*)emb;
        void* next_in = dev_bf16(H, 0.f);
        auto o_plain = [&](int i) { GemvArgs g = o_args(i, 1); g.x = attn_out; return g; };
        auto sp_args = [&](int i) { SamplePredArgs a{}; a.st = st_dev; a.logits = lg; a.V = Vp; a.cb = i % 15; a.c_imm = pc; a.codes = codes; a.G = 16;
                                    a.next_emb = embp; a.next_in = (bf16_t*)next_in; a.H = H; return a; };
        auto layer = [&](int j, bool pre) {
            const int i = j / 5;
            switch (j % 5) {
                case 0: pre ? gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(i), 2) : gemv_struct<2, PRO_NORM, EPI_STORE>(qkv_args(i), 2); break;
                case 1: if (pre) attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st);
                        else hipLaunchKernelGGL(attn_pred_struct_kernel, dim3(2 * NKV), dim3(64), 0, st, pattn_args(8));
                        break;
                case 2: pre ? gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(o_plain(i), 1) : gemv_struct<4, PRO_PLAIN, EPI_RESIDUAL>(o_plain(i), 1); break;
                case 3: pre ? gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(i + 1), 2) : gemv_struct<2, PRO_NORM, EPI_SWIGLU>(gu_args(i + 1), 2); break;
                default: pre ? gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(i + 1), 1) : gemv_struct<6, PRO_PLAIN, EPI_RESIDUAL>(dn_args(i + 1), 1); break;
            }
        };
        auto head_sample = [&](int j, bool pre) {
            const int i = j / 2;
            if (!(j & 1)) { pre ? gemv<2, PRO_NORM, EPI_STORE, false>(head_args(i), 2) : gemv_struct<2, PRO_NORM, EPI_STORE>(head_args(i), 2); return; }
            if (pre) sample_pred_wave_launch<bf16_t, 1>(st_dev, lg, Vp, i % 15, pc, (const bf16_t*)nullptr, codes, 16, (int64_t*)nullptr, embp, (bf16_t*)next_in, H,
                                                        (const TeacherForcing*)nullptr, st);
            else hipLaunchKernelGGL(sample_pred_struct_kernel, dim3(1), dim3(256), 0, st, sp_args(i));
        };
        // self-check: two layers + head + sampler through either entry, every buffer they write compared bit for bit
        std::vector<unsigned short> a0(8192), b0(8192);
        CHK(hipMemcpy(a0.data(), bufA, 8192 * 2, hipMemcpyDeviceToHost)); CHK(hipMemcpy(b0.data(), bufB, 8192 * 2, hipMemcpyDeviceToHost));
        std::vector<float> got[2];
        for (int pre = 0; pre < 2; ++pre) {
            CHK(hipMemcpy(bufA, a0.data(), 8192 * 2, hipMemcpyHostToDevice)); CHK(hipMemcpy(bufB, b0.data(), 8192 * 2, hipMemcpyHostToDevice));
            CHK(hipMemset(codes, 0, 64 * 4)); CHK(hipMemset(next_in, 0, H * 2));
            for (int j = 0; j < 10; ++j) layer(j, pre != 0);
            for (int j = 0; j < 2; ++j) head_sample(j, pre != 0);
            CHK(hipStreamSynchronize(st));
            const std::pair<void*, int> outs[] = {{bufA, H}, {bufB, H}, {qkv, NQKV}, {attn_out, QD}, {act, I}, {logits, Vp}, {next_in, H}, {pk, NKV * pred_seq * 128}};
            for (const auto& o : outs) { auto v = fetch_bf16(o.first, o.second); got[pre].insert(got[pre].end(), v.begin(), v.end()); }
            std::vector<int> ch(16); CHK(hipMemcpy(ch.data(), codes, 64, hipMemcpyDeviceToHost));
            for (int v : ch) got[pre].push_back((float)v);
        }
        int bad = 0, nan = 0;
        for (size_t i = 0; i < got[0].size(); ++i) { bad += memcmp(&got[0][i], &got[1][i], 4) != 0; nan += !(fabs(got[1][i]) < 1e30f); }
        report("preloaded entry == struct entry (2 layers, head, sampler: bitwise)", bad, 0.5);
        report("  ... and every value finite", nan, 0.5);
        CHK(hipMemcpy(bufA, a0.data(), 8192 * 2, hipMemcpyHostToDevice)); CHK(hipMemcpy(bufB, b0.data(), 8192 * 2, hipMemcpyHostToDevice));

        // the two glue kernels of the frame, against their definition
        const int rope_rows = 512;
        float* rope_tab = (float*)dev_f32((size_t)2 * rope_rows * 64, 1.f); float* rope_now = (float*)dev_f32(128, 0.f);
        void* pad = dev_bf16(H, 1.f); void* past = dev_bf16(H, 1.f); void* hold = dev_bf16(H, 0.f); void* pred_in = dev_bf16(2 * H, 0.f); void* xin = dev_bf16(H, 0.f);
        DecodeState hg = hs; hg.tts_pad = pad;
        CHK(hipMemcpy(st_dev, &hg, sizeof hg, hipMemcpyHostToDevice)); CHK(hipMemset(codes, 0, 64 * 4));
        // 16 tables inside one allocation, table g from row 64 g on: any id below Vp (the samplers' range) stays inside it
        void* emb16 = dev_bf16((size_t)(Vp + 16 * 64) * H, 1.f);
        EmbTables tabs{}; for (int g = 0; g < 16; ++g) tabs.t[g] = (const bf16_t*)emb16 + (size_t)g * 64 * H;
        auto fb = [&]() { frame_begin_launch<bf16_t>(st_dev, embp, (const bf16_t*)past, (bf16_t*)hold, (bf16_t*)pred_in, codes, seen, H, 16, st); };
        auto es = [&]() { embed_sum_launch<bf16_t, 16>(st_dev, tabs, codes, (bf16_t*)xin, H, rope_tab, rope_tab + (size_t)rope_rows * 64, rope_rows, 3, rope_now, st); };
        fb(); es(); CHK(hipStreamSynchronize(st));
        {
            auto pin = fetch_bf16(pred_in, 2 * H), ph = fetch_bf16(past, H), em = fetch_bf16(emb, (size_t)Vp * H), e16 = fetch_bf16(emb16, (size_t)(Vp + 16 * 64) * H), pd = fetch_bf16(pad, H), x = fetch_bf16(xin, H);
            auto rt = fetch_f32(rope_tab, (size_t)2 * rope_rows * 64), rn = fetch_f32(rope_now, 128);
            std::vector<int> ch(16); CHK(hipMemcpy(ch.data(), codes, 64, hipMemcpyDeviceToHost));
            double e = ch[0] == hs.token ? 0 : 1;
            for (int i = 0; i < H; ++i) { e = fmax(e, fabs(pin[i] - ph[i])); e = fmax(e, fabs(pin[H + i] - em[(size_t)hs.token * H + i])); }
            report("frame_begin_kernel: first id recorded, predictor input", e, 0);
            double e2 = 0;
            for (int i = 0; i < H; ++i) {
                float sum = 0.f;
                for (int g = 0; g < 16; ++g) sum += e16[((size_t)g * 64 + ch[g]) * H + i];
                e2 = fmax(e2, fabs(x[i] - rbf(rbf(sum) + pd[i])));
            }
            for (int i = 0; i < 64; ++i) { e2 = fmax(e2, fabs(rn[i] - rt[(size_t)303 * 64 + i])); e2 = fmax(e2, fabs(rn[64 + i] - rt[(size_t)(rope_rows + 303) * 64 + i])); }
            report("embed_sum_kernel: 16-row sum + pad row, RoPE row of pos + delta", e2, 0.13);      // one bf16 ulp at |x| < 32
        }
        if (g_fail) { printf("SELF-CHECK FAILURES: %d\n", g_fail); }

        printf("# kernel entry: chains of %d dependent launches, medians of 15 alternating rounds, >= 2 s of replays per side\n", N);
        chain_ab("empty kernel node (1 wave)", N, [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, st, cosr); }, nullptr);
        auto [l0, l1] = chain_ab("predictor layer x64: qkv, attn_pred, o plain, gate_up, down", N, [&](int j) { layer(j, false); }, [&](int j) { layer(j, true); });
        printf("   -> per five-launch layer: struct %.3f us, preloaded %.3f us: %+.3f us (go / no-go line: -0.5 us)\n", 5 * l0, 5 * l1, 5 * (l1 - l0));
        auto [h0, h1] = chain_ab("head gemv<2,NORM,STORE> + sample_pred_wave_kernel x160", N, [&](int j) { head_sample(j, false); }, [&](int j) { head_sample(j, true); });
        printf("   -> per head + sampler pair: struct %.3f us, preloaded %.3f us: %+.3f us\n", 2 * h0, 2 * h1, 2 * (h1 - h0));
        for (int k = 0; k < 5; ++k) {
            const char* nm[5] = {"  qkv     gemv<2,NORM,STORE> R=2", "  attn    attn_pred_kernel 16 x 64 thr, pos 8", "  o_proj  gemv<4,PLAIN,RESID> R=1", "  gate_up gemv<2,NORM,SWIGLU> R=2",
                                 "  down    gemv<6,PLAIN,RESID> R=1"};
            chain_ab(nm[k], N, [&](int j) { layer(5 * j + k, false); }, [&](int j) { layer(5 * j + k, true); });
        }
        chain_ab("  sample_pred_wave_kernel<1> V=2048 (device state)", N, [&](int j) { head_sample(2 * j + 1, false); }, [&](int j) { head_sample(2 * j + 1, true); });
        chain_ab("frame_begin_kernel (preloaded entry only)", N, [&](int) { fb(); }, nullptr);
        chain_ab("embed_sum_kernel<16> (preloaded entry only)", N, [&](int) { es(); }, nullptr);
        CHK(hipMemcpy(st_dev, &hs, sizeof hs, hipMemcpyHostToDevice));
    }

    // ---- round-3 candidates for the single-stream frame (measured negative / positive results go to DESIGN.md 4.1) ----
    if (want("fuse")) {
        unsigned* counters; CHK(hipMalloc(&counters, 64 * 4)); CHK(hipMemset(counters, 0, 64 * 4));
        void* attn_ref = dev_bf16(QD, 0.f);
        void* pk2 = dev_bf16((size_t)NKV * pred_seq * 128, 1.f); void* pv2 = dev_bf16((size_t)NKV * pred_seq * 128, 1.f);
        CHK(hipMemcpy(pk2, pk, (size_t)NKV * pred_seq * 128 * 2, hipMemcpyDeviceToDevice)); CHK(hipMemcpy(pv2, pv, (size_t)NKV * pred_seq * 128 * 2, hipMemcpyDeviceToDevice));
        // reference: the two product launches
        gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(0), 2);
        { AttnArgs a = pattn_args(8); a.out = attn_ref; a.kcache = pk2; a.vcache = pv2; attn_pred_launch<bf16_t>(a, 2 * NKV, st); }
        CHK(hipStreamSynchronize(st));
        auto ref_o = fetch_bf16(attn_ref, QD); auto ref_k = fetch_bf16(pk2, (size_t)NKV * pred_seq * 128);
        CHK(hipMemset(qkv, 0, (size_t)NQKV * 2)); CHK(hipMemset(attn_out, 0, (size_t)QD * 2));
        for (int rep = 0; rep < 3; ++rep)               // several launches: the counters must re-arm themselves
            hipLaunchKernelGGL((qkv_attn_fused_kernel<bf16_t>), dim3(NQKV / 8), dim3(256), 0, st, qkv_args(0), pattn_args(8), counters, QD, KVD);
        CHK(hipStreamSynchronize(st));
        auto got_o = fetch_bf16(attn_out, QD); auto got_k = fetch_bf16(pk, (size_t)NKV * pred_seq * 128);
        int bad = 0; for (int i = 0; i < QD; ++i) bad += got_o[i] != ref_o[i];
        for (size_t i = 0; i < got_k.size(); ++i) bad += got_k[i] != ref_k[i];
        report("fused qkv GEMV + last-arriver attention == qkv, attn_pred (bitwise)", bad, 0.5);
        chain("fuse   qkv gemv, then attn_pred_kernel (2 launches per step)", N, [&](int j) {
            if (j & 1) attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st); else gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(j / 2), 2); });
        chain("fuse   qkv gemv + release/ticket only (no attention)", N, [&](int j) {
            hipLaunchKernelGGL((qkv_ticket_only_kernel<bf16_t>), dim3(NQKV / 8), dim3(256), 0, st, qkv_args(j), counters); });
        chain("fuse   qkv gemv + last-arriver attention (1 launch per step)", N, [&](int j) {
            hipLaunchKernelGGL((qkv_attn_fused_kernel<bf16_t>), dim3(NQKV / 8), dim3(256), 0, st, qkv_args(j), pattn_args(8), counters, QD, KVD); });
        chain("fuse   predictor layer x64, 5 launches (qkv, attn_pred, o, gate_up, down)", N, [&](int j) {
            const int i = j / 5;
            switch (j % 5) {
                case 0: gemv<2, PRO_NORM, EPI_STORE, false>(qkv_args(i), 2); break;
                case 1: attn_pred_launch<bf16_t>(pattn_args(8), 2 * NKV, st); break;
                case 2: { GemvArgs g = o_args(i, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); } break;
                case 3: gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(i + 1), 2); break;
                default: gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(i + 1), 1); break;
            } });
        chain("fuse   predictor layer x80, 4 launches (qkv+attn fused, o, gate_up, down)", N, [&](int j) {
            const int i = j / 4;
            switch (j % 4) {
                case 0: hipLaunchKernelGGL((qkv_attn_fused_kernel<bf16_t>), dim3(NQKV / 8), dim3(256), 0, st, qkv_args(i), pattn_args(8), counters, QD, KVD); break;
                case 1: { GemvArgs g = o_args(i, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); } break;
                case 2: gemv<2, PRO_NORM, EPI_SWIGLU, false>(gu_args(i + 1), 2); break;
                default: gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(i + 1), 1); break;
            } });
        // (ii) what a dependent GEMV step can cost at best: the talker o_proj (4.2 MB) / down (6.3 MB) against the empty node
        chain("fuse   empty kernel node", N, [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, st, cosr); });
        chain("fuse   o_proj PLAIN R=1 grid 256 (4.2 MB)", N, [&](int i) { GemvArgs g = o_args(i, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); });
        chain("fuse   o_proj PLAIN R=1 nontemporal loads", N, [&](int i) { GemvArgs g = o_args(i, 1); g.x = attn_out; gemv<4, PRO_PLAIN, EPI_RESIDUAL, true>(g, 1); });
        chain("fuse   o_proj COMBINE 8 parts R=1 (talker)", N, [&](int i) { gemv<4, PRO_COMBINE, EPI_RESIDUAL, false>(o_args(i, 8), 1); });
        chain("fuse   down PLAIN R=1 grid 256 (6.3 MB)", N, [&](int i) { gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(dn_args(i), 1); });
        chain("fuse   down PLAIN R=1 nontemporal loads", N, [&](int i) { gemv<6, PRO_PLAIN, EPI_RESIDUAL, true>(dn_args(i), 1); });
    }

    // ---- batched decode (csrc/batch_kernels.cuh): B tokens share one pass over the weights ----
    if (want("batch")) {
        constexpr int MB = kMaxLanes;
        void* xb = dev_bf16((size_t)MB * 8192, 1.f);          // [B][8192] activations in
        void* yb = dev_bf16((size_t)MB * 8192, 1.f);          // batch kernel out
        void* y1 = dev_bf16((size_t)MB * 8192, 1.f);          // reference: B single-token launches of the product kernels
        void* ym = dev_bf16((size_t)MB * 8192, 1.f);          // MFMA kernel out
        void* bias = dev_bf16(8192, 0.3f);
        void* xn8 = dev_bf16((size_t)MB * 8192, 0.f);
        void** xn_tab = nullptr;                               // device table of the per-lane xn_out rows (BatchGemvArgs::xn_out)
        {
            std::vector<void*> h(MB);
            for (int m = 0; m < MB; ++m) h[m] = (bf16_t*)xn8 + (size_t)m * 8192;
            CHK(hipMalloc((void**)&xn_tab, MB * sizeof(void*)));
            CHK(hipMemcpy(xn_tab, h.data(), MB * sizeof(void*), hipMemcpyHostToDevice));
        }
        const size_t pstride = (size_t)NKV * kMaxWorkers * 4 * kPartStride;
        float* part8 = (float*)dev_f32((size_t)MB * pstride, 0.5f);
        {   // make the softmax denominators of the synthetic partial slots positive (l in [0.5, 1.5))
            const size_t n = (size_t)MB * pstride;
            std::vector<float> hp(n); CHK(hipMemcpy(hp.data(), part8, n * 4, hipMemcpyDeviceToHost));
            for (size_t s0 = 0; s0 + kPartStride <= n; s0 += kPartStride) hp[s0 + kHeadDim + 1] = 1.0f + hp[s0 + kHeadDim + 1];
            CHK(hipMemcpy(part8, hp.data(), n * 4, hipMemcpyHostToDevice));
        }
        auto bargs = [&](int kind, int i, int B, void* y) {
            BatchGemvArgs g{}; g.B = B; g.eps = 1e-6f; g.norm_w = norm_w; g.x = xb; g.x_stride = 8192; g.y = y; g.y_stride = 8192; g.res = xb; g.res_stride = 8192;
            if (kind == 0) { g.W = Wqkv[i % NL]; g.N = NQKV; g.K = H; }
            else if (kind == 1) { g.W = Wo[i % NL]; g.N = H; g.K = QD; }
            else if (kind == 2) { g.W = Wgu[i % NL]; g.N = I; g.K = H; g.up_off = I; }
            else if (kind == 3) { g.W = Wdn[i % NL]; g.N = H; g.K = I; }
            else { g.W = Whead[i % NL]; g.N = Vp; g.K = H; g.bias = bias; g.xn_out = xn_tab; } // head + bias + xn_out
            return g;
        };
        auto run_v = [&](int kind, int i, int B, void* y) {      // VALU batch kernel (bit-identical to single-token launches)
            BatchGemvArgs g = bargs(kind, i, B, y);
            g.group = B < kGroupLanes ? B : kGroupLanes;
            const int grid = (g.N + 3) / 4; const size_t shm = (size_t)g.group * g.K * 2;
            if (kind == 0) hipLaunchKernelGGL((gemv_batch_kernel<bf16_t, 2, PRO_NORM, EPI_STORE>), dim3(grid), dim3(256), shm, st, g);
            else if (kind == 1) hipLaunchKernelGGL((gemv_batch_kernel<bf16_t, 4, PRO_PLAIN, EPI_RESIDUAL>), dim3(grid), dim3(256), shm, st, g);
            else if (kind == 2) hipLaunchKernelGGL((gemv_batch_kernel<bf16_t, 2, PRO_NORM, EPI_SWIGLU>), dim3(grid), dim3(256), shm, st, g);
            else if (kind == 3) hipLaunchKernelGGL((gemv_batch_kernel<bf16_t, 6, PRO_PLAIN, EPI_RESIDUAL>), dim3(grid), dim3(256), shm, st, g);
            else hipLaunchKernelGGL((gemv_batch_kernel<bf16_t, 2, PRO_NORM, EPI_STORE>), dim3(grid), dim3(256), shm, st, g);
        };
        auto run_m = [&](int kind, int i, int B, void* y) {      // matrix-core batch kernels
            BatchGemvArgs g = bargs(kind, i, B, y);
            const int grid = (g.N + 15) / 16; const int NRr = kind == 2 ? 2 : 1;
            const size_t shm = (((size_t)kTokTile * (g.K + 8) * 2 + 15) & ~(size_t)15) + (size_t)4 * NRr * 256 * 4;
            if (B <= kTokTile) {
                if (kind == 0) hipLaunchKernelGGL((gemv_batch_mfma_norm_kernel<8, EPI_STORE, 1>), dim3(grid), dim3(256), shm, st, g);
                else if (kind == 1) hipLaunchKernelGGL((gemv_batch_mfma_plain_kernel<8, 8, EPI_RESIDUAL, 1>), dim3(grid), dim3(512), 0, st, g);
                else if (kind == 2) hipLaunchKernelGGL((gemv_batch_mfma_norm_kernel<8, EPI_SWIGLU, 1>), dim3(grid), dim3(256), shm, st, g);
                else if (kind == 3) hipLaunchKernelGGL((gemv_batch_mfma_plain_kernel<12, 8, EPI_RESIDUAL, 1>), dim3(grid), dim3(512), 0, st, g);
                else hipLaunchKernelGGL((gemv_batch_mfma_norm_kernel<8, EPI_STORE, 1>), dim3(grid), dim3(256), shm, st, g);
            } else {
                if (kind == 0) hipLaunchKernelGGL((gemv_batch_mfma_norm_kernel<8, EPI_STORE, 2>), dim3(grid), dim3(256), shm, st, g);
                else if (kind == 1) hipLaunchKernelGGL((gemv_batch_mfma_plain_kernel<8, 8, EPI_RESIDUAL, 2>), dim3(grid), dim3(512), 0, st, g);
                else if (kind == 2) hipLaunchKernelGGL((gemv_batch_mfma_norm_kernel<8, EPI_SWIGLU, 2>), dim3(grid), dim3(256), shm, st, g);
                else if (kind == 3) hipLaunchKernelGGL((gemv_batch_mfma_plain_kernel<12, 8, EPI_RESIDUAL, 2>), dim3(grid), dim3(512), 0, st, g);
                else hipLaunchKernelGGL((gemv_batch_mfma_norm_kernel<8, EPI_STORE, 2>), dim3(grid), dim3(256), shm, st, g);
            }
        };
        auto run_1 = [&](int kind, int i, int m) {                // product single-token kernels, token m of the same buffers
            GemvArgs g{}; g.eps = 1e-6f; g.norm_w = norm_w;
            g.x = (const bf16_t*)xb + (size_t)m * 8192; g.y = (bf16_t*)y1 + (size_t)m * 8192; g.res = (const bf16_t*)xb + (size_t)m * 8192;
            if (kind == 0) { g.W = Wqkv[i % NL]; g.N = NQKV; g.K = H; gemv<2, PRO_NORM, EPI_STORE, false>(g, 2); }
            else if (kind == 1) { g.W = Wo[i % NL]; g.N = H; g.K = QD; gemv<4, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); }
            else if (kind == 2) { g.W = Wgu[i % NL]; g.N = I; g.K = H; g.up_off = I; gemv<2, PRO_NORM, EPI_SWIGLU, false>(g, 2); }
            else if (kind == 3) { g.W = Wdn[i % NL]; g.N = H; g.K = I; gemv<6, PRO_PLAIN, EPI_RESIDUAL, false>(g, 1); }
            else if (kind == 4) { g.W = Wo[i % NL]; g.N = H; g.K = QD; g.part = part8 + (size_t)m * pstride; g.n_part = 8; g.rep = 2; gemv<4, PRO_COMBINE, EPI_RESIDUAL, false>(g, 1); }
            else { g.W = Whead[i % NL]; g.N = Vp; g.K = H; g.bias = bias; gemv<2, PRO_NORM, EPI_STORE, false>(g, 2); }
        };
        const char* kn[6] = {"qkv NORM/STORE", "o PLAIN/RESID", "gate_up NORM/SWIGLU", "down PLAIN/RESID", "", "head NORM/STORE+bias+xn_out"};
        const int outn[6] = {NQKV, H, I, H, H, Vp};
        for (int B : {32, 27, 16, 11, 8, 3}) for (int kind = 0; kind < 6; ++kind) {
            if (kind == 4) continue;
            CHK(hipMemset(yb, 0, (size_t)MB * 8192 * 2)); CHK(hipMemset(ym, 0, (size_t)MB * 8192 * 2)); CHK(hipMemset(y1, 0, (size_t)MB * 8192 * 2));
            run_v(kind, 0, B, yb); run_m(kind, 0, B, ym);
            for (int m = 0; m < B; ++m) run_1(kind, 0, m);
            CHK(hipStreamSynchronize(st));
            auto av = fetch_bf16(yb, (size_t)MB * 8192), am = fetch_bf16(ym, (size_t)MB * 8192), a1 = fetch_bf16(y1, (size_t)MB * 8192);
            int bad = 0; double e = 0;
            for (int m = 0; m < MB; ++m) for (int r = 0; r < outn[kind]; ++r) {
                const size_t ix = (size_t)m * 8192 + r;
                bad += av[ix] != a1[ix];                          // rows of lanes >= B must stay untouched (0) in all three
                e = fmax(e, fabs(am[ix] - a1[ix]) / (1.0 + fabs(a1[ix])));
            }
            char nm[112]; snprintf(nm, sizeof nm, "batch VALU B=%d %s == single-token", B, kn[kind]); report(nm, bad, 0.5);
            snprintf(nm, sizeof nm, "batch MFMA B=%d %s ~ single-token", B, kn[kind]); report(nm, e, 1e-2);
        }
        {   // merge kernel + PLAIN o_proj (the batch chain's pair) must equal the single-stream COMBINE o_proj bit for bit (VALU kernel)
            void* merged = dev_bf16((size_t)MB * 8192, 0.f);
            const int B = 32;
            CHK(hipMemset(yb, 0, (size_t)MB * 8192 * 2)); CHK(hipMemset(y1, 0, (size_t)MB * 8192 * 2));
            hipLaunchKernelGGL((combine_batch_kernel<bf16_t>), dim3((QD / 8 + 255) / 256, B), dim3(256), 0, st, (const float*)part8, pstride, 8, 2, QD, (bf16_t*)merged, 8192);
            { BatchGemvArgs g = bargs(1, 0, B, yb); g.x = merged; g.x_stride = 8192; g.group = kGroupLanes;
              hipLaunchKernelGGL((gemv_batch_kernel<bf16_t, 4, PRO_PLAIN, EPI_RESIDUAL>), dim3((g.N + 3) / 4), dim3(256), (size_t)g.group * g.K * 2, st, g); }
            for (int m = 0; m < B; ++m) run_1(4, 0, m);
            CHK(hipStreamSynchronize(st));
            auto a0 = fetch_bf16(yb, (size_t)MB * 8192), a2 = fetch_bf16(y1, (size_t)MB * 8192);
            int bad = 0; for (int m = 0; m < B; ++m) for (int r = 0; r < H; ++r) bad += a0[(size_t)m * 8192 + r] != a2[(size_t)m * 8192 + r];
            report("merge kernel + PLAIN o_proj == single-stream COMBINE o_proj (B=32)", bad, 0.5);
        }
        chain("batch  B=1 (single-token product kernels): qkv, o, gate_up, down x80", N, [&](int j) { run_1(j % 4, j / 4, 0); });
        for (int B : {8, 16, 32}) {
            char nm[112];
            snprintf(nm, sizeof nm, "batch  B=%d VALU kernel: qkv, o, gate_up, down x80", B); chain(nm, N, [&](int j) { run_v(j % 4, j / 4, B, yb); });
            snprintf(nm, sizeof nm, "batch  B=%d MFMA kernels: qkv, o, gate_up, down x80", B); chain(nm, N, [&](int j) { run_m(j % 4, j / 4, B, ym); });
            const char* one[4] = {"qkv NORM", "o PLAIN (8 waves)", "gate_up NORM/SWIGLU", "down PLAIN (8 waves)"};
            for (int kind = 0; kind < 4; ++kind) {
                snprintf(nm, sizeof nm, "batch  B=%d MFMA %s alone", B, one[kind]); chain(nm, N, [&](int j) { run_m(kind, j, B, ym); });
            }
        }
        {   // round 4: the two-panel form of the normalising GEMVs at 17..32 lanes (both token tiles prepared before the first MFMA)
            const int B = 32;
            auto run_d = [&](int kind, int i, void* y) {
                BatchGemvArgs g = bargs(kind, i, B, y);
                const int grid = (g.N + 15) / 16; const int NRr = kind == 2 ? 2 : 1;
                const size_t shm2 = (((size_t)2 * kTokTile * (g.K + 8) * 2 + 15) & ~(size_t)15) + (size_t)2 * 4 * NRr * 256 * 4;
                if (kind == 2) {
                    auto k = gemv_batch_mfma_norm_kernel<8, EPI_SWIGLU, 2, true>;
                    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm2);
                    hipLaunchKernelGGL(k, dim3(grid), dim3(256), shm2, st, g);
                } else {
                    auto k = gemv_batch_mfma_norm_kernel<8, EPI_STORE, 2, true>;
                    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm2);
                    hipLaunchKernelGGL(k, dim3(grid), dim3(256), shm2, st, g);
                }
            };
            for (int kind : {0, 2, 5}) {
                CHK(hipMemset(yb, 0, (size_t)MB * 8192 * 2)); CHK(hipMemset(ym, 0, (size_t)MB * 8192 * 2));
                run_m(kind, 0, B, ym); run_d(kind, 0, yb); CHK(hipStreamSynchronize(st));
                auto a0 = fetch_bf16(ym, (size_t)MB * 8192), a1 = fetch_bf16(yb, (size_t)MB * 8192);
                int bad = 0; for (size_t i = 0; i < a0.size(); ++i) bad += a0[i] != a1[i];
                char nm[112]; snprintf(nm, sizeof nm, "batch MFMA B=32 %s: two panels == one panel (bit for bit)", kn[kind]); report(nm, bad, 0.5);
            }
            chain("batch  B=32 MFMA qkv NORM alone, two panels", N, [&](int j) { run_d(0, j, ym); });
            chain("batch  B=32 MFMA gate_up NORM/SWIGLU alone, two panels", N, [&](int j) { run_d(2, j, ym); });
        }
    }
    return g_fail ? 1 : 0;
}
