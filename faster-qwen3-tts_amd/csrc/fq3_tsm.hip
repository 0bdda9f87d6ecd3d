// Time-scale modification behind the C ABI: the `speed` of a stream, applied to the vocoder's float32 PCM in front of the audio
// output stage (fq3_audio.hip).  Duration changes, pitch does not.
//   fq3_tsm_design / _count   host only (no HIP call): the parameters and window of a rate, and the stream's output count
//   fq3_tsm_create / _push    streaming WSOLA (waveform-similarity overlap-add, plain cross-correlation search), ONE launch per push
//   fq3_tsm_push_group        the pushes of up to 32 objects of one in_rate in ONE launch (a workgroup per row), each row its single push
//
// P = speed in per-mille, Hs = round(in_rate / 100), N = 2 Hs, D = Hs, w = periodic Hann of length N.  With x = 0 outside the stream:
//     a(s) = floor(s Hs P / 1000)          pos(s) = a(s) + delta(s)          pos(-1) = -Hs          delta(0) = 0
//     s >= 1:  t[j] = x[pos(s-1) + Hs + j],  c(d) = sum_j x[a(s) + d + j] t[j]  (j in [0, N)),  delta(s) = argmax over d in [-D, D],
//              ties to the smallest d
//     y[s Hs + j] = fmaf(w[j], x[pos(s) + j], w[j + Hs] x[pos(s-1) + Hs + j])          j in [0, Hs)
// A finished stream of n samples has T(n) = ceil(1000 n / P) outputs.  An unfinished one has whole segments only: segment s >= 1 once
// need(s) = max(a(s), a(s-1) + Hs) + D + N <= n (every sample any candidate could read exists; need(0) = Hs), and never more than
// Hs floor(T(n) / Hs) samples, so that a stream that ends right there takes nothing back.
#include "../../include/fq3hip.h"
#include "tsm_kernels.cuh"

#include <cmath>
#include <string>
#include <vector>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define THIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kMinPermille = 250, kMaxPermille = 4000;       // the OpenAI range of `speed`
constexpr int kMinHs = 16, kMaxHs = 480;
constexpr int64_t kMaxLength = (int64_t)1 << 50;              // 1000 n stays far inside 64 bits

struct Plan { int Hs, P, HL; };

int plan_(int in_rate, int permille, Plan* p) {
    if (in_rate <= 0) return fq3_fail_(FQ3_EINVAL, "tsm: the sample rate must be positive");
    if (permille < kMinPermille || permille > kMaxPermille)
        return fq3_fail_(FQ3_EINVAL, "tsm: speed " + std::to_string(permille / 1000.0) + " is outside [0.25, 4.0]");
    const int64_t Hs = ((int64_t)in_rate + 50) / 100;
    if (Hs < kMinHs || Hs > kMaxHs || Hs % 16)
        return fq3_fail_(FQ3_EINVAL, "tsm: " + std::to_string(in_rate) + " Hz gives a hop of " + std::to_string(Hs) +
                         " samples; it must be a multiple of 16 in [16, 480] (8, 16, 24, 32, 48 kHz are)");
    p->Hs = (int)Hs; p->P = permille;
    // history the next segment S can still reach: from min(a(S), a(S-1) + Hs) - D to the end of the input.  S is held back either by
    // need(S) > n, then that is below |a(S) - a(S-1) - Hs| + 2 D + N, or by the cap, then n <= a(S+1).  Steps of a() are dlo or dhi.
    const int64_t q = Hs * permille, dlo = q / 1000, dhi = (q + 999) / 1000;
    const int64_t by_need = std::max(std::llabs(dhi - Hs), std::llabs(dlo - Hs)) + 2 * Hs + 2 * Hs;
    const int64_t by_cap = std::max(dhi, 2 * dhi - Hs) + Hs + 1;
    p->HL = (int)std::max(by_need, by_cap);
    return 0;
}

inline int64_t a_(const Plan& p, int64_t s) { return s * p.Hs * p.P / 1000; }                         // s >= 0
inline int64_t need_(const Plan& p, int64_t s) { return s == 0 ? p.Hs : std::max(a_(p, s), a_(p, s - 1) + p.Hs) + 3 * (int64_t)p.Hs; }
inline int64_t total_(const Plan& p, int64_t n) { return (n * 1000 + p.P - 1) / p.P; }

// outputs that exist once n samples have been pushed (n >= 0)
int64_t count_(const Plan& p, int64_t n, int final) {
    const int64_t T = total_(p, n);
    if (final) return T;
    // need() does not decrease in s: the largest S <= floor(T / Hs) whose segments 0 .. S-1 all have need <= n
    int64_t lo = 0, hi = T / p.Hs;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (need_(p, mid - 1) <= n) lo = mid; else hi = mid - 1;
    }
    return lo * p.Hs;
}

void window_(int N, float* w) {
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < N; ++j) w[j] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)j / (double)N));
}

}  // namespace

struct fq3_tsm {
    Plan p{};
    float* window = nullptr;          // device [N]
    float* hist[2] = {nullptr, nullptr};
    int* state = nullptr;             // device: delta of the last emitted segment
    int cur = 0, hist_valid = 0;
    int64_t n_in = 0, n_out = 0;      // cumulative input / output samples of the current stream
    bool finished = false;
};

extern "C" int fq3_tsm_design(int in_rate, int speed_permille, int* N, int* Hs, int* delta, float* window, int64_t capacity) {
    if (!N || !Hs || !delta) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_design: null N / Hs / delta");
    Plan p{};
    if (int rc = plan_(in_rate, speed_permille, &p)) return rc;
    *N = 2 * p.Hs; *Hs = p.Hs; *delta = p.Hs;
    if (window) {
        if (capacity < 2 * p.Hs) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_design: window capacity below N floats");
        window_(2 * p.Hs, window);
    }
    return 0;
}

extern "C" int64_t fq3_tsm_count(int in_rate, int speed_permille, int64_t n_in, int final) {
    Plan p{};
    if (int rc = plan_(in_rate, speed_permille, &p)) return rc;
    if (n_in < 0) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_count: negative length");
    if (n_in > kMaxLength) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_count: length above 2^50 samples");
    return count_(p, n_in, final);
}

extern "C" int fq3_tsm_create(const fq3_tsm_config* cfg, fq3_tsm** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_create: null argument");
    Plan p{};
    if (int rc = plan_(cfg->in_rate, cfg->speed_permille, &p)) return rc;
    fq3_tsm* t = new fq3_tsm();
    t->p = p;
    const int N = 2 * p.Hs;
    std::vector<float> w(N);
    window_(N, w.data());
    hipError_t e = hipMalloc((void**)&t->window, (size_t)N * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&t->hist[0], (size_t)(2 * p.HL) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&t->state, sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(t->window, w.data(), (size_t)N * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->state, 0, sizeof(int));
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_tsm_create: ") + hipGetErrorString(e);
        fq3_tsm_destroy(t);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    t->hist[1] = t->hist[0] + p.HL;
    *out = t;
    return 0;
}

extern "C" int fq3_tsm_destroy(fq3_tsm* t) {
    if (!t) return 0;
    if (t->window) (void)hipFree(t->window);
    if (t->hist[0]) (void)hipFree(t->hist[0]);
    if (t->state) (void)hipFree(t->state);
    delete t;
    return 0;
}

extern "C" int fq3_tsm_reset(fq3_tsm* t, void* stream) {
    if (!t) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_reset: null object");
    (void)stream;                     // nothing to enqueue: a stream's first segment reads neither the history nor the stored delta
    t->n_in = t->n_out = 0;
    t->hist_valid = 0;
    t->finished = false;
    return 0;
}

namespace {

// One push, in the steps the single and the group entry share (as in fq3_audio.hip): check_push_ refuses or counts and leaves the
// object alone, plan_push_ reads the object's state into the kernel's arguments, commit_push_ moves the object.
int check_push_(const std::string& who, const fq3_tsm* t, const float* pcm, int64_t n_in, int final, const float* out,
                int64_t capacity_samples, const int32_t* deltas, int64_t deltas_capacity, int64_t* cnt_out) {
    if (n_in < 0 || capacity_samples < 0 || deltas_capacity < 0 || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (t->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_tsm_reset starts the next one");
    const Plan& p = t->p;
    if (n_in > kMaxLength - t->n_in) return fq3_fail_(FQ3_EINVAL, who + ": stream above 2^50 samples");
    const int64_t total = t->n_in + n_in;
    const int64_t cnt = count_(p, total, final) - t->n_out;
    if (cnt > capacity_samples)
        return fq3_fail_(FQ3_EINVAL, who + ": " + std::to_string(cnt) + " output samples, capacity " + std::to_string(capacity_samples));
    if (cnt > 0 && !out) return fq3_fail_(FQ3_EINVAL, who + ": null output");
    const int64_t s0 = t->n_out / p.Hs, n_seg = (cnt + p.Hs - 1) / p.Hs;      // an unfinished stream holds whole segments only
    if (deltas && n_seg > deltas_capacity)
        return fq3_fail_(FQ3_EINVAL, who + ": " + std::to_string(n_seg) + " segments, delta capacity " + std::to_string(deltas_capacity));
    if (!final) {
        // what the next segment may reach back to must be inside the history this push leaves (plan_ sizes it; never expected)
        const int64_t S = s0 + n_seg;
        const int64_t reach = S == 0 ? 0 : std::min(a_(p, S), a_(p, S - 1) + p.Hs) - p.Hs;
        if (total - reach > p.HL) return fq3_fail_(FQ3_ESTATE, who + ": history too short for the next segment");
    }
    *cnt_out = cnt;
    return 0;
}

void plan_push_(const fq3_tsm* t, const float* pcm, int64_t n_in, float* out, int64_t cnt, int32_t* deltas, TsmArgs* kp) {
    const Plan& p = t->p;
    const int64_t s0 = t->n_out / p.Hs, n_seg = (cnt + p.Hs - 1) / p.Hs;
    TsmArgs& k = *kp;
    k.pcm = pcm; k.hist = t->hist[t->cur]; k.hist_next = t->hist[t->cur ^ 1]; k.window = t->window; k.out = out;
    k.delta_out = deltas; k.state = t->state;
    k.n_in = n_in; k.n_out = cnt; k.n_seg = n_seg;
    const int64_t u0 = s0 * p.Hs * p.P;                    // 64-bit: hours of audio pass 2^31
    k.a0 = u0 / 1000 - t->n_in;
    k.r0 = (int)(u0 % 1000);
    k.prev_a = (s0 == 0 ? -(int64_t)p.Hs : a_(p, s0 - 1)) - t->n_in;
    k.step = (int64_t)p.Hs * p.P;
    k.Hs = p.Hs; k.HL = p.HL; k.hist_valid = t->hist_valid;
    k.first_is_zero = s0 == 0;
}

void commit_push_(fq3_tsm* t, int64_t n_in, int64_t cnt, int final) {
    const int64_t total = t->n_in + n_in;
    if (n_in > 0) {                                        // (a push with input is always launched)
        t->cur ^= 1;
        t->hist_valid = (int)(total < t->p.HL ? total : t->p.HL);
    }
    t->n_in = total;
    t->n_out += cnt;
    if (final) t->finished = true;
}

}  // namespace

extern "C" int fq3_tsm_push(fq3_tsm* t, const float* pcm, int64_t n_in, int final, float* out, int64_t capacity_samples,
                            int64_t* n_out, int32_t* deltas, int64_t deltas_capacity, void* stream) {
    if (!t || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_push: null argument");
    int64_t cnt = 0;
    if (int rc = check_push_("fq3_tsm_push", t, pcm, n_in, final, out, capacity_samples, deltas, deltas_capacity, &cnt)) return rc;
    *n_out = cnt;
    if (cnt > 0 || n_in > 0) {
        TsmArgs k{};
        plan_push_(t, pcm, n_in, out, cnt, deltas, &k);
        hipLaunchKernelGGL(tsm_kernel, dim3(1), dim3(kTsmThreads), (size_t)tsm_lds_floats(t->p.Hs) * sizeof(float), (hipStream_t)stream, k);
        THIP(hipGetLastError());
    }
    commit_push_(t, n_in, cnt, final);
    return 0;
}

extern "C" int fq3_tsm_push_group(fq3_tsm* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                                  float* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_tsm_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !final || !out || !capacity_samples || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_tsm_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
        if (objs[b]->p.Hs != objs[0]->p.Hs)
            return fq3_fail_(FQ3_EINVAL, "fq3_tsm_push_group: row " + std::to_string(b) + " has another in_rate (hop) than row 0");
    }
    // every row is checked and planned before any object moves
    static_assert(FQ3_STAGE_GROUP_MAX == kTsmGroupMax, "the header's limit is the descriptor table's size");
    TsmGroupArgs g{};
    g.window = objs[0]->window; g.Hs = objs[0]->p.Hs;
    int64_t cnt[FQ3_STAGE_GROUP_MAX];
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (int rc = check_push_("fq3_tsm_push_group: row " + std::to_string(b), objs[b], pcm[b], n_in[b], final[b], out[b], capacity_samples[b], nullptr, 0, &cnt[b]))
            return rc;
        TsmArgs k{};
        plan_push_(objs[b], pcm[b], n_in[b], out[b], cnt[b], nullptr, &k);
        any = any || cnt[b] > 0 || n_in[b] > 0;
        TsmRow& r = g.rows[b];
        r.pcm = k.pcm; r.hist = k.hist; r.hist_next = k.hist_next; r.out = k.out; r.state = k.state;
        r.n_in = k.n_in; r.n_out = k.n_out; r.n_seg = k.n_seg; r.a0 = k.a0; r.prev_a = k.prev_a; r.step = k.step;
        r.r0 = k.r0; r.HL = k.HL; r.hist_valid = k.hist_valid; r.first_is_zero = k.first_is_zero;
    }
    if (any) {
        hipLaunchKernelGGL(tsm_group_kernel, dim3((unsigned)B), dim3(kTsmThreads), (size_t)tsm_lds_floats(g.Hs) * sizeof(float), (hipStream_t)stream, g);
        THIP(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) {
        n_out[b] = cnt[b];
        commit_push_(objs[b], n_in[b], cnt[b], final[b]);
    }
    return 0;
}
