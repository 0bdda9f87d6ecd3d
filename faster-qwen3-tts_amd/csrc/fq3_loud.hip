// Loudness behind the C ABI: an ITU-R BS.1770-4 meter (mono, integrated, gated) over the vocoder's float32 PCM, the gain that brings
// an utterance to a target level under a peak ceiling, and the multiply that applies a gain -- in front of the time-scale and output
// stages (fq3_tsm.hip, fq3_audio.hip), where the PCM already is.
//   fq3_loud_design           host only (no HIP call): hop, K-weighting coefficients, the absolute gate as an integer, the gain constants
//   fq3_loud_create / _push   hop energies, peaks and non-finite counts of the hops a push completes; ONE launch per push
//   fq3_loud_push_group_      (internal, for fq3_leveller_push_group) the pushes of up to 32 meters of one rate in ONE launch
//   fq3_loud_finish           gating and gain, one launch of one workgroup, into a device fq3_loud_stats
//   fq3_loud_apply            out = pcm * *gain_dev
// The host tracks what follows from the lengths alone: samples pushed, hops completed, which history buffer is current, whether the
// stream has ended.  What depends on the data stays on the device.
#include "../../include/fq3hip.h"
#include "loud_kernels.cuh"

#include <cmath>
#include <string>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define LHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kMinRate = 8000, kMaxRate = 48000, kDefaultHops = 4096, kMaxHops = 1 << 20;
constexpr int64_t kMaxPush = (int64_t)1 << 40;

struct Plan {
    int H;
    double c64[10];
    float c32[10];
    uint64_t abs_gate;
    double target_power, ceiling, max_gain;
};

// the libebur128 construction of the two K-weighting biquads (bilinear transform of the analogue prototypes)
void biquads_(int rate, double* c) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / rate);
        const double a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

int plan_(int rate, double target_lufs, double ceiling_db, double max_gain_db, Plan* p) {
    if (rate < kMinRate || rate > kMaxRate || rate % 100)
        return fq3_fail_(FQ3_EINVAL, "loud: the sample rate " + std::to_string(rate) + " must be a multiple of 100 in [8000, 48000]");
    if (!(target_lufs >= -40.0 && target_lufs <= -5.0)) return fq3_fail_(FQ3_EINVAL, "loud: target_lufs outside [-40, -5]");
    if (!(ceiling_db >= -20.0 && ceiling_db <= 0.0)) return fq3_fail_(FQ3_EINVAL, "loud: ceiling_db outside [-20, 0]");
    if (!(max_gain_db >= 0.0 && max_gain_db <= 40.0)) return fq3_fail_(FQ3_EINVAL, "loud: max_gain_db outside [0, 40]");
    p->H = rate / 10;
    biquads_(rate, p->c64);
    for (int i = 0; i < 10; ++i) p->c32[i] = (float)p->c64[i];
    p->abs_gate = (uint64_t)std::floor(std::pow(10.0, (-70.0 + 0.691) / 10.0) * (double)(4 * p->H) * kLoudScale);
    p->target_power = std::pow(10.0, (target_lufs + 0.691) / 10.0);
    p->ceiling = std::pow(10.0, ceiling_db / 20.0);
    p->max_gain = std::pow(10.0, max_gain_db / 20.0);
    return 0;
}

LoudCoef coef_(const float* c) { return LoudCoef{c[0], c[1], c[2], c[3], c[4]}; }

}  // namespace

struct fq3_loud {
    Plan p{};
    int capacity = 0;
    float* hist[2] = {nullptr, nullptr};      // 2 H floats each
    uint64_t* energy = nullptr;               // capacity + 1 of each: entry n_hops of the last two is the partial hop at the end
    float* peak = nullptr;
    int* bad = nullptr;
    int cur = 0;
    int64_t total = 0;                        // samples pushed
    bool finished = false;
};

extern "C" int fq3_loud_design(int in_rate, double target_lufs, double ceiling_db, double max_gain_db, int* H, double* coef64,
                               float* coef32, uint64_t* abs_gate, double* target_power, double* ceiling, double* max_gain) {
    Plan p{};
    if (int rc = plan_(in_rate, target_lufs, ceiling_db, max_gain_db, &p)) return rc;
    if (H) *H = p.H;
    for (int i = 0; i < 10; ++i) {
        if (coef64) coef64[i] = p.c64[i];
        if (coef32) coef32[i] = p.c32[i];
    }
    if (abs_gate) *abs_gate = p.abs_gate;
    if (target_power) *target_power = p.target_power;
    if (ceiling) *ceiling = p.ceiling;
    if (max_gain) *max_gain = p.max_gain;
    return 0;
}

extern "C" int fq3_loud_create(const fq3_loud_config* cfg, fq3_loud** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_loud_create: null argument");
    Plan p{};
    if (int rc = plan_(cfg->in_rate, cfg->target_lufs, cfg->ceiling_db, cfg->max_gain_db, &p)) return rc;
    if (cfg->capacity_hops < 0 || cfg->capacity_hops > kMaxHops) return fq3_fail_(FQ3_EINVAL, "loud: capacity_hops outside [0, 2^20]");
    fq3_loud* l = new fq3_loud();
    l->p = p;
    l->capacity = cfg->capacity_hops ? cfg->capacity_hops : kDefaultHops;
    const size_t rows = (size_t)l->capacity + 1;
    hipError_t e = hipMalloc((void**)&l->hist[0], (size_t)(4 * p.H) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&l->energy, rows * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void**)&l->peak, rows * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&l->bad, rows * sizeof(int));
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_loud_create: ") + hipGetErrorString(e);
        fq3_loud_destroy(l);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    l->hist[1] = l->hist[0] + 2 * p.H;
    *out = l;
    return 0;
}

extern "C" int fq3_loud_destroy(fq3_loud* l) {
    if (!l) return 0;
    if (l->hist[0]) (void)hipFree(l->hist[0]);
    if (l->energy) (void)hipFree(l->energy);
    if (l->peak) (void)hipFree(l->peak);
    if (l->bad) (void)hipFree(l->bad);
    delete l;
    return 0;
}

// fq3_level.hip: the per-hop arrays of a meter the leveller owns (capacity + 1 entries each), read by its target kernel
void fq3_loud_buffers_(fq3_loud* l, const uint64_t** energy, const float** peak, const int** bad) {
    *energy = l->energy; *peak = l->peak; *bad = l->bad;
}

extern "C" int fq3_loud_reset(fq3_loud* l, void* stream) {
    if (!l) return fq3_fail_(FQ3_EINVAL, "fq3_loud_reset: null object");
    (void)stream;                     // nothing to enqueue: every entry a finish reads is written by the pushes in front of it
    l->total = 0;
    l->finished = false;
    return 0;
}

namespace {

// One push, in the steps the single and the group entry share (as in fq3_audio.hip): check_push_ refuses and leaves the object alone,
// plan_push_ reads the object's state into the kernel's arguments, commit_push_ moves the object.
int check_push_(const std::string& who, const fq3_loud* l, const float* pcm, int64_t n_in) {
    if (n_in < 0 || n_in > kMaxPush || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (l->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_loud_reset starts the next one");
    const int64_t h1 = (l->total + n_in) / l->p.H;
    if (h1 > l->capacity)
        return fq3_fail_(FQ3_ETOOLONG, who + ": " + std::to_string(h1) + " hops exceed the capacity of " + std::to_string(l->capacity));
    return 0;
}

// a push with nothing to complete and nothing to end is not launched and changes nothing
bool has_work_(int64_t n_in, int final) { return n_in > 0 || final; }

void plan_push_(const fq3_loud* l, const float* pcm, int64_t n_in, int final, LoudPushArgs* kp) {
    const int H = l->p.H;
    const int64_t h0 = l->total / H, total = l->total + n_in, h1 = total / H;
    LoudPushArgs& k = *kp;
    k.v0 = h0 > 0 ? (h0 - 1) * H : 0;
    k.pcm = pcm; k.hist = l->hist[l->cur]; k.hist_next = l->hist[l->cur ^ 1];
    k.energy = l->energy; k.peak = l->peak; k.bad = l->bad;
    k.n_hist = l->total - k.v0; k.n_in = n_in;
    k.h0 = h0; k.n_new = (int)(h1 - h0); k.H = H; k.final = final ? 1 : 0;
    k.keep = final ? 0 : (int)(total - (h1 > 0 ? (h1 - 1) * H : 0));
    k.shelf = coef_(l->p.c32); k.hp = coef_(l->p.c32 + 5);
}

void commit_push_(fq3_loud* l, int64_t n_in, int final) {
    if (!has_work_(n_in, final)) return;
    l->cur ^= 1;
    l->total += n_in;
    if (final) l->finished = true;
}

}  // namespace

extern "C" int fq3_loud_push(fq3_loud* l, const float* pcm, int64_t n_in, int final, void* stream) {
    if (!l) return fq3_fail_(FQ3_EINVAL, "fq3_loud_push: null object");
    if (int rc = check_push_("fq3_loud_push", l, pcm, n_in)) return rc;
    if (!has_work_(n_in, final)) return 0;                          // nothing completes and nothing changes
    LoudPushArgs k{};
    plan_push_(l, pcm, n_in, final, &k);
    const int n_wg = (k.n_new + kLoudLanes - 1) / kLoudLanes;
    hipLaunchKernelGGL(loud_push_kernel, dim3(n_wg + 1), dim3(kLoudLanes), 0, (hipStream_t)stream, k);
    LHIP(hipGetLastError());
    commit_push_(l, n_in, final);
    return 0;
}

// fq3_level.hip (fq3_leveller_push_group): the pushes of up to FQ3_STAGE_GROUP_MAX meters of one rate in ONE launch, each row bit for bit
// its fq3_loud_push.  Every row is checked before any meter moves; on a refusal the first failing row's code comes back, nothing is
// launched and no meter has changed.  The caller has checked B and the arrays and hands over distinct meters; another rate is FQ3_EINVAL.
int fq3_loud_push_group_(fq3_loud* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final, void* stream) {
    static_assert(FQ3_STAGE_GROUP_MAX == kLoudGroupMax, "the header's limit is the descriptor table's size");
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX) return fq3_fail_(FQ3_EINVAL, "fq3_loud_push_group_: a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    LoudGroupArgs g{};
    g.H = objs[0]->p.H; g.shelf = coef_(objs[0]->p.c32); g.hp = coef_(objs[0]->p.c32 + 5);
    int wg_max = 0;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const fq3_loud* l = objs[b];
        if (l->p.H != g.H) return fq3_fail_(FQ3_EINVAL, "fq3_loud_push_group_: row " + std::to_string(b) + " has another rate than row 0");
        if (int rc = check_push_("fq3_loud_push_group_: row " + std::to_string(b), l, pcm[b], n_in[b])) return rc;
        LoudRow& r = g.rows[b];
        r.active = has_work_(n_in[b], final[b]) ? 1 : 0;
        if (!r.active) continue;
        LoudPushArgs k{};
        plan_push_(l, pcm[b], n_in[b], final[b], &k);
        r.pcm = k.pcm; r.hist = k.hist; r.hist_next = k.hist_next; r.energy = k.energy; r.peak = k.peak; r.bad = k.bad;
        r.n_hist = k.n_hist; r.n_in = k.n_in; r.v0 = k.v0; r.h0 = k.h0;
        r.n_new = k.n_new; r.final = k.final; r.keep = k.keep;
        const int n_wg = (k.n_new + kLoudLanes - 1) / kLoudLanes;
        wg_max = n_wg > wg_max ? n_wg : wg_max;
        any = true;
    }
    if (any) {
        hipLaunchKernelGGL(loud_push_group_kernel, dim3((unsigned)(wg_max + 1), (unsigned)B), dim3(kLoudLanes), 0, (hipStream_t)stream, g);
        LHIP(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) commit_push_(objs[b], n_in[b], final[b]);
    return 0;
}

extern "C" int fq3_loud_finish(fq3_loud* l, fq3_loud_stats* stats_dev, void* stream) {
    if (!l || !stats_dev) return fq3_fail_(FQ3_EINVAL, "fq3_loud_finish: null argument");
    if (!l->finished) return fq3_fail_(FQ3_ESTATE, "fq3_loud_finish: the stream has not ended (a final push comes first)");
    LoudFinishArgs k{};
    k.energy = l->energy; k.peak = l->peak; k.bad = l->bad; k.out = stats_dev;
    k.n_hops = (int)(l->total / l->p.H);
    k.abs_gate = l->p.abs_gate;
    k.four_h = (double)(4 * l->p.H); k.target_power = l->p.target_power; k.ceiling = l->p.ceiling; k.max_gain = l->p.max_gain;
    hipLaunchKernelGGL(loud_finish_kernel, dim3(1), dim3(kLoudFinishThreads), 0, (hipStream_t)stream, k);
    LHIP(hipGetLastError());
    return 0;
}

extern "C" int fq3_loud_hops(fq3_loud* l, uint64_t* out_dev, int64_t capacity, int64_t* n_hops, void* stream) {
    if (!l || !n_hops) return fq3_fail_(FQ3_EINVAL, "fq3_loud_hops: null argument");
    const int64_t n = l->total / l->p.H;
    if (capacity < n || (n > 0 && !out_dev))
        return fq3_fail_(FQ3_EINVAL, "fq3_loud_hops: capacity " + std::to_string(capacity) + " below the " + std::to_string(n) + " hops");
    if (n > 0) LHIP(hipMemcpyAsync(out_dev, l->energy, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    *n_hops = n;
    return 0;
}

extern "C" int fq3_loud_apply(const float* gain_dev, const float* pcm, int64_t n, float* out, void* stream) {
    if (n < 0 || n > kMaxPush) return fq3_fail_(FQ3_EINVAL, "fq3_loud_apply: length outside [0, 2^40]");
    if (!gain_dev || (n > 0 && (!pcm || !out))) return fq3_fail_(FQ3_EINVAL, "fq3_loud_apply: null argument");
    if (n == 0) return 0;
    int64_t blocks = (n + 4 * kLoudApplyThreads - 1) / (4 * kLoudApplyThreads);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(loud_apply_kernel, dim3((unsigned)blocks), dim3(kLoudApplyThreads), 0, (hipStream_t)stream, gain_dev, pcm, out, n);
    LHIP(hipGetLastError());
    return 0;
}
