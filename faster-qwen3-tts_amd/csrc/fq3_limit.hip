// True-peak look-ahead limiter behind the C ABI: float32 mono in, float32 out at the same rate, length-preserving, with a fixed
// latency of A + 6 samples -- behind the gain and in front of the time-scale and output stages (fq3_tsm.hip, fq3_audio.hip).
//   fq3_limit_design / _count   host only (no HIP call): attack, hold, ceiling, the detector's three rows, the default tile
//   fq3_limit_create / _push    ONE launch per push: a workgroup per tile of output samples plus one that keeps the history
//   fq3_limit_push_group        the pushes of up to 32 objects of one design in ONE launch, each row bit for bit its single push
//   fq3_limit_stats             the accumulators (true-peak estimate, smallest gain, limited and non-finite counts) into a device struct
// The host tracks what follows from the lengths alone: samples pushed, samples emitted, which history buffer is current, whether the
// stream has ended.  What depends on the data stays on the device.
#include "../../include/fq3hip.h"
#include "fq3_common.cuh"
#include "limit_kernels.cuh"

#include <cmath>
#include <string>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define MHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kMinRate = 8000, kMaxRate = 48000;
constexpr int kMinAttack = 8, kMaxAttack = 480, kMaxHold = 1920;
constexpr int kDefaultTile = 1024, kMinTile = 256, kMaxTile = 4096;
constexpr int64_t kMaxPush = (int64_t)1 << 31;          // the grid of a push stays below 2^32 threads at the smallest tile

struct Plan {
    int A, H, tile;
    float c;
    float rows[3 * kLimitTaps];
};

double bessel_i0_(double x) {
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

int plan_(int rate, double ceiling_db, double lookahead_ms, double hold_ms, int tile, Plan* p, bool rows = true) {
    if (rate < kMinRate || rate > kMaxRate)
        return fq3_fail_(FQ3_EINVAL, "limit: the sample rate " + std::to_string(rate) + " is outside [8000, 48000]");
    if (!(ceiling_db >= -20.0 && ceiling_db <= 0.0)) return fq3_fail_(FQ3_EINVAL, "limit: ceiling_db outside [-20, 0]");
    if (!(lookahead_ms >= 0.0 && lookahead_ms <= 1000.0)) return fq3_fail_(FQ3_EINVAL, "limit: lookahead_ms is not a time");
    if (!(hold_ms >= 0.0 && hold_ms <= 1000.0)) return fq3_fail_(FQ3_EINVAL, "limit: hold_ms is not a time");
    const double a = std::round((double)rate * lookahead_ms / 1000.0), h = std::round((double)rate * hold_ms / 1000.0);
    if (a < kMinAttack || a > kMaxAttack)
        return fq3_fail_(FQ3_EINVAL, "limit: the attack of " + std::to_string((long)a) + " samples is outside [8, 480]");
    if (h < 0 || h > kMaxHold) return fq3_fail_(FQ3_EINVAL, "limit: the hold of " + std::to_string((long)h) + " samples is outside [0, 1920]");
    if (tile != 0 && (tile < kMinTile || tile > kMaxTile || tile % kLimitThreads))
        return fq3_fail_(FQ3_EINVAL, "limit: the tile must be 0 or a multiple of 256 in [256, 4096]");
    p->A = (int)a; p->H = (int)h; p->tile = tile ? tile : kDefaultTile;
    p->c = (float)std::pow(10.0, ceiling_db / 20.0);
    if (!rows) return 0;
    const double pi = 3.14159265358979323846, beta = 8.0, half = 6.0;
    for (int f = 1; f <= 3; ++f) {
        double w[kLimitTaps], sum = 0.0;
        for (int t = 0; t < kLimitTaps; ++t) {
            const double d = (double)(t - kLimitBefore) - 0.25 * f;            // tap position seen from the point n + f / 4
            const double r = d / half;
            w[t] = std::sin(pi * d) / (pi * d) * bessel_i0_(beta * std::sqrt(1.0 - r * r)) / bessel_i0_(beta);
            sum += w[t];
        }
        for (int t = 0; t < kLimitTaps; ++t) p->rows[(f - 1) * kLimitTaps + t] = (float)(w[t] / sum);
    }
    return 0;
}

size_t lds_bytes_(const Plan& p) {
    const int cap = p.tile + 2 * p.A + p.H + kLimitBefore + kLimitAfter;
    return (size_t)3 * ((cap + 3) & ~3) * sizeof(float);
}

}  // namespace

struct fq3_limit {
    Plan p{};
    int rate = 0;
    int n_keep = 0;                           // 2 A + H + 11
    float* hist[2] = {nullptr, nullptr};      // n_keep floats each
    LimitAcc* acc = nullptr;
    int cur = 0;
    int64_t total = 0, emitted = 0;
    bool finished = false;
};

extern "C" int fq3_limit_design(int in_rate, double ceiling_db, double lookahead_ms, double hold_ms, int* A, int* H, float* ceiling,
                                float* rows, int* tile) {
    Plan p{};
    if (int rc = plan_(in_rate, ceiling_db, lookahead_ms, hold_ms, 0, &p)) return rc;
    if (A) *A = p.A;
    if (H) *H = p.H;
    if (ceiling) *ceiling = p.c;
    if (rows) for (int i = 0; i < 3 * kLimitTaps; ++i) rows[i] = p.rows[i];
    if (tile) *tile = p.tile;
    return 0;
}

extern "C" int64_t fq3_limit_count(int in_rate, double lookahead_ms, int64_t n_in, int final) {
    Plan p{};
    if (int rc = plan_(in_rate, 0.0, lookahead_ms, 0.0, 0, &p, false)) return rc;
    if (n_in < 0 || n_in > kMaxPush) return fq3_fail_(FQ3_EINVAL, "fq3_limit_count: n_in outside [0, 2^31]");
    if (final) return n_in;
    const int64_t n = n_in - p.A - kLimitAfter;
    return n > 0 ? n : 0;
}

extern "C" int fq3_limit_create(const fq3_limit_config* cfg, fq3_limit** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_limit_create: null argument");
    Plan p{};
    if (int rc = plan_(cfg->in_rate, cfg->ceiling_db, cfg->lookahead_ms, cfg->hold_ms, cfg->tile, &p)) return rc;
    fq3_limit* l = new fq3_limit();
    l->p = p;
    l->rate = cfg->in_rate;
    l->n_keep = 2 * p.A + p.H + kLimitBefore + kLimitAfter;
    hipError_t e = hipMalloc((void**)&l->hist[0], (size_t)(2 * l->n_keep) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&l->acc, sizeof(LimitAcc));
    if (e == hipSuccess) e = hipMemset(l->acc, 0, sizeof(LimitAcc));
    if (e == hipSuccess && !lds_limit_at_least<limit_push_kernel>(lds_bytes_(p))) e = hipErrorInvalidValue;
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_limit_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        fq3_limit_destroy(l);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    l->hist[1] = l->hist[0] + l->n_keep;
    *out = l;
    return 0;
}

extern "C" int fq3_limit_destroy(fq3_limit* l) {
    if (!l) return 0;
    if (l->hist[0]) (void)hipFree(l->hist[0]);
    if (l->acc) (void)hipFree(l->acc);
    delete l;
    return 0;
}

extern "C" int fq3_limit_reset(fq3_limit* l, void* stream) {
    if (!l) return fq3_fail_(FQ3_EINVAL, "fq3_limit_reset: null object");
    MHIP(hipMemsetAsync(l->acc, 0, sizeof(LimitAcc), (hipStream_t)stream));      // the history needs nothing: its length starts at 0
    l->total = l->emitted = 0;
    l->finished = false;
    return 0;
}

namespace {

// One push, in the steps the single and the group entry share (as in fq3_audio.hip): check_push_ refuses or counts and leaves the
// object alone, plan_push_ reads the object's state into the kernel's arguments, commit_push_ moves the object.
int check_push_(const std::string& who, const fq3_limit* l, const float* pcm, int64_t n_in, int final, const float* out,
                int64_t capacity_samples, int64_t* cnt_out) {
    if (n_in < 0 || n_in > kMaxPush || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (l->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_limit_reset starts the next one");
    const int64_t total = l->total + n_in;
    const int64_t reach = total - l->p.A - kLimitAfter;
    const int64_t upto = final ? total : (reach > 0 ? reach : 0);
    const int64_t n = upto - l->emitted;
    if (n > capacity_samples || (n > 0 && !out))
        return fq3_fail_(FQ3_EINVAL, who + ": " + std::to_string(n) + " output samples exceed the capacity of " + std::to_string(capacity_samples));
    *cnt_out = n;
    return 0;
}

// a push with nothing to complete and nothing to end is not launched and changes nothing
bool has_work_(int64_t n_in, int final) { return n_in > 0 || final; }

void plan_push_(const fq3_limit* l, const float* pcm, int64_t n_in, int final, float* out, int64_t cnt, LimitPushArgs* kp) {
    const int64_t total = l->total + n_in;
    LimitPushArgs& k = *kp;
    k.n_hist = l->total < l->n_keep ? l->total : l->n_keep;
    k.pcm = pcm; k.hist = l->hist[l->cur]; k.hist_next = l->hist[l->cur ^ 1]; k.out = out; k.acc = l->acc;
    k.n_in = n_in; k.v0 = l->total - k.n_hist; k.total = total; k.o0 = l->emitted; k.n_out = cnt;
    k.A = l->p.A; k.H = l->p.H; k.tile = l->p.tile;
    k.keep = final ? 0 : (int)(total < l->n_keep ? total : l->n_keep);
    k.c = l->p.c;
    for (int i = 0; i < 3 * kLimitTaps; ++i) k.h[i] = l->p.rows[i];
}

void commit_push_(fq3_limit* l, int64_t n_in, int64_t cnt, int final) {
    if (!has_work_(n_in, final)) return;
    l->cur ^= 1;
    l->total += n_in;
    l->emitted += cnt;
    if (final) l->finished = true;
}

// in_rate, ceiling_db, lookahead_ms, hold_ms and tile, as the device sees them (the taps depend on nothing: plan_ builds the same 36)
bool same_design_(const fq3_limit* a, const fq3_limit* b) {
    return a->rate == b->rate && a->p.A == b->p.A && a->p.H == b->p.H && a->p.tile == b->p.tile && a->p.c == b->p.c;
}

}  // namespace

extern "C" int fq3_limit_push(fq3_limit* l, const float* pcm, int64_t n_in, int final, float* out, int64_t capacity_samples,
                              int64_t* n_out, void* stream) {
    if (!l || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_limit_push: null argument");
    int64_t n = 0;
    if (int rc = check_push_("fq3_limit_push", l, pcm, n_in, final, out, capacity_samples, &n)) return rc;
    *n_out = n;
    if (!has_work_(n_in, final)) return 0;                          // nothing completes and nothing changes
    LimitPushArgs k{};
    plan_push_(l, pcm, n_in, final, out, n, &k);
    const size_t shm = lds_bytes_(l->p);
    if (!lds_limit_at_least<limit_push_kernel>(shm)) return fq3_fail_(FQ3_EHIP, "fq3_limit_push: could not raise the kernel's LDS limit");
    const int64_t n_tiles = (n + k.tile - 1) / k.tile;
    hipLaunchKernelGGL(limit_push_kernel, dim3((unsigned)(n_tiles + 1)), dim3(kLimitThreads), shm, (hipStream_t)stream, k);
    MHIP(hipGetLastError());
    commit_push_(l, n_in, n, final);
    return 0;
}

extern "C" int fq3_limit_push_group(fq3_limit* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                                    float* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_limit_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !final || !out || !capacity_samples || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_limit_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_limit_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_limit_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
        if (!same_design_(objs[b], objs[0]))
            return fq3_fail_(FQ3_EINVAL, "fq3_limit_push_group: row " + std::to_string(b) + " has another design (rate, ceiling, look-ahead, hold, tile) than row 0");
    }
    // every row is checked and planned before any object moves
    static_assert(FQ3_STAGE_GROUP_MAX == kLimitGroupMax, "the header's limit is the descriptor table's size");
    LimitGroupArgs g{};
    const Plan& p0 = objs[0]->p;
    g.A = p0.A; g.H = p0.H; g.tile = p0.tile; g.c = p0.c;
    for (int i = 0; i < 3 * kLimitTaps; ++i) g.h[i] = p0.rows[i];
    int64_t cnt[FQ3_STAGE_GROUP_MAX], tiles_max = 0;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (int rc = check_push_("fq3_limit_push_group: row " + std::to_string(b), objs[b], pcm[b], n_in[b], final[b], out[b], capacity_samples[b], &cnt[b]))
            return rc;
        LimitRow& r = g.rows[b];
        r.active = has_work_(n_in[b], final[b]) ? 1 : 0;
        if (!r.active) continue;
        LimitPushArgs k{};
        plan_push_(objs[b], pcm[b], n_in[b], final[b], out[b], cnt[b], &k);
        r.pcm = k.pcm; r.hist = k.hist; r.hist_next = k.hist_next; r.out = k.out; r.acc = k.acc;
        r.n_hist = k.n_hist; r.n_in = k.n_in; r.v0 = k.v0; r.total = k.total; r.o0 = k.o0; r.n_out = k.n_out;
        r.keep = k.keep;
        const int64_t n_tiles = (cnt[b] + g.tile - 1) / g.tile;
        tiles_max = n_tiles > tiles_max ? n_tiles : tiles_max;
        any = true;
    }
    if (any) {
        const size_t shm = lds_bytes_(p0);
        if (!lds_limit_at_least<limit_push_group_kernel>(shm)) return fq3_fail_(FQ3_EHIP, "fq3_limit_push_group: could not raise the kernel's LDS limit");
        hipLaunchKernelGGL(limit_push_group_kernel, dim3((unsigned)(tiles_max + 1), (unsigned)B), dim3(kLimitThreads), shm, (hipStream_t)stream, g);
        MHIP(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) {
        n_out[b] = cnt[b];
        commit_push_(objs[b], n_in[b], cnt[b], final[b]);
    }
    return 0;
}

extern "C" int fq3_limit_stats(fq3_limit* l, fq3_limit_report* stats_dev, void* stream) {
    if (!l || !stats_dev) return fq3_fail_(FQ3_EINVAL, "fq3_limit_stats: null argument");
    hipLaunchKernelGGL(limit_stats_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (const LimitAcc*)l->acc, stats_dev);
    MHIP(hipGetLastError());
    return 0;
}
