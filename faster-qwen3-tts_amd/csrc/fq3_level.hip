// Leveller behind the C ABI: a causal, zero-latency BS.1770 gain for a stream that has not ended (include/fq3hip.h, "Leveller").
//   fq3_level_create / _push   the meter's launch (fq3_loud_push on a meter the object owns: the hop integers ARE the meter's), the
//                              targets T of the hops the push enters (one workgroup per hop), the ramped multiply: three launches
//   fq3_leveller_push_group       the pushes of up to 32 objects of one design in at most three launches (the meters', the targets',
//                              the multiplies'), each row bit for bit its single push
//   fq3_level_set_initial_gain g0 of the next stream on a kept object (host only)
//   fq3_level_stats            the newest T and S and the prefix's measure into device memory, one launch of one thread
//   fq3_level_trace            hop integers and T so far, for tests and probes
// The host tracks what follows from the lengths alone: samples pushed, T values computed, whether the stream has ended.
#include "../../include/fq3hip.h"
#define FQ3_LOUD_NO_KERNELS               // loud_kernels.cuh: the meter's kernels are defined once, in fq3_loud.hip
#include "level_kernels.cuh"

#include <cmath>
#include <string>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
void fq3_loud_buffers_(fq3_loud* l, const uint64_t** energy, const float** peak, const int** bad);      // fq3_loud.hip
int fq3_loud_push_group_(fq3_loud* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final, void* stream);      // fq3_loud.hip
#define VHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {
constexpr int kDefaultHops = 4096, kMaxHops = 1 << 20;
constexpr int64_t kMaxPush = (int64_t)1 << 40;
}  // namespace

struct fq3_level {
    int H = 0, k = 0, m = 0, capacity = 0;
    float g0 = 1.0f;
    uint64_t abs_gate = 0;
    double target_power = 0, ceiling = 0, max_gain = 0;
    fq3_loud* meter = nullptr;
    const uint64_t* energy = nullptr;         // the meter's arrays
    const float* peak = nullptr;
    const int* bad = nullptr;
    float* T = nullptr;                       // capacity + 1
    fq3_level_report* slot = nullptr;
    int64_t total = 0;                        // samples pushed
    int t_done = 0;                           // T[0 .. t_done) are computed (enqueued)
    bool finished = false;
};

extern "C" int fq3_level_create(const fq3_level_config* cfg, fq3_level** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_level_create: null argument");
    int H = 0;
    uint64_t gate = 0;
    double tp = 0, ce = 0, mg = 0;
    if (int rc = fq3_loud_design(cfg->in_rate, cfg->target_lufs, cfg->ceiling_db, cfg->max_gain_db, &H, nullptr, nullptr, &gate, &tp, &ce, &mg))
        return rc;
    if (!(cfg->initial_gain_db >= -60.0 && cfg->initial_gain_db <= 40.0)) return fq3_fail_(FQ3_EINVAL, "level: initial_gain_db outside [-60, 40]");
    if (cfg->smooth_hops < 1 || cfg->smooth_hops > kLevelMaxSmooth) return fq3_fail_(FQ3_EINVAL, "level: smooth_hops outside [1, 64]");
    if (cfg->min_blocks < 1 || cfg->min_blocks > 64) return fq3_fail_(FQ3_EINVAL, "level: min_blocks outside [1, 64]");
    if (cfg->capacity_hops < 0 || cfg->capacity_hops > kMaxHops) return fq3_fail_(FQ3_EINVAL, "level: capacity_hops outside [0, 2^20]");
    fq3_level* l = new fq3_level();
    l->H = H; l->k = cfg->smooth_hops; l->m = cfg->min_blocks;
    l->capacity = cfg->capacity_hops ? cfg->capacity_hops : kDefaultHops;
    l->g0 = (float)std::pow(10.0, cfg->initial_gain_db / 20.0);
    l->abs_gate = gate; l->target_power = tp; l->ceiling = ce; l->max_gain = mg;
    fq3_loud_config mc{cfg->in_rate, cfg->target_lufs, cfg->ceiling_db, cfg->max_gain_db, l->capacity};
    if (int rc = fq3_loud_create(&mc, &l->meter)) {
        fq3_level_destroy(l);
        return rc;
    }
    fq3_loud_buffers_(l->meter, &l->energy, &l->peak, &l->bad);
    hipError_t e = hipMalloc((void**)&l->T, ((size_t)l->capacity + 1) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&l->slot, sizeof(fq3_level_report));
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_level_create: ") + hipGetErrorString(e);
        fq3_level_destroy(l);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    *out = l;
    return 0;
}

extern "C" int fq3_level_destroy(fq3_level* l) {
    if (!l) return 0;
    if (l->meter) (void)fq3_loud_destroy(l->meter);
    if (l->T) (void)hipFree(l->T);
    if (l->slot) (void)hipFree(l->slot);
    delete l;
    return 0;
}

extern "C" int fq3_level_reset(fq3_level* l, void* stream) {
    if (!l) return fq3_fail_(FQ3_EINVAL, "fq3_level_reset: null object");
    if (int rc = fq3_loud_reset(l->meter, stream)) return rc;
    l->total = 0;                     // nothing to enqueue: every T a push reads is written by the pushes in front of it
    l->t_done = 0;
    l->finished = false;
    return 0;
}

extern "C" int fq3_level_set_initial_gain(fq3_level* l, double initial_gain_db) {
    if (!l) return fq3_fail_(FQ3_EINVAL, "fq3_level_set_initial_gain: null object");
    if (!(initial_gain_db >= -60.0 && initial_gain_db <= 40.0)) return fq3_fail_(FQ3_EINVAL, "level: initial_gain_db outside [-60, 40]");
    if (l->total > 0 || l->finished)
        return fq3_fail_(FQ3_ESTATE, "fq3_level_set_initial_gain: the stream has begun; the initial gain is set between fq3_level_reset and the first sample");
    l->g0 = (float)std::pow(10.0, initial_gain_db / 20.0);      // (the kernels take g0 by value with every launch: nothing to enqueue)
    return 0;
}

namespace {

// One push, in the steps the single and the group entry share (as in fq3_audio.hip): check_push_ refuses and leaves the object alone,
// plan_push_ reads the object's state into the two kernels' arguments, commit_push_ moves the object.  The meter's launch lies between
// check and plan: fq3_loud_push (or its group form) checks the meter itself and moves nothing when it refuses.
int check_push_(const std::string& who, const fq3_level* l, const float* pcm, int64_t n_in, const float* out) {
    if (n_in < 0 || n_in > kMaxPush || (n_in > 0 && (!pcm || !out))) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (l->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_level_reset starts the next one");
    const int64_t h1 = (l->total + n_in) / l->H;
    if (h1 > l->capacity)
        return fq3_fail_(FQ3_ETOOLONG, who + ": " + std::to_string(h1) + " hops exceed the capacity of " + std::to_string(l->capacity));
    return 0;
}

// n_in > 0.  -> whether the push enters a hop: T[t_done .. h1], hop h1 being the last one a sample of this push lies in (or the one behind it)
bool plan_push_(const fq3_level* l, const float* pcm, int64_t n_in, float* out, LevelTargetArgs* tp, LevelApplyArgs* ap) {
    const int64_t h1 = (l->total + n_in) / l->H;
    LevelTargetArgs& k = *tp;
    k.energy = l->energy; k.peak = l->peak; k.bad = l->bad; k.T = l->T; k.slot = l->slot;
    k.h_first = l->t_done; k.h_last = (int)h1; k.min_blocks = l->m; k.g0 = l->g0;
    k.abs_gate = l->abs_gate; k.four_h = (double)(4 * l->H); k.target_power = l->target_power; k.ceiling = l->ceiling; k.max_gain = l->max_gain;
    LevelApplyArgs& a = *ap;
    a.pcm = pcm; a.out = out; a.T = l->T; a.n0 = l->total; a.n_in = n_in; a.H = l->H; a.k = l->k; a.g0 = l->g0;
    return (int)h1 >= l->t_done;
}

void commit_push_(fq3_level* l, int64_t n_in, int final) {
    if (n_in > 0) {
        const int64_t total = l->total + n_in, h1 = total / l->H;
        if ((int)h1 >= l->t_done) l->t_done = (int)h1 + 1;
        l->total = total;
    }
    if (final) l->finished = true;
}

// rows share every config field but initial_gain_db and capacity_hops
bool same_design_(const fq3_level* a, const fq3_level* b) {
    return a->H == b->H && a->k == b->k && a->m == b->m && a->abs_gate == b->abs_gate && a->target_power == b->target_power &&
           a->ceiling == b->ceiling && a->max_gain == b->max_gain;
}

}  // namespace

extern "C" int fq3_level_push(fq3_level* l, const float* pcm, int64_t n_in, int final, float* out, void* stream) {
    if (!l) return fq3_fail_(FQ3_EINVAL, "fq3_level_push: null object");
    if (int rc = check_push_("fq3_level_push", l, pcm, n_in, out)) return rc;
    if (n_in > 0) {                                                 // (an empty push completes and emits nothing)
        // 1: the hops this push completes (its own arguments were checked above: it can only fail in the launch)
        if (int rc = fq3_loud_push(l->meter, pcm, n_in, final, stream)) return rc;
        LevelTargetArgs k{};
        LevelApplyArgs a{};
        // 2: T of the hops it enters
        if (plan_push_(l, pcm, n_in, out, &k, &a)) {
            hipLaunchKernelGGL(level_target_kernel, dim3((unsigned)(k.h_last - k.h_first + 1)), dim3(kLevelTargetThreads), 0, (hipStream_t)stream, k);
            VHIP(hipGetLastError());
        }
        // 3: the ramped gain
        const int64_t tiles = (n_in + kLevelTile - 1) / kLevelTile;
        hipLaunchKernelGGL(level_apply_kernel, dim3((unsigned)tiles), dim3(kLevelApplyThreads), 0, (hipStream_t)stream, a);
        VHIP(hipGetLastError());
    }
    commit_push_(l, n_in, final);
    return 0;
}

extern "C" int fq3_leveller_push_group(fq3_level* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                                    float* const* out, void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_leveller_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !final || !out) return fq3_fail_(FQ3_EINVAL, "fq3_leveller_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_leveller_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_leveller_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
        if (!same_design_(objs[b], objs[0]))
            return fq3_fail_(FQ3_EINVAL, "fq3_leveller_push_group: row " + std::to_string(b) + " has another design (rate, target, ceiling, largest gain, smoothing, gate) than row 0");
    }
    static_assert(FQ3_STAGE_GROUP_MAX == kLevelGroupMax, "the header's limit is the descriptor table's size");
    // every row is checked before any object moves; the meters of the rows with samples are checked once more by their group push
    for (int b = 0; b < B; ++b)
        if (int rc = check_push_("fq3_leveller_push_group: row " + std::to_string(b), objs[b], pcm[b], n_in[b], out[b])) return rc;
    fq3_loud* meters[FQ3_STAGE_GROUP_MAX];
    const float* m_pcm[FQ3_STAGE_GROUP_MAX];
    int64_t m_n[FQ3_STAGE_GROUP_MAX];
    int m_final[FQ3_STAGE_GROUP_MAX];
    int n_m = 0;
    for (int b = 0; b < B; ++b) {
        if (n_in[b] == 0) continue;                                 // (an empty push never reaches the meter, final or not)
        meters[n_m] = objs[b]->meter; m_pcm[n_m] = pcm[b]; m_n[n_m] = n_in[b]; m_final[n_m] = final[b];
        ++n_m;
    }
    // 1: the hops the rows complete
    if (int rc = fq3_loud_push_group_(meters, n_m, m_pcm, m_n, m_final, stream)) return rc;
    if (n_m > 0) {
        LevelTargetGroupArgs tg{};
        LevelApplyGroupArgs ag{};
        const fq3_level* l0 = objs[0];
        tg.min_blocks = l0->m; tg.abs_gate = l0->abs_gate; tg.four_h = (double)(4 * l0->H);
        tg.target_power = l0->target_power; tg.ceiling = l0->ceiling; tg.max_gain = l0->max_gain;
        ag.H = l0->H; ag.k = l0->k;
        int hops_max = 0;
        int64_t tiles_max = 0;
        for (int b = 0; b < B; ++b) {
            LevelTargetRow& tr = tg.rows[b];
            LevelApplyRow& ar = ag.rows[b];
            tr.h_first = 0; tr.h_last = -1;                         // (a row that enters no hop; an empty row has n_in = 0 in ar)
            if (n_in[b] == 0) continue;
            LevelTargetArgs k{};
            LevelApplyArgs a{};
            if (plan_push_(objs[b], pcm[b], n_in[b], out[b], &k, &a)) {
                tr.energy = k.energy; tr.peak = k.peak; tr.bad = k.bad; tr.T = k.T; tr.slot = k.slot;
                tr.h_first = k.h_first; tr.h_last = k.h_last; tr.g0 = k.g0;
                const int hops = k.h_last - k.h_first + 1;
                hops_max = hops > hops_max ? hops : hops_max;
            }
            ar.pcm = a.pcm; ar.out = a.out; ar.T = a.T; ar.n0 = a.n0; ar.n_in = a.n_in; ar.g0 = a.g0;
            const int64_t tiles = (a.n_in + kLevelTile - 1) / kLevelTile;
            tiles_max = tiles > tiles_max ? tiles : tiles_max;
        }
        // 2: T of the hops they enter
        if (hops_max > 0) {
            hipLaunchKernelGGL(level_target_group_kernel, dim3((unsigned)hops_max, (unsigned)B), dim3(kLevelTargetThreads), 0, (hipStream_t)stream, tg);
            VHIP(hipGetLastError());
        }
        // 3: the ramped gains
        hipLaunchKernelGGL(level_apply_group_kernel, dim3((unsigned)tiles_max, (unsigned)B), dim3(kLevelApplyThreads), 0, (hipStream_t)stream, ag);
        VHIP(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) commit_push_(objs[b], n_in[b], final[b]);
    return 0;
}

extern "C" int fq3_level_stats(fq3_level* l, fq3_level_report* stats_dev, void* stream) {
    if (!l || !stats_dev) return fq3_fail_(FQ3_EINVAL, "fq3_level_stats: null argument");
    hipLaunchKernelGGL(level_stats_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, l->slot, l->T, stats_dev, l->t_done > 0 ? 1 : 0, l->k, l->g0);
    VHIP(hipGetLastError());
    return 0;
}

extern "C" int fq3_level_trace(fq3_level* l, uint64_t* energy_dev, float* peak_dev, int32_t* bad_dev, float* target_dev, int64_t capacity,
                               int64_t* n_hops, void* stream) {
    if (!l || !n_hops) return fq3_fail_(FQ3_EINVAL, "fq3_level_trace: null argument");
    const int64_t n = l->total / l->H;
    if (capacity < n) return fq3_fail_(FQ3_EINVAL, "fq3_level_trace: capacity " + std::to_string(capacity) + " below the " + std::to_string(n) + " hops");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0 && energy_dev) VHIP(hipMemcpyAsync(energy_dev, l->energy, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if (n > 0 && peak_dev) VHIP(hipMemcpyAsync(peak_dev, l->peak, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (n > 0 && bad_dev) VHIP(hipMemcpyAsync(bad_dev, l->bad, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (l->t_done > 0 && target_dev) VHIP(hipMemcpyAsync(target_dev, l->T, (size_t)(n + 1) * sizeof(float), hipMemcpyDeviceToDevice, s));
    *n_hops = n;
    return 0;
}
