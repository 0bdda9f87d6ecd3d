// Segment join behind the C ABI: a stream that is a sequence of SEGMENTS (the sentences of a long text, each the vocoder's float32
// PCM) becomes one continuous PCM stream in front of the time-scale and output stages (fq3_tsm.hip, fq3_audio.hip, fq3_flac.hip).
//   fq3_join_bound            host only (no HIP call): the output room a push needs
//   fq3_join_create / _push   per segment: leading and trailing silence removed, a pause of zeros behind it; ONE launch per push
//   fq3_join_push_group       the pushes of up to 32 objects (the streams of many texts) in ONE launch, a workgroup per row, each row
//                             bit for bit its single push
//
// H = in_rate / 100.  A segment of n samples has hops h = 0 .. last = ceil(n / H) - 1; active(h): some |x| >= threshold in hop h.
// No active hop: the segment and its pause contribute nothing.  Else with a / b the first / last active hop and L = last - b the
// segment contributes samples [max(0, a - lead_hops) H, end of hop last - R), R = min(max(0, L - tail_hops), hold_hops), bit for
// bit, then pause_samples zeros.  The result is a function of the segments' samples and pauses alone, not of the pushes.
// How long the output is depends on the data: only the device knows (n_out_dev).  The host tracks what it can: the length of the
// current segment modulo H, which of the two pending buffers is current, whether the stream has ended.
#include "../../include/fq3hip.h"
#include "join_kernels.cuh"

#include <string>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define JHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kMinRate = 8000, kMaxRate = 48000, kMaxLead = 16, kMaxHold = 400, kMaxPauseSeconds = 5;
constexpr int64_t kMaxPush = (int64_t)1 << 40;

struct Plan { int H, lead, tail, hold; float threshold; int64_t state_floats; };

int plan_(const fq3_join_config* c, Plan* p) {
    if (!c) return fq3_fail_(FQ3_EINVAL, "join: null config");
    if (c->in_rate < kMinRate || c->in_rate > kMaxRate || c->in_rate % 100)
        return fq3_fail_(FQ3_EINVAL, "join: the sample rate " + std::to_string(c->in_rate) + " must be a multiple of 100 in [8000, 48000]");
    if (!(c->threshold > 0.0f && c->threshold < 1.0f)) return fq3_fail_(FQ3_EINVAL, "join: the threshold must lie in (0, 1)");
    if (c->lead_hops < 0 || c->lead_hops > kMaxLead) return fq3_fail_(FQ3_EINVAL, "join: lead_hops outside [0, 16]");
    if (c->hold_hops < 0 || c->hold_hops > kMaxHold) return fq3_fail_(FQ3_EINVAL, "join: hold_hops outside [0, 400]");
    if (c->tail_hops < 0 || c->tail_hops > c->hold_hops) return fq3_fail_(FQ3_EINVAL, "join: tail_hops outside [0, hold_hops]");
    p->H = c->in_rate / 100; p->lead = c->lead_hops; p->tail = c->tail_hops; p->hold = c->hold_hops; p->threshold = c->threshold;
    p->state_floats = (int64_t)(c->hold_hops + c->lead_hops + 1) * p->H;
    return 0;
}

}  // namespace

struct fq3_join {
    Plan p{};
    int in_rate = 0;
    float* pend[2] = {nullptr, nullptr};
    int* state = nullptr;             // device: phase, q, released
    int cur = 0, part = 0;
    bool fresh = true, finished = false;
};

extern "C" int64_t fq3_join_bound(const fq3_join_config* cfg, int64_t n_in, int64_t pause_samples) {
    Plan p{};
    if (int rc = plan_(cfg, &p)) return rc;
    if (n_in < 0 || n_in > kMaxPush) return fq3_fail_(FQ3_EINVAL, "fq3_join_bound: length outside [0, 2^40]");
    if (pause_samples < 0 || pause_samples > (int64_t)kMaxPauseSeconds * cfg->in_rate)
        return fq3_fail_(FQ3_EINVAL, "fq3_join_bound: pause outside [0, 5 s]");
    return n_in + p.state_floats + pause_samples;
}

extern "C" int fq3_join_create(const fq3_join_config* cfg, fq3_join** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_join_create: null argument");
    Plan p{};
    if (int rc = plan_(cfg, &p)) return rc;
    fq3_join* j = new fq3_join();
    j->p = p; j->in_rate = cfg->in_rate;
    hipError_t e = hipMalloc((void**)&j->pend[0], (size_t)(2 * p.state_floats) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&j->state, 4 * sizeof(int));
    if (e == hipSuccess) e = hipMemset(j->state, 0, 4 * sizeof(int));
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_join_create: ") + hipGetErrorString(e);
        fq3_join_destroy(j);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    j->pend[1] = j->pend[0] + p.state_floats;
    *out = j;
    return 0;
}

extern "C" int fq3_join_destroy(fq3_join* j) {
    if (!j) return 0;
    if (j->pend[0]) (void)hipFree(j->pend[0]);
    if (j->state) (void)hipFree(j->state);
    delete j;
    return 0;
}

extern "C" int fq3_join_reset(fq3_join* j, void* stream) {
    if (!j) return fq3_fail_(FQ3_EINVAL, "fq3_join_reset: null object");
    (void)stream;                     // nothing to enqueue: the first push of a stream reads neither the state words nor the pending samples
    j->part = 0;
    j->fresh = true;
    j->finished = false;
    return 0;
}

namespace {

// One push, checked and described: the single push and every row of a group go through these two, so they cannot drift apart.
// check_: changes nothing, fills the descriptor.  advance_: the host-side bookkeeping behind a launch that was accepted.
int check_(const std::string& who, const fq3_join* j, const float* pcm, int64_t n_in, int end, int64_t pause_samples, float* out,
           int64_t capacity, int64_t* n_out_dev, JoinArgs* k) {
    if (!j || !n_out_dev || !out) return fq3_fail_(FQ3_EINVAL, who + ": null argument");
    if (n_in < 0 || n_in > kMaxPush || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (end < 0 || end > 2) return fq3_fail_(FQ3_EINVAL, who + ": end must be 0, 1 or 2");
    if (pause_samples < 0 || pause_samples > (int64_t)kMaxPauseSeconds * j->in_rate)
        return fq3_fail_(FQ3_EINVAL, who + ": pause outside [0, 5 s]");
    if (j->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_join_reset starts the next one");
    const Plan& p = j->p;
    const int64_t pause = end == 1 ? pause_samples : 0;            // only a segment that ends inside the stream is followed by a pause
    const int64_t bound = n_in + p.state_floats + pause;
    if (capacity < bound)
        return fq3_fail_(FQ3_EINVAL, who + ": capacity " + std::to_string(capacity) + " below the bound " + std::to_string(bound));
    *k = JoinArgs{};
    k->pcm = pcm; k->pend = j->pend[j->cur]; k->pend_next = j->pend[j->cur ^ 1]; k->out = out; k->n_out = n_out_dev; k->state = j->state;
    k->n_in = n_in; k->pause = pause; k->threshold = p.threshold;
    k->H = p.H; k->lead = p.lead; k->tail = p.tail; k->hold = p.hold;
    k->part = j->part; k->end = end; k->fresh = j->fresh ? 1 : 0;
    return 0;
}

void advance_(fq3_join* j, int64_t n_in, int end) {
    j->cur ^= 1;
    j->part = end ? 0 : (int)((j->part + n_in) % j->p.H);
    j->fresh = false;
    if (end == 2) j->finished = true;
}

}  // namespace

extern "C" int fq3_join_push(fq3_join* j, const float* pcm, int64_t n_in, int end, int64_t pause_samples, float* out, int64_t capacity,
                             int64_t* n_out_dev, void* stream) {
    JoinArgs k;
    if (int rc = check_("fq3_join_push", j, pcm, n_in, end, pause_samples, out, capacity, n_out_dev, &k)) return rc;
    hipLaunchKernelGGL(join_kernel, dim3(1), dim3(kJoinThreads), 0, (hipStream_t)stream, k);
    JHIP(hipGetLastError());
    advance_(j, n_in, end);
    return 0;
}

// The pushes of up to FQ3_STAGE_GROUP_MAX objects in ONE launch of B workgroups: row b is fq3_join_push of its own arguments, bit for
// bit.  Every row is checked before any object changes; each row's descriptor carries its own configuration, so the objects may differ
// in it.  The descriptors travel in the launch's argument block: no copy, no host synchronisation.
extern "C" int fq3_join_push_group(fq3_join* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* end,
                                   const int64_t* pause_samples, float* const* out, const int64_t* capacity,
                                   int64_t* const* n_out_dev, void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_join_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !end || !pause_samples || !out || !capacity || !n_out_dev)
        return fq3_fail_(FQ3_EINVAL, "fq3_join_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_join_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_join_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
    }
    static_assert(FQ3_STAGE_GROUP_MAX == kJoinGroupMax, "the header's limit is the descriptor table's size");
    JoinGroupArgs g{};
    for (int b = 0; b < B; ++b)
        if (int rc = check_("fq3_join_push_group: row " + std::to_string(b), objs[b], pcm[b], n_in[b], end[b], pause_samples[b], out[b],
                            capacity[b], n_out_dev[b], &g.row[b]))
            return rc;
    g.B = B;
    hipLaunchKernelGGL(join_group_kernel, dim3(B), dim3(kJoinThreads), 0, (hipStream_t)stream, g);
    JHIP(hipGetLastError());
    for (int b = 0; b < B; ++b) advance_(objs[b], n_in[b], end[b]);
    return 0;
}
