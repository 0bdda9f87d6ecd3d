// Provenance watermark behind the C ABI: float32 mono in at 24 kHz, float32 out, length-preserving -- behind the join, the gains and
// the leveller, in front of the limiter and the output stage (fq3_limit.hip, fq3_audio.hip; the time-scale stage is part of the
// output stage, so the model refuses a speed other than 1 together with the mark).
//   fq3_mark_design / _count   host only (no HIP call): the framing constants, the strength as the device's float, the chip words
//   fq3_mark_create / _push    ONE launch per push: a workgroup per 15 hops of output plus one that keeps the history
//   fq3_mark_push_group        the pushes of up to 32 objects in ONE launch on a packed grid, each row bit for bit its single push
//   fq3_mark_detect            two launches: the partial sums of every (offset, frame tile), then z[32][128]
//   fq3_mark_scan              two launches for up to 32 clips: the sums of every block of 16 frames, then a verdict per sliding window
// The host tracks what follows from the lengths alone: samples pushed, samples emitted, which history buffer is current, whether the
// stream has ended.  The two DFT tables (2 x 256 KB) depend on nothing a caller chooses: one copy per device, made at the first
// create or detect there and kept for the life of the process.
#include "../../include/fq3hip.h"
#include "fq3_common.cuh"
#include "mark_kernels.cuh"

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define KHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr double kMinStrength = 0.02, kMaxStrength = 0.3;
constexpr int64_t kMaxPush = (int64_t)1 << 31;
constexpr int64_t kMaxDetect = (int64_t)1 << 27;        // 93 minutes at 24 kHz; the partials stay below 2^31 floats
constexpr int kMaxDevices = 64;

// Philox4x32-10 on the host, as philox4x32_10 in noise_kernels.cuh
void philox_host_(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

int strength_(const std::string& who, double strength, float* a) {
    if (!(strength == 0.0 || (strength >= kMinStrength && strength <= kMaxStrength)))
        return fq3_fail_(FQ3_EINVAL, who + ": strength is neither 0 nor in [0.02, 0.3]");
    *a = (float)strength;
    return 0;
}

// both tables in fragment order: element (k, n) of a [K][N] operand lies at ((n / 16) * (K / 4) + k / 4) * 64 + (k % 4) * 16 + n % 16
void tables_(std::vector<float>& fwd, std::vector<float>& inv) {
    const double pi = 3.14159265358979323846;
    double w[kMarkN], cs[kMarkN], sn[kMarkN];
    for (int i = 0; i < kMarkN; ++i) {
        w[i] = std::sqrt(0.5 - 0.5 * std::cos(2.0 * pi * i / kMarkN));
        cs[i] = std::cos(2.0 * pi * i / kMarkN);
        sn[i] = std::sin(2.0 * pi * i / kMarkN);
    }
    fwd.assign(kMarkFwdFloats, 0.0f);
    inv.assign(kMarkInvFloats, 0.0f);
    for (int i = 0; i < kMarkN; ++i)
        for (int c = 0; c < 2 * kMarkBins; ++c) {
            const int bin = kMarkLo + (c & (kMarkBins - 1)), m = (bin * i) & (kMarkN - 1);      // the angle, reduced exactly
            const double v = c < kMarkBins ? w[i] * cs[m] : -w[i] * sn[m];
            fwd[((size_t)(c / 16) * (kMarkN / 4) + i / 4) * 64 + (i % 4) * 16 + c % 16] = (float)v;
            inv[((size_t)(i / 16) * (2 * kMarkBins / 4) + c / 4) * 64 + (c % 4) * 16 + i % 16] = (float)(v * 2.0 / kMarkN);
        }
}

// the device's copy of the tables: fwd, then inv
int device_tables_(const float** out) {
    static std::mutex mu;
    static float* dev_tables[kMaxDevices] = {};
    int dev = -1;
    KHIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return fq3_fail_(FQ3_EINVAL, "mark: device index out of range");
    std::lock_guard<std::mutex> lock(mu);
    if (!dev_tables[dev]) {
        std::vector<float> fwd, inv;
        tables_(fwd, inv);
        float* p = nullptr;
        KHIP(hipMalloc((void**)&p, (size_t)(kMarkFwdFloats + kMarkInvFloats) * sizeof(float)));
        hipError_t e = hipMemcpy(p, fwd.data(), fwd.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p + kMarkFwdFloats, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fq3_fail_(FQ3_EHIP, std::string("mark: table upload: ") + hipGetErrorString(e));
        }
        dev_tables[dev] = p;
    }
    *out = dev_tables[dev];
    return 0;
}

int64_t count_(int64_t total, int final) {
    if (final) return total;
    const int64_t hops = total / kMarkH - 1;
    return hops > 0 ? hops * kMarkH : 0;
}

int64_t detect_frames_(int64_t n) { return (n + kMarkH - 1) / kMarkH + 1; }
int64_t detect_tiles_(int64_t n) { return (detect_frames_(n) - 2 + kMarkInner - 1) / kMarkInner; }

constexpr int kMaxWinBlocks = 4096;
int64_t scan_blocks_(int64_t n) { return (detect_frames_(n) - 2 + kMarkBlock - 1) / kMarkBlock; }
int64_t scan_windows_(int64_t nb, int win, int hop) { return nb <= win ? 1 : 1 + (nb - win + hop - 1) / hop; }

int scan_check_(const std::string& who, int win_blocks, int hop_blocks) {
    if (win_blocks < 1 || win_blocks > kMaxWinBlocks) return fq3_fail_(FQ3_EINVAL, who + ": win_blocks outside [1, 4096]");
    if (hop_blocks < 1 || hop_blocks > win_blocks) return fq3_fail_(FQ3_EINVAL, who + ": hop_blocks outside [1, win_blocks]");
    return 0;
}

int scan_rows_(const std::string& who, int B, const int64_t* n) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, who + ": B = " + std::to_string(B) + "; a call has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B > 0 && !n) return fq3_fail_(FQ3_EINVAL, who + ": null array");
    for (int b = 0; b < B; ++b)
        if (n[b] < 2 * kMarkH || n[b] > kMaxDetect) return fq3_fail_(FQ3_EINVAL, who + ": row " + std::to_string(b) + ": n outside [512, 2^27]");
    return 0;
}

}  // namespace

struct fq3_mark {
    uint64_t key = 0;
    float a = 0.0f;
    const float* tables = nullptr;            // the device's shared copy; not owned
    float* hist[2] = {nullptr, nullptr};      // kMarkKeep floats each
    int cur = 0;
    int64_t total = 0, emitted = 0;
    bool finished = false;
};

extern "C" int fq3_mark_design(uint64_t key, double strength, int* N, int* H, int* bin_lo, int* n_bins, int* period, float* a,
                               uint32_t* chip_words) {
    float af = 0.0f;
    if (int rc = strength_("fq3_mark_design", strength, &af)) return rc;
    if (N) *N = kMarkN;
    if (H) *H = kMarkH;
    if (bin_lo) *bin_lo = kMarkLo;
    if (n_bins) *n_bins = kMarkBins;
    if (period) *period = kMarkPeriod;
    if (a) *a = af;
    if (chip_words)
        for (int c = 0; c < kMarkPeriod / 2; ++c)
            philox_host_((uint32_t)c, 0u, kMarkSlot, 0u, (uint32_t)(key & 0xffffffffull), (uint32_t)(key >> 32), chip_words + 4 * c);
    return 0;
}

extern "C" int64_t fq3_mark_count(int64_t n_in, int final) {
    if (n_in < 0 || n_in > kMaxPush) return fq3_fail_(FQ3_EINVAL, "fq3_mark_count: n_in outside [0, 2^31]");
    return count_(n_in, final);
}

extern "C" int fq3_mark_create(const fq3_mark_config* cfg, fq3_mark** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_mark_create: null argument");
    float af = 0.0f;
    if (int rc = strength_("fq3_mark_create", cfg->strength, &af)) return rc;
    const float* tables = nullptr;
    if (int rc = device_tables_(&tables)) return rc;
    fq3_mark* m = new fq3_mark();
    m->key = cfg->key; m->a = af; m->tables = tables;
    const hipError_t e = hipMalloc((void**)&m->hist[0], (size_t)(2 * kMarkKeep) * sizeof(float));
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_mark_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        delete m;
        return fq3_fail_(FQ3_EHIP, msg);
    }
    m->hist[1] = m->hist[0] + kMarkKeep;
    *out = m;
    return 0;
}

extern "C" int fq3_mark_destroy(fq3_mark* m) {
    if (!m) return 0;
    if (m->hist[0]) (void)hipFree(m->hist[0]);
    delete m;
    return 0;
}

extern "C" int fq3_mark_reset(fq3_mark* m, void* stream) {
    if (!m) return fq3_fail_(FQ3_EINVAL, "fq3_mark_reset: null object");
    (void)stream;                                  // the history needs nothing: its length starts at 0
    m->total = m->emitted = 0;
    m->finished = false;
    return 0;
}

namespace {

// the single push's checks; nothing moves.  *n: the samples the push emits
int check_push_(const std::string& who, const fq3_mark* m, const float* pcm, int64_t n_in, int final, const float* out, int64_t capacity_samples,
                int64_t* n) {
    if (n_in < 0 || n_in > kMaxPush || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (m->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_mark_reset starts the next one");
    *n = count_(m->total + n_in, final) - m->emitted;
    if (*n > capacity_samples || (*n > 0 && !out))
        return fq3_fail_(FQ3_EINVAL, who + ": " + std::to_string(*n) + " output samples exceed the capacity of " + std::to_string(capacity_samples));
    return 0;
}

bool has_work_(int64_t n_in, int final) { return n_in > 0 || final; }    // else nothing completes and nothing changes

// what the kernel needs of a checked push
void plan_push_(const fq3_mark* m, const float* pcm, int64_t n_in, int final, float* out, int64_t n, MarkPushArgs* k) {
    const int64_t total = m->total + n_in;
    const int64_t n_hist = m->total < kMarkKeep ? m->total : kMarkKeep;
    k->src = MarkSrc{pcm, m->hist[m->cur], m->total - n_hist, m->total, total};
    k->hist_next = m->hist[m->cur ^ 1];
    k->out = out; k->fwd = m->tables; k->inv = m->tables + kMarkFwdFloats;
    k->o0 = m->emitted; k->n_out = n;
    k->keep = final ? 0 : (int)(total < kMarkKeep ? total : kMarkKeep);
    k->a = m->a;
    k->k0 = (uint32_t)(m->key & 0xffffffffull); k->k1 = (uint32_t)(m->key >> 32);
}

// workgroups of a push that emits n samples: one per 15 hops, and the one that keeps the history
int64_t push_grid_(int64_t n) {
    const int64_t hops = (n + kMarkH - 1) / kMarkH;
    return (hops + kMarkHops - 1) / kMarkHops + 1;
}

void commit_push_(fq3_mark* m, int64_t n_in, int64_t n, int final) {
    m->cur ^= 1;
    m->total += n_in;
    m->emitted += n;
    if (final) m->finished = true;
}

}  // namespace

extern "C" int fq3_mark_push(fq3_mark* m, const float* pcm, int64_t n_in, int final, float* out, int64_t capacity_samples,
                             int64_t* n_out, void* stream) {
    if (!m || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_mark_push: null argument");
    int64_t n = 0;
    if (int rc = check_push_("fq3_mark_push", m, pcm, n_in, final, out, capacity_samples, &n)) return rc;
    *n_out = n;
    if (!has_work_(n_in, final)) return 0;
    MarkPushArgs k{};
    plan_push_(m, pcm, n_in, final, out, n, &k);
    hipLaunchKernelGGL(mark_embed_kernel, dim3((unsigned)push_grid_(n)), dim3(kMarkThreads), 0, (hipStream_t)stream, k);
    KHIP(hipGetLastError());
    commit_push_(m, n_in, n, final);
    return 0;
}

static_assert(FQ3_STAGE_GROUP_MAX == kMarkGroupMax, "the header's limit is the descriptor table's size");

extern "C" int fq3_mark_push_group(fq3_mark* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                                   float* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_mark_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !final || !out || !capacity_samples || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_mark_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_mark_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_mark_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
        if (objs[b]->tables != objs[0]->tables)
            return fq3_fail_(FQ3_EINVAL, "fq3_mark_push_group: row " + std::to_string(b) + " was created on another device than row 0");
    }
    // every row is checked and planned before any object moves
    MarkGroupArgs g{};
    int64_t cnt[FQ3_STAGE_GROUP_MAX], grid = 0;
    for (int b = 0; b < B; ++b) {
        if (int rc = check_push_("fq3_mark_push_group: row " + std::to_string(b), objs[b], pcm[b], n_in[b], final[b], out[b], capacity_samples[b], &cnt[b]))
            return rc;
        g.wg0[b] = (int)grid;
        if (!has_work_(n_in[b], final[b])) continue;
        MarkPushArgs k{};
        plan_push_(objs[b], pcm[b], n_in[b], final[b], out[b], cnt[b], &k);
        MarkGroupRow& r = g.rows[b];
        r.src = k.src; r.hist_next = k.hist_next; r.out = k.out; r.o0 = k.o0; r.n_out = k.n_out;
        r.keep = k.keep; r.a = k.a; r.k0 = k.k0; r.k1 = k.k1;
        grid += push_grid_(cnt[b]);
    }
    if (grid > 0x7fffffff) return fq3_fail_(FQ3_EINVAL, "fq3_mark_push_group: the rows of one call need more than 2^31 workgroups");
    for (int b = B; b <= kMarkGroupMax; ++b) g.wg0[b] = (int)grid;
    if (grid > 0) {
        g.fwd = objs[0]->tables; g.inv = objs[0]->tables + kMarkFwdFloats;
        hipLaunchKernelGGL(mark_embed_group_kernel, dim3((unsigned)grid), dim3(kMarkThreads), 0, (hipStream_t)stream, g);
        KHIP(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) {
        n_out[b] = cnt[b];
        if (has_work_(n_in[b], final[b])) commit_push_(objs[b], n_in[b], cnt[b], final[b]);
    }
    return 0;
}

extern "C" int64_t fq3_mark_detect_workspace(int64_t n) {
    if (n < 2 * kMarkH || n > kMaxDetect) return fq3_fail_(FQ3_EINVAL, "fq3_mark_detect_workspace: n outside [512, 2^27]");
    return (int64_t)kMarkOffsets * detect_tiles_(n) * kMarkPartLd;
}

extern "C" int fq3_mark_detect(const float* pcm, int64_t n, uint64_t key, float* work, int64_t work_floats, float* z, void* stream) {
    if (!pcm || !work || !z) return fq3_fail_(FQ3_EINVAL, "fq3_mark_detect: null argument");
    if (n < 2 * kMarkH || n > kMaxDetect) return fq3_fail_(FQ3_EINVAL, "fq3_mark_detect: n outside [512, 2^27]");
    const int64_t tiles = detect_tiles_(n);
    if (work_floats < (int64_t)kMarkOffsets * tiles * kMarkPartLd)
        return fq3_fail_(FQ3_EINVAL, "fq3_mark_detect: the workspace is smaller than fq3_mark_detect_workspace(n)");
    const float* tables = nullptr;
    if (int rc = device_tables_(&tables)) return rc;
    MarkDetectArgs k{};
    k.pcm = pcm; k.fwd = tables; k.part = work; k.n = n; k.T = (int)detect_frames_(n);
    k.k0 = (uint32_t)(key & 0xffffffffull); k.k1 = (uint32_t)(key >> 32);
    hipLaunchKernelGGL(mark_detect_kernel, dim3((unsigned)tiles, kMarkOffsets), dim3(kMarkThreads), 0, (hipStream_t)stream, k);
    KHIP(hipGetLastError());
    hipLaunchKernelGGL(mark_reduce_kernel, dim3(kMarkOffsets), dim3(kMarkPeriod), 0, (hipStream_t)stream, (const float*)work, (int)tiles, z);
    KHIP(hipGetLastError());
    return 0;
}

// ---- scan: per-window verdicts of up to 32 clips, two launches per call -----------------------------------------------------------------
static_assert(sizeof(fq3_mark_window) == sizeof(MarkVerdict), "fq3_mark_window is the window kernel's record");
static_assert(FQ3_STAGE_GROUP_MAX == kMarkScanMax, "the header's limit is the descriptor table's size");

extern "C" int64_t fq3_mark_scan_windows(int64_t n, int win_blocks, int hop_blocks) {
    if (n < 2 * kMarkH || n > kMaxDetect) return fq3_fail_(FQ3_EINVAL, "fq3_mark_scan_windows: n outside [512, 2^27]");
    if (int rc = scan_check_("fq3_mark_scan_windows", win_blocks, hop_blocks)) return rc;
    return scan_windows_(scan_blocks_(n), win_blocks, hop_blocks);
}

extern "C" int64_t fq3_mark_scan_workspace(int B, const int64_t* n) {
    if (int rc = scan_rows_("fq3_mark_scan_workspace", B, n)) return rc;
    int64_t blocks = 0;
    for (int b = 0; b < B; ++b) blocks += scan_blocks_(n[b]);
    return blocks * kMarkBlockDoubles;
}

extern "C" int fq3_mark_scan(int B, const float* const* pcm, const int64_t* n, const uint64_t* key, int win_blocks, int hop_blocks,
                             double* work, int64_t work_doubles, fq3_mark_window* out, float* tables, void* stream) {
    if (int rc = scan_rows_("fq3_mark_scan", B, n)) return rc;
    if (int rc = scan_check_("fq3_mark_scan", win_blocks, hop_blocks)) return rc;
    if (B == 0) return 0;
    if (!pcm || !key || !work || !out) return fq3_fail_(FQ3_EINVAL, "fq3_mark_scan: null argument");
    MarkScanArgs k{};
    int64_t blocks = 0, windows = 0;
    for (int b = 0; b < B; ++b) {
        if (!pcm[b]) return fq3_fail_(FQ3_EINVAL, "fq3_mark_scan: row " + std::to_string(b) + ": null pointer");
        MarkScanRow& r = k.rows[b];
        r.pcm = pcm[b]; r.n = (int)n[b]; r.T = (int)detect_frames_(n[b]); r.NB = (int)scan_blocks_(n[b]);
        r.W = (int)scan_windows_(r.NB, win_blocks, hop_blocks);
        r.blk0 = (int)blocks; r.win0 = (int)windows;
        r.k0 = (uint32_t)(key[b] & 0xffffffffull); r.k1 = (uint32_t)(key[b] >> 32);
        blocks += r.NB; windows += r.W;
    }
    if (work_doubles < blocks * kMarkBlockDoubles)
        return fq3_fail_(FQ3_EINVAL, "fq3_mark_scan: the workspace is smaller than fq3_mark_scan_workspace(B, n)");
    const float* dev_tables = nullptr;
    if (int rc = device_tables_(&dev_tables)) return rc;
    // The cut into (range of R blocks) x (group of G offsets) changes no result (mark_kernels.cuh): take the coarsest of these that
    // still gives the machine two workgroups per compute unit, so that few clips spread out and many clips re-use what they staged.
    static const int cuts[][2] = {{16, 8}, {8, 8}, {8, 4}, {4, 4}, {4, 2}, {2, 2}, {2, 1}};
    int64_t grid = 0;
    for (const auto& c : cuts) {
        k.R = c[0]; k.G = c[1];
        grid = 0;
        for (int b = 0; b < B; ++b) grid += (int64_t)((k.rows[b].NB + k.R - 1) / k.R) * (kMarkOffsets / k.G);
        if (grid >= 512) break;
    }
    int64_t at = 0;
    for (int b = 0; b < kMarkScanMax; ++b) {
        k.part_wg0[b] = (int)at;
        k.win_wg0[b] = b < B ? k.rows[b].win0 : (int)windows;
        if (b < B) at += (int64_t)((k.rows[b].NB + k.R - 1) / k.R) * (kMarkOffsets / k.G);
    }
    k.fwd = dev_tables; k.work = work; k.out = reinterpret_cast<MarkVerdict*>(out); k.tables = tables;
    k.win_blocks = win_blocks; k.hop_blocks = hop_blocks;
    hipLaunchKernelGGL(mark_scan_blocks_kernel, dim3((unsigned)grid), dim3(kMarkThreads), 0, (hipStream_t)stream, k);
    KHIP(hipGetLastError());
    hipLaunchKernelGGL(mark_scan_windows_kernel, dim3((unsigned)windows), dim3(kMarkScanWinThreads), 0, (hipStream_t)stream, k);
    KHIP(hipGetLastError());
    return 0;
}
