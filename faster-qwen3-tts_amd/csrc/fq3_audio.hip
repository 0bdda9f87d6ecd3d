// Audio output stage behind the C ABI: what happens to the vocoder's float32 PCM before it leaves the device.
//   fq3_audio_out_design / _count   host only (no HIP call): the polyphase bank of a rate pair and the stream's output count
//   fq3_audio_out_create / _push    streaming resampler + sample encoder (f32, s16, G.711 mu-law / A-law), ONE launch per push
//   fq3_audio_out_push_group        the pushes of up to 32 objects of one design in ONE launch, each row bit for bit its single push
//
// The rate pair in_rate -> out_rate reduces to L / M (L = out / g, M = in / g, g = gcd).  The prototype is a Kaiser-windowed sinc of
// half length half = Z m (m = max(L, M), Z zero crossings a side), cutoff rho / m of the up-sampled Nyquist, scaled to sum L; phase
// row p of the bank holds its taps p' + t L in the order in which they meet ASCENDING input samples.  Output n stands at input time
// n M / L (zero phase):
//     e(n) = floor((n M + half) / L)                 the last input sample output n reads
//     p(n) = (n M) mod L
//     y[n] = sum_k bank[p(n)][k] x[e(n) - (K - 1) + k],        x = 0 outside the stream
// An output exists as soon as e(n) is below the cumulative input length, so the count is a function of that length alone; a finished
// stream of N samples has ceil(N L / M) outputs (the samples past its end are zeros).
#include "../../include/fq3hip.h"
#include "audio_kernels.cuh"

#include <cmath>
#include <string>
#include <vector>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define AHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kMaxRatioTerm = 320;          // L and M
constexpr int kDefaultZero = 16, kMaxZero = 64;
constexpr int kMaxTaps = 12288;             // K: the inputs of even the smallest tile must fit the span's LDS
constexpr double kBeta = 8.0, kRho = 0.96;
constexpr int kLdsFloats = 16384;           // 64 KiB: what a launch gets without raising the kernel's limit
constexpr int kBankLdsFloats = 12288;       // the bank is staged when its padded copy is at most this
constexpr int kTileOutputs = 1024;

struct Ratio { int L, M, K, half; };

int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

int ratio_(int in_rate, int out_rate, int zero_crossings, Ratio* r) {
    if (in_rate <= 0 || out_rate <= 0) return fq3_fail_(FQ3_EINVAL, "audio out: sample rates must be positive");
    if (zero_crossings < 0 || zero_crossings > kMaxZero) return fq3_fail_(FQ3_EINVAL, "audio out: zero_crossings must be in [0, 64] (0 = 16)");
    const int64_t g = gcd64(in_rate, out_rate);
    const int64_t L = out_rate / g, M = in_rate / g;
    if (L > kMaxRatioTerm || M > kMaxRatioTerm)
        return fq3_fail_(FQ3_EINVAL, "audio out: " + std::to_string(in_rate) + " -> " + std::to_string(out_rate) + " Hz reduces to " +
                         std::to_string(L) + "/" + std::to_string(M) + "; both terms must be at most 320");
    r->L = (int)L; r->M = (int)M;
    if (L == 1 && M == 1) { r->K = 1; r->half = 0; return 0; }
    const int Z = zero_crossings ? zero_crossings : kDefaultZero;
    const int64_t m = L > M ? L : M;
    const int64_t half = Z * m, K = (2 * half + 1 + L - 1) / L;
    if (K > kMaxTaps) return fq3_fail_(FQ3_EINVAL, "audio out: " + std::to_string(K) + " taps per output; at most 12288 (fewer zero crossings, or a milder ratio)");
    r->K = (int)K; r->half = (int)half;
    return 0;
}

// modified Bessel function of the first kind, order 0, by its power series
double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

void design_bank_(const Ratio& r, float* bank) {
    if (r.L == 1 && r.M == 1) { bank[0] = 1.0f; return; }
    const int L = r.L, K = r.K, half = r.half, n = 2 * half + 1;
    const double fc = kRho / (double)(L > r.M ? L : r.M), pi = 3.14159265358979323846, i0b = bessel_i0(kBeta);
    std::vector<double> h(n);
    double sum = 0.0;
    for (int j = 0; j < n; ++j) {
        const double t = (double)(j - half), u = t / (double)half;
        const double w = bessel_i0(kBeta * std::sqrt(std::fmax(0.0, 1.0 - u * u))) / i0b;
        const double s = t == 0.0 ? 1.0 : std::sin(pi * fc * t) / (pi * fc * t);
        h[j] = fc * s * w;
        sum += h[j];
    }
    const double scale = (double)L / sum;
    // row p, tap k (ascending input sample): prototype index j0 + (K - 1 - k) L with j0 = (p + half) mod L; past the prototype's end: 0
    for (int p = 0; p < L; ++p) {
        const int j0 = (p + half) % L;
        for (int k = 0; k < K; ++k) {
            const int j = j0 + (K - 1 - k) * L;
            bank[(size_t)p * K + k] = j < n ? (float)(h[j] * scale) : 0.0f;
        }
    }
}

// outputs that exist once n_in samples have been pushed (n_in >= 0)
int64_t count_(const Ratio& r, int64_t n_in, int final) {
    const int64_t num = n_in * r.L - (final ? 0 : r.half);
    return num <= 0 ? 0 : (num + r.M - 1) / r.M;
}

template <int FMT> void launch_(bool bank_lds, int blocks, size_t shm, hipStream_t s, const AudioOutArgs& a) {
    if (bank_lds) hipLaunchKernelGGL((audio_out_kernel<FMT, true>), dim3(blocks), dim3(kAudioThreads), shm, s, a);
    else hipLaunchKernelGGL((audio_out_kernel<FMT, false>), dim3(blocks), dim3(kAudioThreads), shm, s, a);
}

}  // namespace

struct fq3_audio_out {
    fq3_audio_out_config cfg{};
    Ratio r{};
    int HL = 0;                       // history length: K - 1
    float* bank = nullptr;            // device [L][K]
    float* hist[2] = {nullptr, nullptr};
    int cur = 0, hist_valid = 0;
    int64_t n_in = 0, n_out = 0;      // cumulative input / output samples of the current stream
    bool finished = false;
    // launch plan (fixed per object)
    int tile_outputs = 0, span_cap = 0, bank_stride = 0;
    bool bank_lds = false;
};

extern "C" int fq3_audio_out_design(int in_rate, int out_rate, int zero_crossings, int* L, int* M, int* K, float* bank, int64_t capacity) {
    if (!L || !M || !K) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_design: null L / M / K");
    Ratio r{};
    if (int rc = ratio_(in_rate, out_rate, zero_crossings, &r)) return rc;
    *L = r.L; *M = r.M; *K = r.K;
    if (bank) {
        if (capacity < (int64_t)r.L * r.K) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_design: bank capacity below L * K floats");
        design_bank_(r, bank);
    }
    return 0;
}

extern "C" int64_t fq3_audio_out_count(int in_rate, int out_rate, int zero_crossings, int64_t n_in, int final) {
    Ratio r{};
    if (int rc = ratio_(in_rate, out_rate, zero_crossings, &r)) return rc;
    if (n_in < 0) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_count: negative length");
    return count_(r, n_in, final);
}

extern "C" int fq3_audio_out_create(const fq3_audio_out_config* cfg, fq3_audio_out** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_create: null argument");
    if (cfg->format < FQ3_PCM_F32 || cfg->format > FQ3_PCM_ALAW) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_create: unknown format");
    Ratio r{};
    if (int rc = ratio_(cfg->in_rate, cfg->out_rate, cfg->zero_crossings, &r)) return rc;
    fq3_audio_out* a = new fq3_audio_out();
    a->cfg = *cfg; a->r = r; a->HL = r.K - 1;
    // plan: the largest tile whose input span fits beside the staged bank; a bank that leaves no room for a span stays in global memory
    const int per = cfg->format == FQ3_PCM_F32 ? 1 : cfg->format == FQ3_PCM_S16 ? 2 : 4;
    a->bank_stride = r.K | 1;                                  // odd row stride: the phases of neighbouring outputs in different LDS banks
    a->bank_lds = (int64_t)r.L * a->bank_stride <= kBankLdsFloats;
    for (;;) {
        const int avail = kLdsFloats - (a->bank_lds ? r.L * a->bank_stride : 0);
        int tile = kTileOutputs;
        auto span_of = [&](int t) { return (int)(((int64_t)(r.L - 1) + (int64_t)(t - 1) * r.M) / r.L) + r.K; };
        while (tile > per && span_of(tile) > avail) tile /= 2;
        if (span_of(tile) <= avail) { a->tile_outputs = tile; a->span_cap = span_of(tile); break; }
        if (!a->bank_lds) { delete a; return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_create: filter too long for the LDS"); }
        a->bank_lds = false;
    }
    std::vector<float> bank((size_t)r.L * r.K);
    design_bank_(r, bank.data());
    hipError_t e = hipMalloc((void**)&a->bank, bank.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&a->hist[0], (size_t)(2 * a->HL + 2) * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(a->bank, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_audio_out_create: ") + hipGetErrorString(e);
        fq3_audio_out_destroy(a);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    a->hist[1] = a->hist[0] + a->HL + 1;
    *out = a;
    return 0;
}

extern "C" int fq3_audio_out_destroy(fq3_audio_out* a) {
    if (!a) return 0;
    if (a->bank) (void)hipFree(a->bank);
    if (a->hist[0]) (void)hipFree(a->hist[0]);
    delete a;
    return 0;
}

extern "C" int fq3_audio_out_reset(fq3_audio_out* a, void* stream) {
    if (!a) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_reset: null object");
    (void)stream;                     // nothing to enqueue: with hist_valid = 0 the next push reads the history as the zeros before the stream
    a->n_in = a->n_out = 0;
    a->hist_valid = 0;
    a->finished = false;
    return 0;
}

namespace {

// One push, in the three steps the single and the group entry share, so that a row of a group IS a single push:
//   check_push_   every refusal, and the number of outputs; the object does not change
//   plan_push_    what the launch reads of the object's state (AudioOutArgs; a group copies the per-row part into its descriptor)
//   commit_push_  the object after the launch was enqueued
int check_push_(const std::string& who, const fq3_audio_out* a, const float* pcm, int64_t n_in, int final, const void* out,
                int64_t capacity_samples, int64_t* cnt_out) {
    if (n_in < 0 || capacity_samples < 0 || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (a->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_audio_out_reset starts the next one");
    const int64_t cnt = count_(a->r, a->n_in + n_in, final) - a->n_out;
    if (cnt > capacity_samples)
        return fq3_fail_(FQ3_EINVAL, who + ": " + std::to_string(cnt) + " output samples, capacity " + std::to_string(capacity_samples));
    if (cnt > 0 && !out) return fq3_fail_(FQ3_EINVAL, who + ": null output");
    *cnt_out = cnt;
    return 0;
}

inline int per_word_(int fmt) { return fmt == FQ3_PCM_F32 ? 1 : fmt == FQ3_PCM_S16 ? 2 : 4; }
inline bool has_work_(const fq3_audio_out* a, int64_t n_in, int64_t cnt) { return cnt > 0 || (n_in > 0 && a->HL > 0); }
inline size_t lds_bytes_(const fq3_audio_out* a) {
    return ((size_t)a->span_cap + (a->bank_lds ? (size_t)a->r.L * a->bank_stride : 0)) * sizeof(float);
}

// -> workgroups of the push (at least one: x = 0 writes the next history)
int64_t plan_push_(const fq3_audio_out* a, const float* pcm, int64_t n_in, void* out, int64_t cnt, AudioOutArgs* kp) {
    const Ratio& r = a->r;
    const int per = per_word_(a->cfg.format);
    AudioOutArgs& k = *kp;
    k.pcm = pcm; k.hist = a->hist[a->cur]; k.hist_next = a->hist[a->cur ^ 1]; k.bank = a->bank; k.out = out;
    k.n_in = n_in; k.n_out = cnt;
    const int64_t u0 = a->n_out * r.M;                    // 64-bit: hours of audio pass 2^31
    k.e0 = (u0 + r.half) / r.L - a->n_in;
    k.r0 = (int)((u0 + r.half) % r.L);
    k.p0 = (int)(u0 % r.L);
    k.L = r.L; k.M = r.M; k.K = r.K; k.HL = a->HL; k.hist_valid = a->hist_valid;
    k.shift = (int)(((uintptr_t)out / (uintptr_t)(4 / per)) % (uintptr_t)per);
    k.tile_groups = a->tile_outputs / per;
    k.span_cap = a->span_cap; k.bank_stride = a->bank_stride;
    const int64_t groups = (cnt + k.shift + per - 1) / per;
    return groups > 0 ? (groups + k.tile_groups - 1) / k.tile_groups : 1;
}

void commit_push_(fq3_audio_out* a, int64_t n_in, int64_t cnt, int final, bool launched) {
    const int64_t total = a->n_in + n_in;
    if (launched && a->HL > 0 && n_in > 0) {
        a->cur ^= 1;
        a->hist_valid = (int)(total < a->HL ? total : a->HL);
    }
    a->n_in = total;
    a->n_out += cnt;
    if (final) a->finished = true;
}

template <int FMT> void launch_group_(bool bank_lds, dim3 grid, size_t shm, hipStream_t s, const AudioGroupArgs& g) {
    if (bank_lds) hipLaunchKernelGGL((audio_out_group_kernel<FMT, true>), grid, dim3(kAudioThreads), shm, s, g);
    else hipLaunchKernelGGL((audio_out_group_kernel<FMT, false>), grid, dim3(kAudioThreads), shm, s, g);
}

}  // namespace

extern "C" int fq3_audio_out_push(fq3_audio_out* a, const float* pcm, int64_t n_in, int final, void* out, int64_t capacity_samples,
                                  int64_t* n_out, void* stream) {
    if (!a || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push: null argument");
    int64_t cnt = 0;
    if (int rc = check_push_("fq3_audio_out_push", a, pcm, n_in, final, out, capacity_samples, &cnt)) return rc;
    *n_out = cnt;
    const bool work = has_work_(a, n_in, cnt);
    if (work) {
        AudioOutArgs k{};
        const int64_t blocks = plan_push_(a, pcm, n_in, out, cnt, &k);
        if (blocks > 0x7FFFFFFF) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push: chunk too long for one launch");
        const size_t shm = lds_bytes_(a);
        hipStream_t s = (hipStream_t)stream;
        switch (a->cfg.format) {
            case FQ3_PCM_F32: launch_<kPcmF32>(a->bank_lds, (int)blocks, shm, s, k); break;
            case FQ3_PCM_S16: launch_<kPcmS16>(a->bank_lds, (int)blocks, shm, s, k); break;
            case FQ3_PCM_MULAW: launch_<kPcmMulaw>(a->bank_lds, (int)blocks, shm, s, k); break;
            default: launch_<kPcmAlaw>(a->bank_lds, (int)blocks, shm, s, k); break;
        }
        AHIP(hipGetLastError());
    }
    commit_push_(a, n_in, cnt, final, work);
    return 0;
}

extern "C" int fq3_audio_out_push_group(fq3_audio_out* const* objs, int B, const float* const* pcm, const int64_t* n_in, const int* final,
                                        void* const* out, const int64_t* capacity_samples, int64_t* n_out, void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !final || !out || !capacity_samples || !n_out) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
        const fq3_audio_out_config &x = objs[0]->cfg, &y = objs[b]->cfg;
        if (x.in_rate != y.in_rate || x.out_rate != y.out_rate || x.format != y.format || x.zero_crossings != y.zero_crossings)
            return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push_group: row " + std::to_string(b) + " has another design (rates, format, zero crossings) than row 0");
    }
    // every row is checked and planned before any object moves
    static_assert(FQ3_STAGE_GROUP_MAX == kAudioGroupMax, "the header's limit is the descriptor table's size");
    const fq3_audio_out* a0 = objs[0];
    AudioGroupArgs g{};
    int64_t cnt[FQ3_STAGE_GROUP_MAX], blocks_max = 1;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const fq3_audio_out* a = objs[b];
        if (int rc = check_push_("fq3_audio_out_push_group: row " + std::to_string(b), a, pcm[b], n_in[b], final[b], out[b], capacity_samples[b], &cnt[b]))
            return rc;
        AudioOutArgs k{};
        const int64_t blocks = plan_push_(a, pcm[b], n_in[b], out[b], cnt[b], &k);
        if (blocks > 0x7FFFFFFF) return fq3_fail_(FQ3_EINVAL, "fq3_audio_out_push_group: row " + std::to_string(b) + ": chunk too long for one launch");
        if (blocks > blocks_max) blocks_max = blocks;
        any = any || has_work_(a, n_in[b], cnt[b]);
        AudioRow& r = g.rows[b];
        r.pcm = k.pcm; r.hist = k.hist; r.hist_next = k.hist_next; r.out = k.out;
        r.n_in = k.n_in; r.n_out = k.n_out; r.e0 = k.e0; r.r0 = k.r0; r.p0 = k.p0; r.hist_valid = k.hist_valid; r.shift = k.shift;
        if (b == 0) {
            g.bank = k.bank; g.L = k.L; g.M = k.M; g.K = k.K; g.HL = k.HL;
            g.tile_groups = k.tile_groups; g.span_cap = k.span_cap; g.bank_stride = k.bank_stride;
        }
    }
    if (any) {
        const dim3 grid((unsigned)blocks_max, (unsigned)B);
        const size_t shm = lds_bytes_(a0);
        hipStream_t s = (hipStream_t)stream;
        switch (a0->cfg.format) {
            case FQ3_PCM_F32: launch_group_<kPcmF32>(a0->bank_lds, grid, shm, s, g); break;
            case FQ3_PCM_S16: launch_group_<kPcmS16>(a0->bank_lds, grid, shm, s, g); break;
            case FQ3_PCM_MULAW: launch_group_<kPcmMulaw>(a0->bank_lds, grid, shm, s, g); break;
            default: launch_group_<kPcmAlaw>(a0->bank_lds, grid, shm, s, g); break;
        }
        AHIP(hipGetLastError());
    }
    for (int b = 0; b < B; ++b) {
        n_out[b] = cnt[b];
        // a row without work was not worth a launch of its own and moves as its single push would: the history stays where it is
        commit_push_(objs[b], n_in[b], cnt[b], final[b], has_work_(objs[b], n_in[b], cnt[b]));
    }
    return 0;
}
