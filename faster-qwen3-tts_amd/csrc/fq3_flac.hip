// FLAC output behind the C ABI: lossless compression of the s16 output stage's samples (fq3_audio.hip) on the device.
//   fq3_flac_design / _header / _count   host only (no HIP call): block size and frame bound, the 42-byte stream header, frame count
//   fq3_flac_create / _push              streaming encoder: per push one launch pair per 64 frames (encode, then gather)
//
// The stream: `fLaC`, one STREAMINFO block, then frames of B samples (only the last one of a stream may be shorter), mono, 16 bits,
// fixed-blocksize numbering.  A frame holds one subframe -- CONSTANT, VERBATIM or FIXED of order 0..4 with partitioned 4-bit Rice
// residuals -- chosen by the exhaustive rule in include/fq3hip.h, and is never longer than 2 B + 18 bytes.  Every frame is a pure
// function of its samples, its number and the config, so the stream does not depend on how it was cut into pushes: the object holds
// back the samples behind the last whole block (fewer than B) until the next push, or the final one.
#include "../../include/fq3hip.h"
#include "flac_kernels.cuh"

#include <cstring>
#include <string>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define FHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int64_t kMaxFrames = (int64_t)1 << 31;               // what the 6-byte frame number holds
constexpr int64_t kMaxTotal = ((int64_t)1 << 36) - 1;
constexpr int64_t kMaxLength = (int64_t)1 << 50;

struct Plan { int rate, block, rate_code; };

int rate_code_(int rate) {
    switch (rate) {
        case 88200: return 1;
        case 8000: return 4;
        case 16000: return 5;
        case 22050: return 6;
        case 24000: return 7;
        case 32000: return 8;
        case 44100: return 9;
        case 48000: return 10;
        case 96000: return 11;
        default: return rate <= 65535 ? 13 : -1;
    }
}

int plan_(int rate, int block, Plan* p) {
    if (rate <= 0) return fq3_fail_(FQ3_EINVAL, "flac: the sample rate must be positive");
    const int rc = rate_code_(rate);
    if (rc < 0) return fq3_fail_(FQ3_EINVAL, "flac: " + std::to_string(rate) + " Hz has no frame-header code (a table rate, or at most 65535 Hz)");
    if (block == 0) block = rate > 16000 ? 1152 : 576;
    if (block < kFlacMinBlock || block > kFlacMaxBlock)
        return fq3_fail_(FQ3_EINVAL, "flac: block size " + std::to_string(block) + " is outside [16, 4608]");
    p->rate = rate; p->block = block; p->rate_code = rc;
    return 0;
}

inline int64_t frames_(const Plan& p, int64_t n, int final) { return final ? (n + p.block - 1) / p.block : n / p.block; }

}  // namespace

struct fq3_flac {
    Plan p{};
    int stride = 0;                   // staging slot: 2 B + 18 rounded up to four bytes
    int16_t* tail[2] = {nullptr, nullptr};
    uint8_t* stage = nullptr;         // kFlacBatch slots
    int32_t* sizes = nullptr;         // kFlacBatch frame lengths
    int64_t* totals = nullptr;        // two running byte counts of a push, used alternately by its launch pairs
    int cur = 0, tail_n = 0;
    int64_t n_in = 0, frame = 0;      // cumulative input samples / frames of the current stream
    bool finished = false;
};

extern "C" int fq3_flac_design(int sample_rate, int block_size, int* block, int* max_frame_bytes) {
    if (!block || !max_frame_bytes) return fq3_fail_(FQ3_EINVAL, "fq3_flac_design: null block / max_frame_bytes");
    Plan p{};
    if (int rc = plan_(sample_rate, block_size, &p)) return rc;
    *block = p.block;
    *max_frame_bytes = 2 * p.block + 18;
    return 0;
}

extern "C" int fq3_flac_header(int sample_rate, int block_size, int64_t total_samples, uint8_t* out, int64_t capacity) {
    if (!out) return fq3_fail_(FQ3_EINVAL, "fq3_flac_header: null output");
    Plan p{};
    if (int rc = plan_(sample_rate, block_size, &p)) return rc;
    if (total_samples < 0 || total_samples > kMaxTotal) return fq3_fail_(FQ3_EINVAL, "fq3_flac_header: total_samples outside [0, 2^36)");
    if (capacity < 42) return fq3_fail_(FQ3_EINVAL, "fq3_flac_header: capacity below 42 bytes");
    uint8_t h[42];
    std::memset(h, 0, sizeof h);
    std::memcpy(h, "fLaC", 4);
    h[4] = 0x80; h[7] = 34;                                      // last block, STREAMINFO, 24-bit length
    h[8] = h[10] = (uint8_t)(p.block >> 8); h[9] = h[11] = (uint8_t)p.block;
    // bytes 12..17: min / max frame size, unknown.  Then 20 bits of rate, 3 of channels - 1, 5 of bits - 1, 36 of total samples
    const uint64_t v = ((uint64_t)p.rate << 44) | ((uint64_t)15 << 36) | (uint64_t)total_samples;
    for (int i = 0; i < 8; ++i) h[18 + i] = (uint8_t)(v >> (56 - 8 * i));
    std::memcpy(out, h, sizeof h);                               // bytes 26..41: MD5, not computed
    return 0;
}

extern "C" int64_t fq3_flac_count(int sample_rate, int block_size, int64_t n_in, int final) {
    Plan p{};
    if (int rc = plan_(sample_rate, block_size, &p)) return rc;
    if (n_in < 0) return fq3_fail_(FQ3_EINVAL, "fq3_flac_count: negative length");
    if (n_in > kMaxLength) return fq3_fail_(FQ3_EINVAL, "fq3_flac_count: length above 2^50 samples");
    return frames_(p, n_in, final);
}

extern "C" int fq3_flac_create(const fq3_flac_config* cfg, fq3_flac** out) {
    if (!cfg || !out) return fq3_fail_(FQ3_EINVAL, "fq3_flac_create: null argument");
    Plan p{};
    if (int rc = plan_(cfg->sample_rate, cfg->block_size, &p)) return rc;
    fq3_flac* f = new fq3_flac();
    f->p = p;
    f->stride = (2 * p.block + 18 + 3) & ~3;
    hipError_t e = hipMalloc((void**)&f->tail[0], (size_t)(2 * p.block) * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc((void**)&f->stage, (size_t)kFlacBatch * f->stride);
    if (e == hipSuccess) e = hipMalloc((void**)&f->sizes, (size_t)kFlacBatch * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&f->totals, 2 * sizeof(int64_t));
    if (e != hipSuccess) {
        const std::string msg = std::string("fq3_flac_create: ") + hipGetErrorString(e);
        fq3_flac_destroy(f);
        return fq3_fail_(FQ3_EHIP, msg);
    }
    f->tail[1] = f->tail[0] + p.block;
    *out = f;
    return 0;
}

extern "C" int fq3_flac_destroy(fq3_flac* f) {
    if (!f) return 0;
    if (f->tail[0]) (void)hipFree(f->tail[0]);
    if (f->stage) (void)hipFree(f->stage);
    if (f->sizes) (void)hipFree(f->sizes);
    if (f->totals) (void)hipFree(f->totals);
    delete f;
    return 0;
}

extern "C" int fq3_flac_reset(fq3_flac* f, void* stream) {
    if (!f) return fq3_fail_(FQ3_EINVAL, "fq3_flac_reset: null object");
    (void)stream;                     // nothing to enqueue: an empty tail reads no buffer
    f->n_in = f->frame = 0;
    f->tail_n = 0;
    f->finished = false;
    return 0;
}

extern "C" int fq3_flac_push(fq3_flac* f, const int16_t* pcm, int64_t n_in, int final, uint8_t* out, int64_t capacity_bytes,
                             int64_t* n_frames, int64_t* n_bytes_dev, void* stream) {
    if (!f || !n_frames || !n_bytes_dev) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: null argument");
    if (n_in < 0 || capacity_bytes < 0 || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: bad input");
    if (f->finished) return fq3_fail_(FQ3_ESTATE, "fq3_flac_push: the stream has ended; fq3_flac_reset starts the next one");
    const Plan& p = f->p;
    if (n_in > kMaxLength - f->n_in) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: stream above 2^50 samples");
    const int64_t avail = f->tail_n + n_in;
    const int64_t frames = frames_(p, avail, final);
    if (f->frame + frames > kMaxFrames) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: stream above 2^31 frames");
    const int64_t bound = 2 * (int64_t)p.block + 18;
    if (frames > capacity_bytes / bound)
        return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: " + std::to_string(frames) + " frames of at most " + std::to_string(bound) +
                         " bytes, capacity " + std::to_string(capacity_bytes));
    if (frames > 0 && !out) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: null output");
    *n_frames = frames;
    hipStream_t s = (hipStream_t)stream;
    const int keep = final ? 0 : (int)(avail - frames * p.block);                // the tail this push leaves
    const bool copy_tail = keep > 0 && n_in > 0;                                    // n_in = 0 and no frame: the tail stays where it is
    if (frames == 0) FHIP(hipMemsetAsync(n_bytes_dev, 0, sizeof(int64_t), s));
    FlacArgs k{};
    k.pcm = pcm; k.tail = f->tail[f->cur]; k.tail_next = f->tail[f->cur ^ 1];
    k.stage = f->stage; k.sizes = f->sizes;
    k.avail = avail; k.tail_n = f->tail_n;
    k.tail_from = frames * p.block; k.tail_len = 0;
    k.block = p.block; k.stride = f->stride;
    k.rate_code = p.rate_code; k.rate_hz = p.rate;
    int64_t done = 0;
    int pair = 0;
    do {
        const int nb = (int)(frames - done < kFlacBatch ? frames - done : kFlacBatch);
        const bool last = done + nb == frames;
        k.first = done * p.block;
        k.n_frames = nb;
        k.frame0 = (uint32_t)(f->frame + done);
        k.tail_len = last && copy_tail ? keep : 0;
        const int grid = nb + (k.tail_len > 0 ? 1 : 0);
        if (grid > 0) {
            hipLaunchKernelGGL(flac_encode_kernel, dim3(grid), dim3(kFlacThreads), 0, s, k);
            FHIP(hipGetLastError());
        }
        if (nb > 0) {
            hipLaunchKernelGGL(flac_gather_kernel, dim3(nb), dim3(kFlacGatherThreads), 0, s, (const uint8_t*)f->stage, (const int32_t*)f->sizes,
                               nb, f->stride, (const int64_t*)(pair ? f->totals + ((pair - 1) & 1) : nullptr), f->totals + (pair & 1),
                               n_bytes_dev, out);
            FHIP(hipGetLastError());
        }
        done += nb;
        ++pair;
    } while (done < frames);
    if (copy_tail) f->cur ^= 1;
    f->tail_n = keep;
    f->n_in += n_in;
    f->frame += frames;
    if (final) f->finished = true;
    return 0;
}
