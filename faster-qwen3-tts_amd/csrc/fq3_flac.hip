// FLAC output behind the C ABI: lossless compression of the s16 output stage's samples (fq3_audio.hip) on the device.
//   fq3_flac_design / _header / _count   host only (no HIP call): block size and frame bound, the 42-byte stream header, frame count
//   fq3_flac_create / _push              streaming encoder: per push one launch pair per 64 frames (encode, then gather)
//   fq3_flac_push_group                  the pushes of up to 32 objects of one design in ONE launch pair per 64 frames, each row bit for
//                                        bit its single push
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

namespace {

// what a push does, worked out from the object's state without changing it
struct Push {
    int64_t avail, frames;
    int keep;                         // the tail this push leaves
    bool copy_tail;                   // n_in = 0 and no frame: the tail stays where it is
};

int check_push_(const std::string& who, const fq3_flac* f, const int16_t* pcm, int64_t n_in, int final, const uint8_t* out,
                int64_t capacity_bytes, Push* q) {
    if (n_in < 0 || capacity_bytes < 0 || (n_in > 0 && !pcm)) return fq3_fail_(FQ3_EINVAL, who + ": bad input");
    if (f->finished) return fq3_fail_(FQ3_ESTATE, who + ": the stream has ended; fq3_flac_reset starts the next one");
    const Plan& p = f->p;
    if (n_in > kMaxLength - f->n_in) return fq3_fail_(FQ3_EINVAL, who + ": stream above 2^50 samples");
    q->avail = f->tail_n + n_in;
    q->frames = frames_(p, q->avail, final);
    if (f->frame + q->frames > kMaxFrames) return fq3_fail_(FQ3_EINVAL, who + ": stream above 2^31 frames");
    const int64_t bound = 2 * (int64_t)p.block + 18;
    if (q->frames > capacity_bytes / bound)
        return fq3_fail_(FQ3_EINVAL, who + ": " + std::to_string(q->frames) + " frames of at most " + std::to_string(bound) +
                         " bytes, capacity " + std::to_string(capacity_bytes));
    if (q->frames > 0 && !out) return fq3_fail_(FQ3_EINVAL, who + ": null output");
    q->keep = final ? 0 : (int)(q->avail - q->frames * p.block);
    q->copy_tail = q->keep > 0 && n_in > 0;
    return 0;
}

void commit_push_(fq3_flac* f, const Push& q, int64_t n_in, int final) {
    if (q.copy_tail) f->cur ^= 1;
    f->tail_n = q.keep;
    f->n_in += n_in;
    f->frame += q.frames;
    if (final) f->finished = true;
}

}  // namespace

extern "C" int fq3_flac_push(fq3_flac* f, const int16_t* pcm, int64_t n_in, int final, uint8_t* out, int64_t capacity_bytes,
                             int64_t* n_frames, int64_t* n_bytes_dev, void* stream) {
    if (!f || !n_frames || !n_bytes_dev) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push: null argument");
    Push q{};
    if (int rc = check_push_("fq3_flac_push", f, pcm, n_in, final, out, capacity_bytes, &q)) return rc;
    const Plan& p = f->p;
    const int64_t frames = q.frames;
    *n_frames = frames;
    hipStream_t s = (hipStream_t)stream;
    if (frames == 0) FHIP(hipMemsetAsync(n_bytes_dev, 0, sizeof(int64_t), s));
    FlacArgs k{};
    k.pcm = pcm; k.tail = f->tail[f->cur]; k.tail_next = f->tail[f->cur ^ 1];
    k.stage = f->stage; k.sizes = f->sizes;
    k.avail = q.avail; k.tail_n = f->tail_n;
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
        k.tail_len = last && q.copy_tail ? q.keep : 0;
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
    commit_push_(f, q, n_in, final);
    return 0;
}

// The pushes of up to FQ3_STAGE_GROUP_MAX objects of one design: per round of 64 frames ONE encode launch and ONE gather launch over the
// rows that have frames (or a tail to copy, or a byte count of 0 to write) in that round.  Everything a row's workgroups read is what
// its single push would hand them, so the bytes, the counts and the objects' state are those of B single pushes.
extern "C" int fq3_flac_push_group(fq3_flac* const* objs, int B, const int16_t* const* pcm, const int64_t* n_in, const int* final,
                                   uint8_t* const* out, const int64_t* capacity_bytes, int64_t* n_frames, int64_t* const* n_bytes_dev,
                                   void* stream) {
    if (B < 0 || B > FQ3_STAGE_GROUP_MAX)
        return fq3_fail_(FQ3_EINVAL, "fq3_flac_push_group: B = " + std::to_string(B) + "; a group has 0 to " + std::to_string(FQ3_STAGE_GROUP_MAX) + " rows");
    if (B == 0) return 0;
    if (!objs || !pcm || !n_in || !final || !out || !capacity_bytes || !n_frames || !n_bytes_dev)
        return fq3_fail_(FQ3_EINVAL, "fq3_flac_push_group: null array");
    for (int b = 0; b < B; ++b) {
        if (!objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push_group: row " + std::to_string(b) + ": null object");
        for (int c = 0; c < b; ++c)
            if (objs[c] == objs[b]) return fq3_fail_(FQ3_EINVAL, "fq3_flac_push_group: rows " + std::to_string(c) + " and " + std::to_string(b) + " are the same object");
        if (objs[b]->p.rate != objs[0]->p.rate || objs[b]->p.block != objs[0]->p.block)
            return fq3_fail_(FQ3_EINVAL, "fq3_flac_push_group: row " + std::to_string(b) + " has another design (sample rate, block size) than row 0");
    }
    // every row is checked and planned before any object moves
    static_assert(FQ3_STAGE_GROUP_MAX == kFlacGroupMax, "the header's limit is the descriptor table's size");
    Push q[FQ3_STAGE_GROUP_MAX];
    int64_t rounds = 1;
    for (int b = 0; b < B; ++b) {
        const std::string who = "fq3_flac_push_group: row " + std::to_string(b);
        if (!n_bytes_dev[b]) return fq3_fail_(FQ3_EINVAL, who + ": null n_bytes_dev");
        if (int rc = check_push_(who, objs[b], pcm[b], n_in[b], final[b], out[b], capacity_bytes[b], &q[b])) return rc;
        const int64_t need = (q[b].frames + kFlacBatch - 1) / kFlacBatch;
        if (need > rounds) rounds = need;
    }
    const Plan& p = objs[0]->p;
    hipStream_t s = (hipStream_t)stream;
    FlacGroupArgs g{};
    g.block = p.block; g.stride = objs[0]->stride; g.rate_code = p.rate_code; g.rate_hz = p.rate;
    for (int b = 0; b < B; ++b) {
        const fq3_flac* f = objs[b];
        FlacGroupRow& r = g.rows[b];
        r.pcm = pcm[b]; r.tail = f->tail[f->cur]; r.tail_next = f->tail[f->cur ^ 1];
        r.stage = f->stage; r.sizes = f->sizes; r.totals = f->totals;
        r.n_bytes = n_bytes_dev[b]; r.out = out[b];
        r.avail = q[b].avail; r.tail_from = q[b].frames * p.block; r.tail_n = f->tail_n;
    }
    for (int64_t round = 0; round < rounds; ++round) {
        const int64_t done = round * kFlacBatch;
        g.first = done * p.block;
        g.round = (int)round;                                 // below 2^25: a stream has at most 2^31 frames
        int enc = 0, gat = 0;
        for (int b = 0; b < B; ++b) {
            FlacGroupRow& r = g.rows[b];
            const int64_t frames = q[b].frames, left = frames - done;
            const int nb = (int)(left < 0 ? 0 : left < kFlacBatch ? left : kFlacBatch);
            const bool last = round == (frames > 0 ? (frames - 1) / kFlacBatch : 0);
            r.n_frames = nb;
            r.frame0 = (uint32_t)(objs[b]->frame + done);
            r.tail_len = last && q[b].copy_tail ? q[b].keep : 0;
            g.enc_wg0[b] = enc;
            g.gat_wg0[b] = gat;
            enc += nb + (r.tail_len > 0 ? 1 : 0);
            gat += nb + (round == 0 && frames == 0 ? 1 : 0);  // a push without a frame: the workgroup that writes its byte count of 0
        }
        for (int b = B; b < FQ3_STAGE_GROUP_MAX; ++b) { g.enc_wg0[b] = enc; g.gat_wg0[b] = gat; }
        if (enc > 0) {
            hipLaunchKernelGGL(flac_encode_group_kernel, dim3(enc), dim3(kFlacThreads), 0, s, g);
            FHIP(hipGetLastError());
        }
        if (gat > 0) {
            hipLaunchKernelGGL(flac_gather_group_kernel, dim3(gat), dim3(kFlacGatherThreads), 0, s, g);
            FHIP(hipGetLastError());
        }
    }
    for (int b = 0; b < B; ++b) {
        n_frames[b] = q[b].frames;
        commit_push_(objs[b], q[b], n_in[b], final[b]);
    }
    return 0;
}
