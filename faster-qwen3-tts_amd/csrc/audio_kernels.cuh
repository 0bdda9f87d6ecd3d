// Audio output stage (fq3_audio.hip): streaming polyphase resampler fused with the sample encoder, one launch per push.
//
// Output d of a push (d counts from the push's first output) reads K consecutive input samples ending at input index e(d) and the
// phase row p(d) of the bank:
//     y = fmaf(bank[p][K-1], x[e], ... fmaf(bank[p][1], x[e-K+2], fmaf(bank[p][0], x[e-K+1], 0.0f)))
// in exactly that order, so a sample is a function of its phase row and its K inputs only: neither the cut of the stream into pushes,
// nor the tile, nor where an input came from (the history of earlier pushes, the new chunk, or the zeros outside the stream) enters it.
// All input indices in the kernel are RELATIVE to the first sample of the new chunk: [-HL, 0) is the history (HL = K - 1 samples kept by
// the object, of which the last hist_valid are real; anything older lies before the stream and is zero), [0, n_in) the chunk, and
// [n_in, ..) the zeros after the end of a finished stream.  The absolute positions (which pass 2^31 in a long stream) stay on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fq3 {

constexpr int kAudioThreads = 256;
enum { kPcmF32 = 0, kPcmS16 = 1, kPcmMulaw = 2, kPcmAlaw = 3 };

struct AudioOutArgs {
    const float* pcm;          // the new chunk, n_in floats
    const float* hist;         // history as of before this push: relative indices [-HL, 0) at hist[0 .. HL)
    float* hist_next;          // receives the history as of after this push (the other of the object's two buffers)
    const float* bank;         // [L][K]
    void* out;
    int64_t n_in, n_out;
    int64_t e0;                // e(0): relative index of the last input the push's first output reads
    int r0;                    // ((n0 M + half) mod L) of the push's first output n0
    int p0;                    // (n0 M) mod L
    int L, M, K, HL, hist_valid;
    int shift;                 // elements by which `out` is past a 4-byte boundary
    int tile_groups;           // 4-byte output groups per workgroup
    int span_cap;              // floats of LDS reserved for the input span
    int bank_stride;           // row stride of the LDS copy of the bank
};

__device__ __forceinline__ float audio_fetch(const AudioOutArgs& a, int64_t c) {
    if (c >= 0) return c < a.n_in ? a.pcm[c] : 0.0f;
    return c >= -(int64_t)a.hist_valid ? a.hist[a.HL + c] : 0.0f;
}

// y * 32768, clamped to the int16 range, truncated toward zero (audio_io.to_pcm16)
__device__ __forceinline__ int audio_s16(float y) {
    const float v = fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f);
    return (int)v;
}

// G.711 mu-law from 16-bit linear: sign, magnitude clipped at 32635, bias 0x84, segment = position of the leading one, complemented
__device__ __forceinline__ unsigned audio_mulaw(int s) {
    const unsigned sign = s < 0 ? 0x80u : 0u;
    int mag = s < 0 ? -s : s;
    mag = (mag > 32635 ? 32635 : mag) + 0x84;
    const int seg = 24 - __clz(mag);                       // mag in [0x84, 0x7FFF]: leading one at bit 7 .. 14
    return ~(sign | ((unsigned)seg << 4) | (((unsigned)mag >> (seg + 3)) & 0xFu)) & 0xFFu;
}

// G.711 A-law from 16-bit linear: 13-bit magnitude (negative values one's-complemented), segment, even bits inverted (XOR 0x55)
__device__ __forceinline__ unsigned audio_alaw(int s) {
    int v = s >> 3;
    const unsigned mask = v >= 0 ? 0xD5u : 0x55u;
    if (v < 0) v = -v - 1;
    const int seg = v < 32 ? 0 : 27 - __clz(v);            // v in [32, 4095]: leading one at bit 5 .. 11 -> segment 1 .. 7
    const unsigned mant = (unsigned)(v >> (seg < 2 ? 1 : seg)) & 0xFu;
    return (((unsigned)seg << 4) | mant) ^ mask;
}

template <int FMT> struct AudioFmt;
template <> struct AudioFmt<kPcmF32>   { static constexpr int per = 1; };
template <> struct AudioFmt<kPcmS16>   { static constexpr int per = 2; };
template <> struct AudioFmt<kPcmMulaw> { static constexpr int per = 4; };
template <> struct AudioFmt<kPcmAlaw>  { static constexpr int per = 4; };

template <int FMT> __device__ __forceinline__ unsigned audio_encode(float y) {
    if constexpr (FMT == kPcmF32) return __float_as_uint(y);
    else if constexpr (FMT == kPcmS16) return (unsigned)audio_s16(y) & 0xFFFFu;
    else if constexpr (FMT == kPcmMulaw) return audio_mulaw(audio_s16(y));
    else return audio_alaw(audio_s16(y));
}

// One workgroup: tile_groups consecutive 4-byte words of the output (AudioFmt::per samples each; the words are aligned whatever the
// alignment of `out`, so the first and the last word of a push may be partial and are then written element by element).
// LDS: [span_cap floats: the inputs the tile reads][BANK_LDS: L rows of bank_stride floats].
// `bx` is the tile's index within its push: the single kernel and the group kernel (one push per blockIdx.y) both run this body.
template <int FMT, bool BANK_LDS>
__device__ __forceinline__ void audio_out_body(const AudioOutArgs& a, const int bx) {
    extern __shared__ float audio_lds[];
    constexpr int per = AudioFmt<FMT>::per;
    float* xs = audio_lds;
    float* bs = audio_lds + a.span_cap;
    const int tid = threadIdx.x;
    const int L = a.L, M = a.M, K = a.K;

    // the history of the NEXT push: the last HL samples of (history ++ chunk), into the other buffer -- no workgroup of this launch reads it
    if (bx == 0)
        for (int j = tid; j < a.HL; j += kAudioThreads) a.hist_next[j] = audio_fetch(a, a.n_in - a.HL + j);

    // outputs [d_a, d_b) of this tile
    const int64_t g0 = (int64_t)bx * a.tile_groups;
    int64_t d_a = g0 * per - a.shift, d_b = (g0 + a.tile_groups) * per - a.shift;
    if (d_a < 0) d_a = 0;
    if (d_b > a.n_out) d_b = a.n_out;
    if (d_a >= d_b) return;
    // 64-bit once per tile: e(d_a) = e0 + (r0 + d_a M) / L; everything below is a small offset from it
    const int64_t t_a = (int64_t)a.r0 + d_a * M;
    const int64_t e_a = a.e0 + t_a / L;
    const int r_a = (int)(t_a % L);
    const int p_a = (int)(((int64_t)a.p0 + d_a * M) % L);
    const int n_tile = (int)(d_b - d_a);
    const int64_t lo = e_a - (K - 1);
    const int span = (int)(((int64_t)r_a + (int64_t)(n_tile - 1) * M) / L) + K;      // e(d_b - 1) - lo + 1 <= span_cap
    for (int j = tid; j < span; j += kAudioThreads) xs[j] = audio_fetch(a, lo + j);
    if constexpr (BANK_LDS)
        for (int j = tid; j < L * K; j += kAudioThreads) bs[(j / K) * a.bank_stride + (j % K)] = a.bank[j];
    __syncthreads();

    for (int g = tid; g < a.tile_groups; g += kAudioThreads) {
        const int64_t d_first = (g0 + g) * per - a.shift;
        unsigned word = 0;
        int n_valid = 0;
#pragma unroll
        for (int e = 0; e < per; ++e) {
            const int64_t d = d_first + e;
            if (d < d_a || d >= d_b) continue;
            const int off = (int)(d - d_a) * M;
            const int x0 = (r_a + off) / L;                // e(d) - e_a
            const int p = (p_a + off) % L;
            const float* x = xs + x0;
            float acc = 0.0f;
            if constexpr (BANK_LDS) {
                const float* h = bs + p * a.bank_stride;
                for (int k = 0; k < K; ++k) acc = fmaf(h[k], x[k], acc);
            } else {
                const float* h = a.bank + (size_t)p * K;
                for (int k = 0; k < K; ++k) acc = fmaf(h[k], x[k], acc);
            }
            const unsigned v = audio_encode<FMT>(acc);
            if constexpr (per == 1) word = v;
            else word |= v << (e * (32 / per));
            ++n_valid;
        }
        if (n_valid == per) {
            // a whole aligned word
            reinterpret_cast<unsigned*>(reinterpret_cast<char*>(a.out) + d_first * (4 / per))[0] = word;
        } else if constexpr (per > 1) {
            // partial first / last word of the push: element stores
#pragma unroll
            for (int e = 0; e < per; ++e) {
                const int64_t d = d_first + e;
                if (d < d_a || d >= d_b) continue;
                const unsigned v = word >> (e * (32 / per));
                if constexpr (per == 2) reinterpret_cast<unsigned short*>(a.out)[d] = (unsigned short)v;
                else reinterpret_cast<unsigned char*>(a.out)[d] = (unsigned char)v;
            }
        }
    }
}

template <int FMT, bool BANK_LDS>
__global__ void __launch_bounds__(kAudioThreads) audio_out_kernel(const AudioOutArgs a) {
    audio_out_body<FMT, BANK_LDS>(a, (int)blockIdx.x);
}

// ---- a group of pushes in one launch (fq3_audio_out_push_group) ----
// Grid (the largest tile count over the rows, B): blockIdx.y picks the row, blockIdx.x the tile of that row's push.  The rows share one
// design -- the bank and the launch plan -- and differ in everything a push derives from its object's state.  The descriptors travel
// BY VALUE in the kernel's argument block: blockIdx.y is uniform, so a row's fields are scalar loads from the argument segment at a
// scalar offset, no table in device memory has to be filled (and kept alive) per call, and nothing is copied.  Workgroups past a row's
// last tile leave before the barrier; workgroup x = 0 of every row writes that row's next history, outputs or not.
constexpr int kAudioGroupMax = 32;              // FQ3_STAGE_GROUP_MAX

struct AudioRow {
    const float* pcm;
    const float* hist;
    float* hist_next;
    void* out;
    int64_t n_in, n_out, e0;
    int r0, p0, hist_valid, shift;
};

struct AudioGroupArgs {
    const float* bank;
    int L, M, K, HL, tile_groups, span_cap, bank_stride;
    AudioRow rows[kAudioGroupMax];
};
static_assert(sizeof(AudioRow) == 72 && sizeof(AudioGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

template <int FMT, bool BANK_LDS>
__global__ void __launch_bounds__(kAudioThreads) audio_out_group_kernel(const AudioGroupArgs g) {
    const AudioRow& r = g.rows[blockIdx.y];
    AudioOutArgs a;
    a.pcm = r.pcm; a.hist = r.hist; a.hist_next = r.hist_next; a.bank = g.bank; a.out = r.out;
    a.n_in = r.n_in; a.n_out = r.n_out; a.e0 = r.e0; a.r0 = r.r0; a.p0 = r.p0;
    a.L = g.L; a.M = g.M; a.K = g.K; a.HL = g.HL; a.hist_valid = r.hist_valid; a.shift = r.shift;
    a.tile_groups = g.tile_groups; a.span_cap = g.span_cap; a.bank_stride = g.bank_stride;
    audio_out_body<FMT, BANK_LDS>(a, (int)blockIdx.x);
}

}  // namespace fq3
