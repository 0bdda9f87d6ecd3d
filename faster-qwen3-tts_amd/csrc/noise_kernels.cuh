// Seeded sampling noise: the Exp(1) variates the samplers divide by (sampler.cuh), as a pure function of
// (seed, emitted-frame index, slot, vocabulary index), generated on the device by a counter-based generator.  No state, no LDS, no
// atomics: every thread computes its own eight elements from two Philox calls and writes them with plain vector stores.
//
// THE CONTRACT (a seed in a log must give the same audio after any later change):
//   generator   Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85
//   key         (seed & 0xffffffff, seed >> 32), seed an unsigned 64-bit integer
//   counter     (v >> 2, frame, slot, 0); the variate of vocabulary index v comes from output word v & 3
//   frame       the emitted-frame index the samplers call st->frame; talker and predictor samplers of a frame read ring row
//               frame % noise_frames
//   slot        0: the talker's row of that frame; 1 + cb: predictor codebook cb in 0 .. G-2; 0xFFFFFFFF with frame 0: the first
//               token after the prefill
//   variate     k = word >> 9; u = (2 k + 1) 2^-24 (exact in fp32, inside (0, 1)); e = -ln(u) in fp64, rounded once to fp32
//               (nearest even) and, for a bf16 context, once more to bf16.  Range [5.96e-8, 16.64]: never zero, never infinite.
#pragma once
#include "fq3_common.cuh"

namespace fq3 {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr uint32_t kNoiseFirstSlot = 0xFFFFFFFFu;

struct Philox4 { uint32_t x, y, z, w; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ float noise_variate(uint32_t word) {
    const double u = (double)(2u * (word >> 9) + 1u) * 0x1p-24;
    return (float)(-log(u));
}

// elements [8 g, 8 g + 8) of one row: two Philox calls
__device__ __forceinline__ void noise_group8(uint32_t g, uint32_t frame, uint32_t slot, uint32_t k0, uint32_t k1, float (&f)[8]) {
    const Philox4 a = philox4x32_10(2u * g, frame, slot, 0u, k0, k1), b = philox4x32_10(2u * g + 1u, frame, slot, 0u, k0, k1);
    f[0] = noise_variate(a.x); f[1] = noise_variate(a.y); f[2] = noise_variate(a.z); f[3] = noise_variate(a.w);
    f[4] = noise_variate(b.x); f[5] = noise_variate(b.y); f[6] = noise_variate(b.z); f[7] = noise_variate(b.w);
}

// group g of a row of V elements: one 16-byte store (bf16) or two (fp32) where the eight elements exist and the destination is
// 16-byte aligned, element by element otherwise (the tail of a row that is no multiple of eight, a row that starts off alignment)
template <typename T>
__device__ __forceinline__ void noise_store_group(T* row, int V, uint32_t g, uint32_t frame, uint32_t slot, uint32_t k0, uint32_t k1) {
    float f[8];
    noise_group8(g, frame, slot, k0, k1, f);
    const int v0 = (int)(g * 8u);
    T* p = row + v0;
    if (v0 + 8 <= V && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        DT<T>::st8(p, f);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (v0 + j < V) DT<T>::st(p + j, f[j]);
    }
}

// By-value descriptor of one fill launch (as PackCont in the packed continuation prefill): nothing is staged through device memory.
constexpr int kNoiseMaxRings = 32;
struct NoiseRings {
    void* talker[kNoiseMaxRings];                   // [ring_frames][V] or null
    void* pred[kNoiseMaxRings];                     // [ring_frames][G - 1][Vp] or null
    uint32_t key0[kNoiseMaxRings], key1[kNoiseMaxRings];
    uint32_t first_frame[kNoiseMaxRings];
    int n_frames[kNoiseMaxRings];
    int ring_frames, V, G1, Vp;                     // G1 = G - 1 predictor codebooks
};

// Grid (eight-element groups of one frame / 256, rows, lanes).  The groups of a frame: ceil(V / 8) of the talker row, then
// ceil(Vp / 8) of each predictor row.  Row j of lane q is frame first_frame + j, written at ring row (first_frame + j) % ring_frames.
template <typename T>
__global__ __launch_bounds__(256) void noise_fill_kernel(NoiseRings nr) {
    const int q = blockIdx.z, j = blockIdx.y;
    if (j >= nr.n_frames[q]) return;
    const int gT = (nr.V + 7) >> 3, gP = (nr.Vp + 7) >> 3;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= gT + nr.G1 * gP) return;
    const uint64_t fr = (uint64_t)nr.first_frame[q] + (uint64_t)j;
    const uint32_t frame = (uint32_t)fr;
    const size_t row = (size_t)(fr % (uint64_t)nr.ring_frames);
    if (g < gT) {
        T* t = gptr(reinterpret_cast<T*>(nr.talker[q]));
        if (t) noise_store_group<T>(t + row * nr.V, nr.V, (uint32_t)g, frame, 0u, nr.key0[q], nr.key1[q]);
    } else {
        T* p = gptr(reinterpret_cast<T*>(nr.pred[q]));
        const int cb = (g - gT) / gP, gg = (g - gT) - cb * gP;
        if (p) noise_store_group<T>(p + (row * nr.G1 + cb) * nr.Vp, nr.Vp, (uint32_t)gg, frame, 1u + (uint32_t)cb, nr.key0[q], nr.key1[q]);
    }
}

// one row of V elements (the first-token row)
template <typename T>
__global__ __launch_bounds__(256) void noise_row_kernel(T* out, int V, uint32_t frame, uint32_t slot, uint32_t k0, uint32_t k1) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ((V + 7) >> 3)) return;
    noise_store_group<T>(out, V, (uint32_t)g, frame, slot, k0, k1);
}

// the raw words of one row: thread t writes words [4 t, 4 t + 4) of the row that lie below V
__global__ __launch_bounds__(256) void noise_words_kernel(uint32_t* out, int64_t V, uint32_t frame, uint32_t slot, uint32_t k0, uint32_t k1) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t v0 = t * 4;
    if (v0 >= V) return;
    const Philox4 a = philox4x32_10((uint32_t)t, frame, slot, 0u, k0, k1);
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (v0 + j < V) out[v0 + j] = w[j];
}

}  // namespace fq3
