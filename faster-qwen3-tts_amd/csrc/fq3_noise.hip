// Seeded sampling noise behind the C ABI (noise_kernels.cuh holds the contract and the kernels):
//   fq3_noise_fill    rows of many lanes' noise rings, one launch per kNoiseMaxRings lanes
//   fq3_noise_first   the first-token row
//   fq3_noise_words   the raw Philox words of one row (conformance hook: the integer generator apart from the fp64 logarithm)
// Nothing here keeps state: a row is a pure function of (seed, frame, slot), so the calls may be cut and ordered in any way.
#include "fq3_ctx.h"
#include "noise_args.h"
#include "noise_kernels.cuh"

using namespace fq3;

#define NHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" int fq3_noise_fill(fq3_ctx* c, const fq3_noise_ring* rings, int n, int ring_frames, void* stream) {
    if (!c) return fq3_fail_(FQ3_EINVAL, "noise fill: NULL context");
    const int V = c->cfg.talker.vocab, G = c->cfg.num_code_groups, Vp = c->cfg.predictor.vocab;
    if (const char* why = fq3_noise_fill_check_(rings, n, ring_frames, c->cfg.dtype, V, G, Vp)) return fq3_fail_(FQ3_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    const int groups = (V + 7) / 8 + (G - 1) * ((Vp + 7) / 8);
    for (int base = 0; base < n; base += kNoiseMaxRings) {
        NoiseRings nr{};
        nr.ring_frames = ring_frames; nr.V = V; nr.G1 = G - 1; nr.Vp = Vp;
        const int m = n - base < kNoiseMaxRings ? n - base : kNoiseMaxRings;
        int rows = 0;
        for (int i = 0; i < m; ++i) {
            const fq3_noise_ring& r = rings[base + i];
            nr.talker[i] = r.talker; nr.pred[i] = r.pred;
            nr.key0[i] = (uint32_t)(r.seed & 0xffffffffull); nr.key1[i] = (uint32_t)(r.seed >> 32);
            nr.first_frame[i] = r.first_frame;
            nr.n_frames[i] = (r.talker || r.pred) ? r.n_frames : 0;
            rows = nr.n_frames[i] > rows ? nr.n_frames[i] : rows;
        }
        if (rows == 0) continue;
        const dim3 grid((groups + 255) / 256, rows, m);
        if (c->cfg.dtype == FQ3_BF16) hipLaunchKernelGGL((noise_fill_kernel<bf16_t>), grid, dim3(256), 0, s, nr);
        else hipLaunchKernelGGL((noise_fill_kernel<float>), grid, dim3(256), 0, s, nr);
        NHIP(hipGetLastError());
    }
    return FQ3_OK;
}

extern "C" int fq3_noise_first(fq3_ctx* c, uint64_t seed, void* out, void* stream) {
    if (!c || !out) return fq3_fail_(FQ3_EINVAL, "noise first: NULL argument");
    const int V = c->cfg.talker.vocab;
    if (V < 1 || (c->cfg.dtype != FQ3_BF16 && c->cfg.dtype != FQ3_F32)) return fq3_fail_(FQ3_EINVAL, "noise first: the context has no config");
    if ((uintptr_t)out & (c->cfg.dtype == FQ3_BF16 ? 1u : 3u)) return fq3_fail_(FQ3_EINVAL, "noise first: out is not aligned to its element type");
    const dim3 grid(((V + 7) / 8 + 255) / 256);
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
    if (c->cfg.dtype == FQ3_BF16) hipLaunchKernelGGL((noise_row_kernel<bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)out, V, 0u, kNoiseFirstSlot, k0, k1);
    else hipLaunchKernelGGL((noise_row_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (float*)out, V, 0u, kNoiseFirstSlot, k0, k1);
    NHIP(hipGetLastError());
    return FQ3_OK;
}

extern "C" int fq3_noise_words(uint64_t seed, uint32_t frame, uint32_t slot, int V, uint32_t* out, void* stream) {
    if (!out || V < 1) return fq3_fail_(FQ3_EINVAL, "noise words: out is NULL or V < 1");
    if ((uintptr_t)out & 3u) return fq3_fail_(FQ3_EINVAL, "noise words: out is not aligned to 4 bytes");
    const dim3 grid((unsigned)((((int64_t)V + 3) / 4 + 255) / 256));
    hipLaunchKernelGGL(noise_words_kernel, grid, dim3(256), 0, (hipStream_t)stream, out, (int64_t)V, frame, slot,
                       (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
    NHIP(hipGetLastError());
    return FQ3_OK;
}
