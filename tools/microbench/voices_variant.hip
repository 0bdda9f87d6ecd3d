// Measurement tool (tools/voices_probe.py loads it with ctypes): the voice library search built from csrc/voices_kernels.cuh with the
// scan variant chosen by the caller -- row blocks per wave RB in {1, 2, 4} and the queries from L2 (what libfq3hip ships) or staged in
// LDS (QLDS, measured slower: DESIGN.md section 4.27).  Not part of the library.
#include "../../faster-qwen3-tts_amd/csrc/voices_kernels.cuh"

using namespace fq3;

#define VHIP(x) do { if ((x) != hipSuccess) { rc = -2; goto done; } } while (0)

template <int RB, bool QLDS>
static bool scan(const float* lib, const float* qp, const uint8_t* live, unsigned long long* part, long n, int kq_n, int rows, int k, long slabs) {
    const size_t shm = (size_t)((kVoiceQueries * (kVoiceWaves * RB * 16 + 1) + 3) & ~3) * sizeof(float) + (QLDS ? 2 * kVoiceChunk * 64 * sizeof(float4) : 0);
    if (!lds_limit_at_least<voices_scan_kernel<RB, QLDS>>(shm)) return false;
    hipLaunchKernelGGL((voices_scan_kernel<RB, QLDS>), dim3((unsigned)slabs), dim3(kVoiceWaves * 64), shm, 0, lib, qp, live, part, n, kq_n, rows > 16 ? 2 : 1, rows, k);
    return true;
}

// raw: device float32[n][dim]; q: device float32[rows][dim]; idx / cos: device [rows][k].  Builds its own library, runs 2 warm-up
// searches, then `samples` timed windows of `calls` searches each (pack, scan, merge); ms[s] = window s in milliseconds per call.
// Returns 0, -1 for an argument out of range, -2 for a HIP error.
extern "C" int voices_variant_time(const float* raw, long n, int dim, const float* q, int rows, int k, int rb, int qlds, int samples, int calls,
                                   int32_t* idx, float* cos, float* ms) {
    if (!raw || !q || !idx || !cos || !ms || n < 1 || n > (1L << 22) || dim < 16 || dim % 16 || rows < 1 || rows > kVoiceQueries || k < 1 ||
        k > kVoiceMaxK || (rb != 1 && rb != 2 && rb != 4) || samples < 1 || calls < 1)
        return -1;
    const long padded = (n + 15) / 16 * 16, slabs = (n + 128 * rb - 1) / (128 * rb);
    float *lib = nullptr, *qp = nullptr;
    uint8_t* live = nullptr;
    unsigned long long* part = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    int rc = 0;
    VHIP(hipMalloc((void**)&lib, (size_t)padded * dim * sizeof(float)));
    VHIP(hipMalloc((void**)&live, (size_t)padded));
    VHIP(hipMalloc((void**)&qp, (size_t)kVoiceQueries * dim * sizeof(float)));
    VHIP(hipMalloc((void**)&part, (size_t)slabs * kVoiceQueries * k * sizeof(unsigned long long)));
    VHIP(hipEventCreate(&a));
    VHIP(hipEventCreate(&b));
    hipLaunchKernelGGL(voices_add_kernel, dim3((unsigned)((padded + 3) / 4)), dim3(256), 0, 0, raw, lib, live, 0L, n, dim);
    for (int s = -2; s < samples; ++s) {
        VHIP(hipEventRecord(a, 0));
        for (int c = 0; c < calls; ++c) {
            hipLaunchKernelGGL(voices_query_pack_kernel, dim3(kVoiceQueries / 4), dim3(256), 0, 0, q, qp, rows, dim);
            const bool ok = qlds ? (rb == 1 ? scan<1, true>(lib, qp, live, part, n, dim / 16, rows, k, slabs) : rb == 2 ? scan<2, true>(lib, qp, live, part, n, dim / 16, rows, k, slabs)
                                                                                                                         : scan<4, true>(lib, qp, live, part, n, dim / 16, rows, k, slabs))
                                 : (rb == 1 ? scan<1, false>(lib, qp, live, part, n, dim / 16, rows, k, slabs) : rb == 2 ? scan<2, false>(lib, qp, live, part, n, dim / 16, rows, k, slabs)
                                                                                                                          : scan<4, false>(lib, qp, live, part, n, dim / 16, rows, k, slabs));
            if (!ok) { rc = -2; goto done; }
            hipLaunchKernelGGL(voices_merge_kernel, dim3(rows), dim3(kVoiceMergeThreads), (size_t)((slabs + 15) & ~15L), 0, part, (int)slabs, k, idx, cos);
        }
        VHIP(hipEventRecord(b, 0));
        VHIP(hipEventSynchronize(b));
        VHIP(hipGetLastError());
        if (s >= 0) {
            float t = 0.f;
            VHIP(hipEventElapsedTime(&t, a, b));
            ms[s] = t / calls;
        }
    }
done:
    (void)hipDeviceSynchronize();
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    (void)hipFree(lib); (void)hipFree(live); (void)hipFree(qp); (void)hipFree(part);
    return rc;
}
