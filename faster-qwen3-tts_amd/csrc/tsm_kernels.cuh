// Time-scale modification (fq3_tsm.hip): WSOLA on the device, one launch per push, ONE workgroup per launch.
//
// Output segment s (Hs samples) overlap-adds two windows of the input: the continuation of the previous segment's window
// (x[pos(s-1) + Hs + j], the "template") and a window at pos(s) = a(s) + delta(s), where delta(s) in [-D, D] maximises the plain
// cross-correlation of the N = 2 Hs samples at a(s) + delta with the template.  delta(s) needs pos(s-1), so the segments form a chain:
// the workgroup walks the push's segments in order and keeps the chain's state in registers; between pushes delta of the last
// segment waits in device memory (the host never learns it).
//
// Per segment: (1) the 2 D + N candidate samples and the N template samples are staged in LDS; (2) thread (q, g), q = tid / 128,
// accumulates eighth q (j in [q N / 8, (q + 1) N / 8), ascending, fmaf from 0.0f) of the FOUR candidates 4 g .. 4 g + 3: per four
// steps of j one new aligned 16-byte read of the samples (neighbouring lanes read neighbouring 16-byte slots; the window slides through
// registers) and one 16-byte broadcast of the template feed 16 fmaf; c(delta) = the eight partial sums added in ascending q -- a
// fixed function of (delta, j), the same for every segment, launch and cut; (3) argmax over (value, -delta): wave butterfly, then the
// waves' winners through LDS, so that ties go to the smallest delta; (4) the same workgroup writes the segment's Hs outputs from the
// staged samples.
//
// All input indices are RELATIVE to the first sample of the new chunk, as in audio_kernels.cuh: [-HL, 0) is the history (the last
// hist_valid of it real, anything older lies before the stream and is zero), [0, n_in) the chunk, [n_in, ..) the zeros after the end
// of a finished stream.  The absolute positions (which pass 2^31 in a long stream) stay on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fq3 {

constexpr int kTsmThreads = 1024;
constexpr int kTsmSlices = 8;                       // parts of the j range
constexpr int kTsmLanes = kTsmThreads / kTsmSlices; // threads per part, four candidates each; more candidates take another round

struct TsmArgs {
    const float* pcm;          // the new chunk, n_in floats
    const float* hist;         // history as of before this push: relative indices [-HL, 0) at hist[0 .. HL)
    float* hist_next;          // receives the history as of after this push (the other of the object's two buffers)
    const float* window;       // periodic Hann, N = 2 Hs floats
    float* out;                // n_out floats
    int* delta_out;            // optional: delta(s) of every segment of this push
    int* state;                // state[0]: delta of the last segment emitted so far
    int64_t n_in, n_out;
    int64_t n_seg;             // segments of this push: ceil(n_out / Hs) (only the last one of a finished stream is partial)
    int64_t a0;                // a(s0) of the push's first segment s0, relative
    int64_t prev_a;            // a(s0 - 1), relative; s0 = 0: pos(-1) = -Hs
    int64_t step;              // Hs P: a(s0 + i) = a0 + floor((r0 + i step) / 1000)
    int r0;                    // (s0 Hs P) mod 1000
    int Hs, HL, hist_valid;
    int first_is_zero;         // s0 = 0: segment 0 has delta = 0, no search, and no state to read
};

__device__ __forceinline__ float tsm_fetch(const TsmArgs& a, int64_t c) {
    if (c >= 0) return c < a.n_in ? a.pcm[c] : 0.0f;
    return c >= -(int64_t)a.hist_valid ? a.hist[a.HL + c] : 0.0f;
}

// (v2, i2) before (v1, i1): the larger value, among equal values the smaller index
__device__ __forceinline__ bool tsm_better(float v2, int i2, float v1, int i1) { return v2 > v1 || (v2 == v1 && i2 < i1); }

// LDS (floats): [4 Hs + 4 candidate samples][2 Hs template][2 Hs window][8 x (2 Hs + 4) partial sums][16 wave values][16 wave indices]
__host__ __device__ inline int tsm_lds_floats(int Hs) { return 24 * Hs + 4 + 8 * 4 + 32; }

// One workgroup, one push: the single kernel and the group kernel (one push per workgroup) both run this body.
__device__ __forceinline__ void tsm_body(const TsmArgs& a) {
    extern __shared__ float tsm_lds[];
    const int Hs = a.Hs, N = 2 * Hs, D = Hs, n_cand = 2 * D + 1;
    const int n_grp = (n_cand + 3) / 4, p_stride = 4 * n_grp, J = N / kTsmSlices;      // Hs is a multiple of 16: J of 4
    float* xs = tsm_lds;                     // x[a(s) - D + k], k in [0, N + 2 D); four floats of padding (the last group's reads)
    float* ts = xs + 4 * Hs + 4;             // x[pos(s-1) + Hs + k], k in [0, N)
    float* ws = ts + 2 * Hs;
    float* part = ws + 2 * Hs;               // part[q p_stride + c]
    float* wv = part + kTsmSlices * p_stride;
    int* wi = reinterpret_cast<int*>(wv + kTsmThreads / 64);
    const int tid = threadIdx.x, q = tid / kTsmLanes, t = tid % kTsmLanes;

    // the history of the NEXT push: the last HL samples of (history ++ chunk), into the other buffer
    if (a.n_in > 0)
        for (int j = tid; j < a.HL; j += kTsmThreads) a.hist_next[j] = tsm_fetch(a, a.n_in - a.HL + j);
    for (int j = tid; j < N; j += kTsmThreads) ws[j] = a.window[j];
    if (tid < 4) xs[N + 2 * D + tid] = 0.0f;

    int64_t prev_pos = a.prev_a + (a.first_is_zero ? 0 : a.state[0]);
    int delta = 0;
    for (int64_t i = 0; i < a.n_seg; ++i) {
        const int64_t a_i = a.a0 + ((int64_t)a.r0 + i * a.step) / 1000;
        const int64_t t_pos = prev_pos + Hs;
        __syncthreads();                     // the previous segment's reads of xs / ts / wv are done
        for (int k = tid; k < N + 2 * D; k += kTsmThreads) xs[k] = tsm_fetch(a, a_i - D + k);
        for (int k = tid; k < N; k += kTsmThreads) ts[k] = tsm_fetch(a, t_pos + k);
        __syncthreads();
        int best = D;                        // segment 0: delta = 0
        if (!(a.first_is_zero && i == 0)) {
            const float* tp = ts + q * J;
            for (int g = t; g < n_grp; g += kTsmLanes) {
                const float* xp = xs + 4 * g + q * J;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                float4 lo = *reinterpret_cast<const float4*>(xp);
                for (int j = 0; j < J; j += 4) {
                    const float4 hi = *reinterpret_cast<const float4*>(xp + j + 4);
                    const float4 tv = *reinterpret_cast<const float4*>(tp + j);
                    a0 = fmaf(lo.x, tv.x, a0); a0 = fmaf(lo.y, tv.y, a0); a0 = fmaf(lo.z, tv.z, a0); a0 = fmaf(lo.w, tv.w, a0);
                    a1 = fmaf(lo.y, tv.x, a1); a1 = fmaf(lo.z, tv.y, a1); a1 = fmaf(lo.w, tv.z, a1); a1 = fmaf(hi.x, tv.w, a1);
                    a2 = fmaf(lo.z, tv.x, a2); a2 = fmaf(lo.w, tv.y, a2); a2 = fmaf(hi.x, tv.z, a2); a2 = fmaf(hi.y, tv.w, a2);
                    a3 = fmaf(lo.w, tv.x, a3); a3 = fmaf(hi.x, tv.y, a3); a3 = fmaf(hi.y, tv.z, a3); a3 = fmaf(hi.z, tv.w, a3);
                    lo = hi;
                }
                *reinterpret_cast<float4*>(part + q * p_stride + 4 * g) = make_float4(a0, a1, a2, a3);
            }
            __syncthreads();
            float bv = -INFINITY;
            int bi = 0x7FFFFFFF;
            for (int c = tid; c < n_cand; c += kTsmThreads) {
                float v = part[c];
#pragma unroll
                for (int p = 1; p < kTsmSlices; ++p) v += part[p * p_stride + c];
                if (!(v == v)) v = -INFINITY;              // a NaN never wins
                if (tsm_better(v, c, bv, bi)) { bv = v; bi = c; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if (tsm_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
            __syncthreads();
            bv = wv[0]; bi = wi[0];
#pragma unroll
            for (int w = 1; w < kTsmThreads / 64; ++w)
                if (tsm_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
            best = bi < n_cand ? bi : n_cand - 1;          // whatever the values were: an index inside the staged samples
        }
        delta = best - D;
        const int64_t left = a.n_out - i * Hs;             // the last segment of a finished stream may be partial
        for (int j = tid; j < Hs && j < left; j += kTsmThreads)
            a.out[i * Hs + j] = fmaf(ws[j], xs[best + j], __fmul_rn(ws[j + Hs], ts[j]));
        if (tid == 0 && a.delta_out) a.delta_out[i] = delta;
        prev_pos = a_i + delta;
    }
    if (tid == 0 && a.n_seg > 0) a.state[0] = delta;
}

__global__ void __launch_bounds__(kTsmThreads) tsm_kernel(const TsmArgs a) { tsm_body(a); }

// ---- a group of pushes in one launch (fq3_tsm_push_group) ----
// Grid B, one workgroup per row: each row's segment chain is serial, the rows' chains run side by side.  The rows share the hop (one
// in_rate, so one window and one LDS layout); the speed enters only the host-computed fields (a0, prev_a, step, r0, HL) and may differ
// per row.  The descriptors travel BY VALUE in the kernel's argument block, as in audio_kernels.cuh: blockIdx.x is uniform, so a row's
// fields are scalar loads from the argument segment.  A row with nothing to do (n_in = 0, n_seg = 0) stages the window and leaves.
constexpr int kTsmGroupMax = 32;                // FQ3_STAGE_GROUP_MAX

struct TsmRow {
    const float* pcm;
    const float* hist;
    float* hist_next;
    float* out;
    int* state;
    int64_t n_in, n_out, n_seg, a0, prev_a, step;
    int r0, HL, hist_valid, first_is_zero;
};

struct TsmGroupArgs {
    const float* window;
    int Hs;
    TsmRow rows[kTsmGroupMax];
};
static_assert(sizeof(TsmRow) == 104 && sizeof(TsmGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

__global__ void __launch_bounds__(kTsmThreads) tsm_group_kernel(const TsmGroupArgs g) {
    const TsmRow& r = g.rows[blockIdx.x];
    TsmArgs a;
    a.pcm = r.pcm; a.hist = r.hist; a.hist_next = r.hist_next; a.window = g.window; a.out = r.out;
    a.delta_out = nullptr; a.state = r.state;
    a.n_in = r.n_in; a.n_out = r.n_out; a.n_seg = r.n_seg; a.a0 = r.a0; a.prev_a = r.prev_a; a.step = r.step;
    a.r0 = r.r0; a.Hs = g.Hs; a.HL = r.HL; a.hist_valid = r.hist_valid; a.first_is_zero = r.first_is_zero;
    tsm_body(a);
}

}  // namespace fq3
