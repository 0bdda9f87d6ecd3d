// FLAC output stage (fq3_flac.hip): int16 PCM -> FLAC frames on the device.  Mono, 16 bits, fixed block size; CONSTANT, VERBATIM and
// FIXED (order 0..4) subframes with partitioned 4-bit Rice residuals; the choice per block is the exhaustive rule of DESIGN.md 4.10.
//
// flac_encode_kernel: ONE workgroup of five waves per block (blocks are independent).
//   (1) the block's n samples are staged in LDS, the LDS bit buffer is zeroed, thread 0 writes the frame header into it;
//   (2) the sample range is cut into 64 segments that refine the finest legal partition order pmax = min(6, ctz(n)); thread
//       (o = wave, g = lane) keeps the 15 sums  sum_i (u_o[i] >> k), k = 0..14, of segment g at predictor order o in registers (the
//       residual is recomputed from the staged samples; warm-up samples i < o are left out);
//   (3) partition orders 6 .. 0: thread (o, first segment of a partition) picks that partition's k and adds its bits to cost[o][p], then
//       neighbouring partitions are added in place (saturating: a sum past 2^31 belongs to a candidate above 16 n bits, which loses to
//       VERBATIM whatever its exact value);
//   (4) thread 0 takes the cheapest (o, p) -- lower o, then lower p on ties -- or VERBATIM when that costs 16 n bits or more;
//   (5) code lengths: every thread owns a run of consecutive residuals, a workgroup exclusive scan of the runs' bit counts gives each
//       run its bit offset, and each code ORs its stop bit and its k low bits into the zeroed LDS buffer (at most two words; LDS atomics);
//   (6) CRC-16: every thread takes a slice of the frame's bytes (slices are cut from the END, so that all but the earliest have the same
//       length), and the slices are combined in a tree by CRC linearity: crc(A | B) = crc(A) x^(8 |B|) + crc(B) mod P;
//   (7) the frame goes to the staging slot of its block, its length to sizes[block].
// flac_gather_kernel (a second launch: no workgroup ever waits for another): block f sums sizes[0 .. f) and copies frame f behind the
// frames before it; block 0 also publishes the running total.
//
// The workgroup with blockIdx == n_frames, when there is one, only copies the samples behind the last whole block into the object's
// other tail buffer.
//
// Both kernels are one __device__ body each (flac_encode_body, flac_gather_body) behind two __global__ shells: the single kernels, whose
// blockIdx is the frame, and flac_encode_group_kernel / flac_gather_group_kernel for the pushes of a group of objects of one design
// (fq3_flac_push_group, at the end of this file), whose workgroups find their (row, frame) in the launch's argument block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fq3 {

constexpr int kFlacThreads = 320;                   // five waves, one per predictor order
constexpr int kFlacSegs = 64;                       // segments per block = lanes of a wave = 2^(largest partition order)
constexpr int kFlacMaxK = 14;                       // Rice parameters 0 .. 14 (15 is the escape code, never emitted)
constexpr int kFlacMinBlock = 16, kFlacMaxBlock = 4608;
constexpr int kFlacBatch = 64;                      // frames per launch pair (= staging slots the object owns)
constexpr int kFlacGatherThreads = 256;
constexpr int kFlacBitWords = (2 * kFlacMaxBlock + 18 + 3) / 4 + 1;
constexpr uint32_t kFlacSat = 0x7FFFFFFFu;

struct FlacArgs {
    const int16_t* pcm;        // the new samples, n_in of them
    const int16_t* tail;       // the tail_n samples earlier pushes held back: logical indices [0, tail_n), pcm follows
    int16_t* tail_next;        // receives the tail_len samples from logical index tail_from on (the object's other tail buffer)
    uint8_t* stage;            // kFlacBatch slots of `stride` bytes
    int32_t* sizes;            // frame lengths of this launch
    int64_t first;             // logical index of the first sample of this launch's frame 0
    int64_t avail;             // tail_n + n_in
    int64_t tail_from;
    int tail_n, tail_len;
    int block, n_frames, stride;
    uint32_t frame0;           // frame number of this launch's frame 0
    int rate_code, rate_hz;    // the header's 4-bit code; 13: rate_hz follows in two bytes
};

__device__ __forceinline__ int flac_fetch(const FlacArgs& a, int64_t i) {
    return i < a.tail_n ? (int)a.tail[i] : (int)a.pcm[i - a.tail_n];
}

__device__ __forceinline__ void flac_put(uint32_t* bits, uint32_t pos, uint32_t val, int nbits) {      // 1 <= nbits <= 32, val < 2^nbits
    const uint32_t w = pos >> 5;
    const int end = (int)(pos & 31) + nbits;
    if (end <= 32) {
        atomicOr(&bits[w], val << (32 - end));
    } else {
        atomicOr(&bits[w], val >> (end - 32));
        atomicOr(&bits[w + 1], val << (64 - end));
    }
}

__device__ __forceinline__ int flac_residual(const int* x, int o, int i) {
    switch (o) {
        case 0: return x[i];
        case 1: return x[i] - x[i - 1];
        case 2: return x[i] - 2 * x[i - 1] + x[i - 2];
        case 3: return x[i] - 3 * x[i - 1] + 3 * x[i - 2] - x[i - 3];
        default: return x[i] - 4 * x[i - 1] + 6 * x[i - 2] - 4 * x[i - 3] + x[i - 4];
    }
}

__device__ __forceinline__ uint32_t flac_fold(int r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// a * b mod x^16 + x^15 + x^2 + 1 over GF(2)
__device__ __forceinline__ uint32_t flac_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r << 1) ^ ((r & 0x8000u) ? 0x18005u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r & 0xFFFFu;
}

__device__ __forceinline__ int flac_block_code(int n) {
    switch (n) {
        case 192: return 1;
        case 576: return 2;
        case 1152: return 3;
        case 2304: return 4;
        case 4608: return 5;
        case 256: return 8;
        case 512: return 9;
        case 1024: return 10;
        case 2048: return 11;
        case 4096: return 12;
        default: return n <= 256 ? 6 : 7;
    }
}

// frame f of the launch `a` describes; f == a.n_frames: the tail copy.  Uniform over the workgroup.
__device__ __forceinline__ void flac_encode_body(const FlacArgs& a, const int f) {
    __shared__ int s_x[kFlacMaxBlock];
    __shared__ uint32_t s_sum[5 * kFlacSegs * (kFlacMaxK + 1)];
    __shared__ uint32_t s_bits[kFlacBitWords];
    __shared__ uint32_t s_cost[5 * 7];
    __shared__ uint8_t s_bestk[5 * 7 * kFlacSegs];
    __shared__ uint32_t s_scan[kFlacThreads / 64];
    __shared__ uint32_t s_crc[512];
    __shared__ int s_hdr, s_order, s_porder, s_body;

    const int tid = threadIdx.x;
    if (f == a.n_frames) {
        for (int i = tid; i < a.tail_len; i += kFlacThreads) a.tail_next[i] = (int16_t)flac_fetch(a, a.tail_from + i);
        return;
    }
    const int64_t start = a.first + (int64_t)f * a.block;
    const int n = (int)(a.avail - start < a.block ? a.avail - start : a.block);      // >= 1: the host counted this frame

    // (1)
    for (int i = tid; i < n; i += kFlacThreads) s_x[i] = flac_fetch(a, start + i);
    for (int i = tid; i < (2 * n + 18 + 3) / 4 + 1; i += kFlacThreads) s_bits[i] = 0;
    if (tid < 5 * 7) s_cost[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        const int bc = flac_block_code(n);
        uint32_t pos = 0;
        uint32_t crc = 0;
        auto put = [&](uint32_t b) {
            flac_put(s_bits, pos, b, 8);
            pos += 8;
            crc ^= b;
            for (int j = 0; j < 8; ++j) crc = ((crc << 1) ^ ((crc & 0x80u) ? 0x07u : 0u)) & 0xFFu;
        };
        put(0xFF); put(0xF8); put((uint32_t)(bc << 4 | a.rate_code)); put(0x08);
        const uint32_t v = a.frame0 + (uint32_t)f;                                  // below 2^31 (the host refuses more frames)
        if (v < 0x80u) {
            put(v);
        } else {
            int nb = 2;
            while (nb < 6 && v >= (1u << (5 * nb + 1))) ++nb;
            put(((0xFF00u >> nb) & 0xFFu) | (v >> (6 * (nb - 1))));
            for (int j = nb - 2; j >= 0; --j) put(0x80u | ((v >> (6 * j)) & 0x3Fu));
        }
        if (bc == 6) put((uint32_t)(n - 1));
        if (bc == 7) { put((uint32_t)(n - 1) >> 8); put((uint32_t)(n - 1) & 0xFFu); }
        if (a.rate_code == 13) { put((uint32_t)a.rate_hz >> 8); put((uint32_t)a.rate_hz & 0xFFu); }
        const uint32_t c8 = crc;
        put(c8);
        s_hdr = (int)(pos >> 3);
    }
    int differs = 0;
    for (int i = tid; i < n; i += kFlacThreads) differs |= s_x[i] != s_x[0];
    const int varied = __syncthreads_or(differs);
    const int hdr = s_hdr;

    if (!varied) {
        if (tid == 0) {
            flac_put(s_bits, (uint32_t)hdr * 8 + 8, (uint32_t)s_x[0] & 0xFFFFu, 16);      // subframe byte 0x00 (CONSTANT) is already there
            s_body = hdr + 3;
        }
    } else {
        // (2)
        const int o = tid >> 6, g = tid & 63;
        const int omax = n - 1 < 4 ? n - 1 : 4;
        int pmax = __builtin_ctz((unsigned)n);
        pmax = pmax > 6 ? 6 : pmax;
        {
            const int size = n >> pmax, sub = kFlacSegs >> pmax, per = (size + sub - 1) / sub;
            const int q = g >> (6 - pmax), j = g & (sub - 1);
            int lo = q * size + (j * per < size ? j * per : size);
            const int hi = q * size + ((j + 1) * per < size ? (j + 1) * per : size);
            lo = lo < o ? o : lo;
            uint32_t acc[kFlacMaxK + 1];
#pragma unroll
            for (int k = 0; k <= kFlacMaxK; ++k) acc[k] = 0;
            if (o <= omax) {
                for (int i = lo; i < hi; ++i) {
                    const uint32_t u = flac_fold(flac_residual(s_x, o, i));
#pragma unroll
                    for (int k = 0; k <= kFlacMaxK; ++k) acc[k] += u >> k;           // a segment has at most 72 samples of u < 2^21
                }
            }
#pragma unroll
            for (int k = 0; k <= kFlacMaxK; ++k) s_sum[tid * (kFlacMaxK + 1) + k] = acc[k];
        }
        __syncthreads();
        // (3)
        for (int p = 6; p >= 0; --p) {
            const int span = kFlacSegs >> p;
            if (p <= pmax && o <= omax && (n >> p) > o && (g & (span - 1)) == 0) {
                const int q = g / span;
                const uint32_t cnt = (uint32_t)((n >> p) - (q == 0 ? o : 0));
                uint32_t best = 0xFFFFFFFFu;
                int bk = 0;
                for (int k = 0; k <= kFlacMaxK; ++k) {
                    const uint32_t bits = cnt * (uint32_t)(1 + k) + s_sum[tid * (kFlacMaxK + 1) + k];
                    if (bits < best) { best = bits; bk = k; }
                }
                s_bestk[(o * 7 + p) * kFlacSegs + q] = (uint8_t)bk;
                atomicAdd(&s_cost[o * 7 + p], 4u + (best < (1u << 24) ? best : (1u << 24)));
            }
            __syncthreads();
            if (p > 0 && (g & (2 * span - 1)) == 0) {
                for (int k = 0; k <= kFlacMaxK; ++k) {
                    const uint32_t s2 = s_sum[tid * (kFlacMaxK + 1) + k] + s_sum[(tid + span) * (kFlacMaxK + 1) + k];
                    s_sum[tid * (kFlacMaxK + 1) + k] = s2 < kFlacSat ? s2 : kFlacSat;
                }
            }
            __syncthreads();
        }
        // (4)
        if (tid == 0) {
            uint32_t best = 0xFFFFFFFFu;
            int bo = 0, bp = 0;
            for (int oo = 0; oo <= omax; ++oo)
                for (int p = 0; p <= pmax; ++p)
                    if ((n >> p) > oo) {
                        const uint32_t c = 16u * oo + 6u + s_cost[oo * 7 + p];
                        if (c < best) { best = c; bo = oo; bp = p; }
                    }
            const bool verbatim = best >= 16u * (uint32_t)n;
            s_order = verbatim ? -1 : bo;
            s_porder = bp;
            uint32_t pos = (uint32_t)hdr * 8;
            if (verbatim) {
                flac_put(s_bits, pos, 0x02u, 8);
            } else {
                flac_put(s_bits, pos, (uint32_t)((8 | bo) << 1), 8);
                pos += 8;
                for (int i = 0; i < bo; ++i, pos += 16) flac_put(s_bits, pos, (uint32_t)s_x[i] & 0xFFFFu, 16);
                flac_put(s_bits, pos, (uint32_t)bp, 6);                               // method 00, then the partition order
            }
        }
        __syncthreads();
        const int order = s_order, porder = s_porder;
        if (order < 0) {
            for (int i = tid; i < n; i += kFlacThreads) flac_put(s_bits, (uint32_t)(hdr + 1 + 2 * i) * 8, (uint32_t)s_x[i] & 0xFFFFu, 16);
            if (tid == 0) s_body = hdr + 1 + 2 * n;
        } else {
            // (5)
            const int size = n >> porder;
            const uint8_t* ks = &s_bestk[(order * 7 + porder) * kFlacSegs];
            const int per = (n - order + kFlacThreads - 1) / kFlacThreads;
            const int c0 = order + tid * per < n ? order + tid * per : n;
            const int c1 = c0 + per < n ? c0 + per : n;
            uint32_t local = 0;
            for (int i = c0; i < c1; ++i) {
                const int q = i / size, k = ks[q];
                if (i == order || i == q * size) local += 4;
                local += (flac_fold(flac_residual(s_x, order, i)) >> k) + 1u + (uint32_t)k;
            }
            uint32_t incl = local;                                                   // inclusive scan inside the wave
            const int lane = tid & 63, wave = tid >> 6;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            if (lane == 63) s_scan[wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (int w = 0; w < kFlacThreads / 64; ++w) {
                const uint32_t t = s_scan[w];
                before += w < wave ? t : 0u;
                total += t;
            }
            const uint32_t base = (uint32_t)(hdr + 1 + 2 * order) * 8 + 6;
            uint32_t pos = base + before + incl - local;
            for (int i = c0; i < c1; ++i) {
                const int q = i / size, k = ks[q];
                if (i == order || i == q * size) { flac_put(s_bits, pos, (uint32_t)k, 4); pos += 4; }
                const uint32_t u = flac_fold(flac_residual(s_x, order, i));
                pos += u >> k;                                                       // the zero bits are there already
                flac_put(s_bits, pos, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
                pos += (uint32_t)k + 1u;
            }
            if (tid == 0) s_body = (int)((base + total + 7) >> 3);
        }
    }
    __syncthreads();
    // (6)
    const int len = s_body;
    {
        const int lb = (len + kFlacThreads - 1) / kFlacThreads;
        const int e = len - tid * lb, b = e - lb < 0 ? 0 : e - lb;
        uint32_t c = 0;
        for (int i = b; i < e; ++i) {
            c ^= ((s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu) << 8;
            for (int j = 0; j < 8; ++j) c = (c << 1) ^ ((c & 0x8000u) ? 0x18005u : 0u);
        }
        s_crc[tid] = c & 0xFFFFu;
        if (tid + kFlacThreads < 512) s_crc[tid + kFlacThreads] = 0;
        uint32_t m = 1;                                                              // x^(8 lb) mod P
        for (int i = 0; i < 8 * lb; ++i) m = (m << 1) ^ ((m & 0x8000u) ? 0x18005u : 0u);
        m &= 0xFFFFu;
        __syncthreads();
        for (int h = 1; h < 512; h <<= 1) {
            uint32_t v = 0;
            const bool mine = (tid & (2 * h - 1)) == 0 && tid + h < 512;
            if (mine) v = flac_mulmod(s_crc[tid + h], m) ^ s_crc[tid];               // slice tid + h holds the EARLIER bytes
            __syncthreads();
            if (mine) s_crc[tid] = v;
            __syncthreads();
            m = flac_mulmod(m, m);
        }
        if (tid == 0) flac_put(s_bits, (uint32_t)len * 8, s_crc[0], 16);
    }
    __syncthreads();
    // (7) the staging slot is 4-byte aligned and a multiple of four bytes long; the bytes behind the frame in its last word are zeros
    const int flen = len + 2;
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.stage + (size_t)f * a.stride);
    for (int w = tid; w < (flen + 3) / 4; w += kFlacThreads) dst[w] = __builtin_bswap32(s_bits[w]);
    if (tid == 0) a.sizes[f] = flen;
}

__global__ __launch_bounds__(kFlacThreads) void flac_encode_kernel(FlacArgs a) { flac_encode_body(a, (int)blockIdx.x); }

// Frames of one launch pair, back to back: out[base + sum sizes[0 .. f)) <- stage slot f.  base = *base_in (null: 0), the bytes the
// earlier launch pairs of the same push wrote; block 0 writes base + sum of all sizes to *total_out (the other of the object's two
// counters, so that no block reads what another one writes) and to *n_bytes.
struct FlacGatherArgs {
    const uint8_t* stage;
    const int32_t* sizes;
    const int64_t* base_in;
    int64_t* total_out;
    int64_t* n_bytes;
    uint8_t* out;
    int n_frames, stride;
};

__device__ __forceinline__ void flac_gather_body(const FlacGatherArgs& a, const int f) {
    __shared__ int64_t s_off;
    const int tid = threadIdx.x;
    if (tid < 64) {
        const int v = tid < a.n_frames ? a.sizes[tid] : 0;
        int pre = tid < f ? v : 0, tot = v;
        for (int d = 32; d >= 1; d >>= 1) {
            pre += __shfl_xor(pre, d);
            tot += __shfl_xor(tot, d);
        }
        if (tid == 0) {
            const int64_t base = a.base_in ? *a.base_in : 0;
            s_off = base + pre;
            if (f == 0) { *a.total_out = base + tot; *a.n_bytes = base + tot; }
        }
    }
    __syncthreads();
    const int len = a.sizes[f];
    const uint8_t* src = a.stage + (size_t)f * a.stride;
    uint8_t* dst = a.out + s_off;
    for (int i = tid; i < len; i += kFlacGatherThreads) dst[i] = src[i];
}

__global__ __launch_bounds__(kFlacGatherThreads) void flac_gather_kernel(const uint8_t* stage, const int32_t* sizes, int n_frames, int stride,
                                                                         const int64_t* base_in, int64_t* total_out, int64_t* n_bytes,
                                                                         uint8_t* out) {
    FlacGatherArgs a;
    a.stage = stage; a.sizes = sizes; a.base_in = base_in; a.total_out = total_out; a.n_bytes = n_bytes; a.out = out;
    a.n_frames = n_frames; a.stride = stride;
    flac_gather_body(a, (int)blockIdx.x);
}

// ---- a group of pushes in one launch pair (fq3_flac_push_group) ----
// The rows share one design (block size and rate) and differ in everything a push derives from its object's state.  A row of a launch
// has between 0 and kFlacBatch + 1 workgroups -- its frames of this round, then its tail copy (encode) or, for a push that completes no
// frame at all, the one that writes its byte count of 0 (gather) -- so the grid is one-dimensional and PACKED: wg0[b] is the first
// workgroup of row b, wg0[b + 1] - wg0[b] its count, and rows past the group's last hold the grid size.  A workgroup counts the rows
// that start at or before it; blockIdx is uniform and the table lies in the argument segment, so this is 31 scalar compares on two
// wide scalar loads, and the row's descriptor is read by scalar loads at a scalar offset.  The descriptors travel BY VALUE, as in
// audio_kernels.cuh: no table in device memory has to be filled (and kept alive) per call.
// LDS: the encode body's 51 KB of static LDS admit three workgroups per CU; the group launch brings the frames of all rows to the CUs
// at once (13 frames a row of a typical chunk: some 420 workgroups for 32 rows) where a row's own launch fills 13 CUs.
constexpr int kFlacGroupMax = 32;                   // FQ3_STAGE_GROUP_MAX

struct FlacGroupRow {
    const int16_t* pcm;
    const int16_t* tail;
    int16_t* tail_next;
    uint8_t* stage;
    int32_t* sizes;
    int64_t* totals;           // the object's two running byte counts
    int64_t* n_bytes;
    uint8_t* out;
    int64_t avail, tail_from;
    int tail_n, tail_len;      // tail_len > 0 in the row's last round only
    int n_frames;              // of this round
    uint32_t frame0;           // frame number of this round's frame 0
};

struct FlacGroupArgs {
    int64_t first;             // logical index of the first sample of this round's frame 0: round * kFlacBatch * block
    int block, stride, rate_code, rate_hz;
    int round, pad_;
    int enc_wg0[kFlacGroupMax], gat_wg0[kFlacGroupMax];
    FlacGroupRow rows[kFlacGroupMax];
};
// hipModuleLaunchKernel / hipLaunchKernelGGL carry at most 4 KB of kernel arguments
static_assert(sizeof(FlacGroupRow) == 96 && sizeof(FlacGroupArgs) <= 4096, "the descriptors must fit the 4 KB of arguments a launch may carry");

__device__ __forceinline__ int flac_group_row(const int* wg0, const int wg) {
    int row = 0;
#pragma unroll
    for (int b = 1; b < kFlacGroupMax; ++b) row += wg >= wg0[b] ? 1 : 0;          // wg0 does not decrease: the last row that starts at or before wg
    return row;
}

__global__ __launch_bounds__(kFlacThreads) void flac_encode_group_kernel(const FlacGroupArgs g) {
    const int wg = (int)blockIdx.x, row = flac_group_row(g.enc_wg0, wg);
    const FlacGroupRow& r = g.rows[row];
    FlacArgs a;
    a.pcm = r.pcm; a.tail = r.tail; a.tail_next = r.tail_next; a.stage = r.stage; a.sizes = r.sizes;
    a.first = g.first; a.avail = r.avail; a.tail_from = r.tail_from; a.tail_n = r.tail_n; a.tail_len = r.tail_len;
    a.block = g.block; a.n_frames = r.n_frames; a.stride = g.stride; a.frame0 = r.frame0;
    a.rate_code = g.rate_code; a.rate_hz = g.rate_hz;
    flac_encode_body(a, wg - g.enc_wg0[row]);
}

__global__ __launch_bounds__(kFlacGatherThreads) void flac_gather_group_kernel(const FlacGroupArgs g) {
    const int wg = (int)blockIdx.x, row = flac_group_row(g.gat_wg0, wg);
    const FlacGroupRow& r = g.rows[row];
    if (r.n_frames == 0) {                                                          // a push that completes no frame: its one workgroup
        if (threadIdx.x == 0) *r.n_bytes = 0;
        return;
    }
    FlacGatherArgs a;
    a.stage = r.stage; a.sizes = r.sizes;
    a.base_in = g.round ? r.totals + ((g.round - 1) & 1) : nullptr;
    a.total_out = r.totals + (g.round & 1);
    a.n_bytes = r.n_bytes; a.out = r.out; a.n_frames = r.n_frames; a.stride = g.stride;
    flac_gather_body(a, wg - g.gat_wg0[row]);
}

}  // namespace fq3
