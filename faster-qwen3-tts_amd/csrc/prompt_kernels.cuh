// Kernels of the prompt builder and of the open text table (launched by fq3_prompt.hip; tools/microbench/state_probe.hip launches each
// of them alone for tests/test_gpu_state_reference.py).  Rounding points are those of the module-by-module Torch execution: one
// rounding to T after the 16-way embedding sum, one after text + codec.
#pragma once
#include "decode_kernels.cuh"

namespace fq3 {

// out[r] = table[clamp(ids[r], 0, vocab - 1)]: one workgroup per row, Ht a multiple of 8
template <typename T>
__global__ __launch_bounds__(256) void text_gather_kernel(const int64_t* ids, const T* table, T* out, int n, int Ht, int vocab) {
    const int r = blockIdx.x;
    int64_t id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);            // F.embedding would fault; clamp keeps the launch safe
    const T* src = table + (size_t)id * Ht;
    for (int e = threadIdx.x * 8; e < Ht; e += 256 * 8) {
        Raw8<T> v; ldraw<false>(v, src + e);
        float f[8]; unpack(v, f);
        DT<T>::st8(out + (size_t)r * Ht + e, f);
    }
}

struct RowTables { const void* t[16]; };

// one workgroup per prompt row; prog[r] = (trow, kind, arg).  The row is text_rows[trow] where 0 <= trow < n_text, plus a codec row by
// kind: 1 = row clamp(arg) of table 0; 2 = spk; 3 = the 16-way sum of the tables' rows of frame clamp(arg) of ref_codes (ids clamped
// per table), rounded once; any other kind: none.  Both present: rnd(text + codec); neither: zeros.  prog lives in device memory, so
// the host cannot refuse a row that names an operand the call does not have: kind 3 with n_ref <= 0 and kind 2 with a null spk read
// nothing and count as an unknown kind (text only, or zeros).
template <typename T>
__global__ __launch_bounds__(256) void prompt_rows_kernel(const T* text_rows, int n_text, const int* prog, const int64_t* ref_codes,
                                                          int n_ref, const T* spk, RowTables tabs, int vocab0, int vocab_rest,
                                                          T* out, int H) {
    const int r = blockIdx.x;
    const int trow = prog[r * 3 + 0], kind = prog[r * 3 + 1], arg = prog[r * 3 + 2];
    const bool has_text = trow >= 0 && trow < n_text;
    for (int e = threadIdx.x * 8; e < H; e += 256 * 8) {
        float c[8], t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { c[i] = 0.f; t[i] = 0.f; }
        bool has_codec = true;
        if (kind == 1) {
            const int id = arg < 0 ? 0 : (arg >= vocab0 ? vocab0 - 1 : arg);
            Raw8<T> v; ldraw<false>(v, reinterpret_cast<const T*>(tabs.t[0]) + (size_t)id * H + e);
            unpack(v, c);
        } else if (kind == 2 && spk) {
            Raw8<T> v; ldraw<false>(v, spk + e);
            unpack(v, c);
        } else if (kind == 3 && n_ref > 0) {
            const int fr = arg < 0 ? 0 : (arg >= n_ref ? n_ref - 1 : arg);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int vmax = g == 0 ? vocab0 : vocab_rest;
                int64_t id = ref_codes[(size_t)fr * 16 + g];
                id = id < 0 ? 0 : (id >= vmax ? vmax - 1 : id);
                Raw8<T> v; ldraw<false>(v, reinterpret_cast<const T*>(tabs.t[g]) + (size_t)id * H + e);
                float f[8]; unpack(v, f);
#pragma unroll
                for (int i = 0; i < 8; ++i) c[i] += f[i];
            }
#pragma unroll
            for (int i = 0; i < 8; i += 2) DT<T>::rnd2(c[i], c[i + 1]);          // torch: cat(...).sum(1), one rounding
        } else has_codec = false;
        if (has_text) {
            Raw8<T> v; ldraw<false>(v, text_rows + (size_t)trow * H + e);
            unpack(v, t);
        }
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (has_text && has_codec) ? t[i] + c[i] : (has_text ? t[i] : c[i]);
        DT<T>::st8(out + (size_t)r * H + e, o);
    }
}

// ---- open text table of the decode loop ----------------------------------------------------------------------------------------
// The loop state lives in device memory and every replay of the frame graph reads it afresh, so the table may grow between replays:
// the rows are written first, then ONE thread publishes the new length on the same stream.  Frames queued before see the old length,
// frames queued after the new one; stream order is the only synchronisation.
// text_open: the `words` 32-bit words of the rows fq3_decode_begin was given are copied into the table, then trailing_text = the
// table's address and text_open = 1; nothing else of the state changes.
static __global__ __launch_bounds__(256) void text_open_kernel(DecodeState* st, uint32_t* table, const uint32_t* rows, int words) {
    for (int i = threadIdx.x; i < words; i += 256) table[i] = rows[i];
    __syncthreads();
    if (threadIdx.x == 0) { st->trailing_text = table; st->text_open = 1; }
}
// text_publish: trailing_len = rows; text_open = 0 only when final
static __global__ void text_publish_kernel(DecodeState* st, int rows, int final) {
    st->trailing_len = rows;
    if (final) st->text_open = 0;
}

}  // namespace fq3
