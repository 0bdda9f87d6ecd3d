// Voice library behind the C ABI: a device-resident table of unit-length speaker embeddings and the nearest
// rows of up to 32 queries.
//   fq3_voices_create / _destroy / _count / _reset      the table [capacity][dim] (fragment-major), a live byte per row, the workspace
//   fq3_voices_add                                      ONE launch: rows normalised and appended
//   fq3_voices_drop                                     one byte cleared on the stream; indices of other rows do not move
//   fq3_voices_search                                   THREE launches whatever N, rows and k: query pack, scan (the library crosses
//                                                       HBM once, the scores stay in registers and LDS), merge
// The host tracks the row count; every argument is validated before the first HIP call.  One search at a time per object: the query
// operand and the partials are the object's.
#include "../../include/fq3hip.h"
#include "fq3_common.cuh"
#include "voices_kernels.cuh"

#include <cstring>
#include <string>

using namespace fq3;

int fq3_fail_(int code, const std::string& m);                 // fq3_api.hip: sets the thread-local error string
#define KHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fq3_fail_(FQ3_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kMinSlab = kVoiceWaves * 16;                     // one row block per wave
constexpr int kMaxDim = 8192;
constexpr int64_t kMaxCapacity = (int64_t)1 << 22;             // the merge keeps a cursor byte per slab in LDS: 32 KB at most

int64_t slabs_(int64_t count, int slab) { return count > 0 ? (count + slab - 1) / slab : 1; }
int64_t part_bytes_(int64_t slabs, int k) { return slabs * kVoiceQueries * k * (int64_t)sizeof(unsigned long long); }

}  // namespace

struct fq3_voices {
    int dim = 0;
    int64_t capacity = 0, count = 0;
    float* lib = nullptr;                     // [ceil(capacity / 16)][dim / 16][64][4]
    uint8_t* live = nullptr;                  // [ceil(capacity / 16) * 16]
    float* qp = nullptr;                      // [2][dim / 16][64][4]
    unsigned long long* part = nullptr;       // [ceil(capacity / kMinSlab)][32][16]
    int slab = 256;                           // rows per workgroup of the scan: 128, 256 or 512
};

namespace {

template <int RB>
size_t scan_lds_() { return (size_t)((kVoiceQueries * (kVoiceWaves * RB * 16 + 1) + 3) & ~3) * sizeof(float); }

}  // namespace

extern "C" int fq3_voices_create(int dim, int64_t capacity, fq3_voices** out) {
    if (!out) return fq3_fail_(FQ3_EINVAL, "fq3_voices_create: null out");
    *out = nullptr;
    if (dim < 16 || dim > kMaxDim || dim % 16) return fq3_fail_(FQ3_EINVAL, "fq3_voices_create: dim must be a multiple of 16 in [16, 8192]");
    if (capacity < 1 || capacity > kMaxCapacity) return fq3_fail_(FQ3_EINVAL, "fq3_voices_create: capacity outside [1, 2^22]");
    fq3_voices* v = new fq3_voices;
    v->dim = dim;
    v->capacity = capacity;
    const int64_t padded = (capacity + 15) / 16 * 16;
    hipError_t e = hipMalloc((void**)&v->lib, (size_t)padded * dim * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&v->live, (size_t)padded);
    if (e == hipSuccess) e = hipMalloc((void**)&v->qp, (size_t)kVoiceQueries * dim * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&v->part, (size_t)part_bytes_(slabs_(capacity, kMinSlab), kVoiceMaxK));
    if (e == hipSuccess) e = hipMemset(v->live, 0, (size_t)padded);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)fq3_voices_destroy(v);
        return fq3_fail_(e == hipErrorOutOfMemory ? FQ3_ENOMEM : FQ3_EHIP, std::string("fq3_voices_create: ") + hipGetErrorString(e));
    }
    *out = v;
    return 0;
}

extern "C" int fq3_voices_destroy(fq3_voices* v) {
    if (!v) return 0;
    (void)hipFree(v->lib); (void)hipFree(v->live); (void)hipFree(v->qp); (void)hipFree(v->part);
    delete v;
    return 0;
}

extern "C" int64_t fq3_voices_count(const fq3_voices* v) {
    if (!v) return fq3_fail_(FQ3_EINVAL, "fq3_voices_count: null object");
    return v->count;
}

extern "C" int fq3_voices_slab_rows(const fq3_voices* v) {
    if (!v) return fq3_fail_(FQ3_EINVAL, "fq3_voices_slab_rows: null object");
    return v->slab;
}

extern "C" int fq3_voices_set_option(fq3_voices* v, const char* name, int value) {
    if (!v || !name) return fq3_fail_(FQ3_EINVAL, "fq3_voices_set_option: null argument");
    if (!std::strcmp(name, "slab_rows")) {
        if (value != 128 && value != 256 && value != 512) return fq3_fail_(FQ3_EINVAL, "fq3_voices_set_option: slab_rows is 128, 256 or 512");
        v->slab = value;
    } else {
        return fq3_fail_(FQ3_EINVAL, std::string("fq3_voices_set_option: unknown option ") + name);
    }
    return 0;
}

extern "C" int64_t fq3_voices_add(fq3_voices* v, const float* embeds, int64_t rows, void* stream) {
    if (!v || !embeds) return fq3_fail_(FQ3_EINVAL, "fq3_voices_add: null argument");
    if (rows < 1 || rows > kMaxCapacity) return fq3_fail_(FQ3_EINVAL, "fq3_voices_add: rows outside [1, 2^22]");
    if (rows > v->capacity - v->count)
        return fq3_fail_(FQ3_ENOMEM, "fq3_voices_add: " + std::to_string(rows) + " rows do not fit: " + std::to_string(v->count) + " of " +
                                     std::to_string(v->capacity) + " taken");
    const int64_t first = v->count, end = (first + rows + 15) / 16 * 16;
    hipLaunchKernelGGL(voices_add_kernel, dim3((unsigned)((end - first + 3) / 4)), dim3(256), 0, (hipStream_t)stream, embeds, v->lib, v->live,
                       (long)first, (long)rows, v->dim);
    KHIP(hipGetLastError());
    v->count += rows;
    return first;
}

extern "C" int fq3_voices_drop(fq3_voices* v, int64_t index, void* stream) {
    if (!v) return fq3_fail_(FQ3_EINVAL, "fq3_voices_drop: null object");
    if (index < 0 || index >= v->count) return fq3_fail_(FQ3_EINVAL, "fq3_voices_drop: index " + std::to_string(index) + " outside [0, count)");
    KHIP(hipMemsetAsync(v->live + index, 0, 1, (hipStream_t)stream));
    return 0;
}

extern "C" int fq3_voices_reset(fq3_voices* v) {
    if (!v) return fq3_fail_(FQ3_EINVAL, "fq3_voices_reset: null object");
    KHIP(hipDeviceSynchronize());
    KHIP(hipMemset(v->live, 0, (size_t)((v->capacity + 15) / 16 * 16)));
    v->count = 0;
    return 0;
}

static int search_check_(const std::string& who, const fq3_voices* v, int rows, int k) {
    if (!v) return fq3_fail_(FQ3_EINVAL, who + ": null object");
    if (rows < 1 || rows > kVoiceQueries) return fq3_fail_(FQ3_EINVAL, who + ": rows = " + std::to_string(rows) + "; a call has 1 to 32 queries");
    if (k < 1 || k > kVoiceMaxK) return fq3_fail_(FQ3_EINVAL, who + ": k = " + std::to_string(k) + " outside [1, 16]");
    return 0;
}

extern "C" int64_t fq3_voices_search_workspace(const fq3_voices* v, int rows, int k) {
    if (int rc = search_check_("fq3_voices_search_workspace", v, rows, k)) return rc;
    return (int64_t)kVoiceQueries * v->dim * (int64_t)sizeof(float) + part_bytes_(slabs_(v->count, v->slab), k);
}

extern "C" int fq3_voices_search(fq3_voices* v, const float* q, int rows, int k, int32_t* idx, float* cos, void* stream) {
    if (int rc = search_check_("fq3_voices_search", v, rows, k)) return rc;
    if (!q || !idx || !cos) return fq3_fail_(FQ3_EINVAL, "fq3_voices_search: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t slabs = slabs_(v->count, v->slab);
    const int tiles = rows > 16 ? 2 : 1, kq_n = v->dim / 16;
    const long count = (long)v->count;
    return with_value<1, 2, 4>(v->slab / kMinSlab, [&](auto rb) {
        constexpr int RB = decltype(rb)::value;
        if (!lds_limit_at_least<voices_scan_kernel<RB, false>>(scan_lds_<RB>()))          // asked before the first launch
            return fq3_fail_(FQ3_EHIP, "fq3_voices_search: the scan's dynamic LDS was refused");
        hipLaunchKernelGGL(voices_query_pack_kernel, dim3(kVoiceQueries / 4), dim3(256), 0, st, q, v->qp, rows, v->dim);
        hipLaunchKernelGGL((voices_scan_kernel<RB, false>), dim3((unsigned)slabs), dim3(kVoiceWaves * 64), scan_lds_<RB>(), st, v->lib, v->qp, v->live,
                           v->part, count, kq_n, tiles, rows, k);
        hipLaunchKernelGGL(voices_merge_kernel, dim3(rows), dim3(kVoiceMergeThreads), (size_t)((slabs + 15) & ~15LL), st, v->part, (int)slabs, k, idx, cos);
        KHIP(hipGetLastError());
        return 0;
    });
}
