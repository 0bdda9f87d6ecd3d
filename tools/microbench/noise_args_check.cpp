// Host only: the argument check of fq3_noise_fill (csrc/noise_args.h) in a stand-alone program, so that it can be built with the host
// sanitizers (`make -C faster-qwen3-tts_amd noise_args_check` builds and runs it with -fsanitize=address,undefined).  No GPU, no HIP:
// the check is what stands between a caller's descriptor array and the launch.
#include "../../faster-qwen3-tts_amd/csrc/noise_args.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

static void expect(bool ok_wanted, const char* why, const char* what) {
    const bool ok = why == nullptr;
    if (ok != ok_wanted) {
        std::printf("FAIL %s: %s\n", what, why ? why : "accepted");
        ++failures;
    }
}

int main() {
    const int V = 3072, G = 16, Vp = 2048, R = 64;
    alignas(16) static float talker[8], pred[8];             // never dereferenced by the check: only their addresses travel
    auto ring = [&](int n_frames, uint32_t first = 0) {
        fq3_noise_ring r;
        std::memset(&r, 0, sizeof r);
        r.talker = talker; r.pred = pred; r.seed = 0xFFFFFFFFFFFFFFFFull; r.first_frame = first; r.n_frames = n_frames;
        return r;
    };
    for (int n : {0, 1, 32, 33, 128}) {                       // exactly n descriptors on the heap: a read past the end is caught
        std::vector<fq3_noise_ring> rs;
        for (int i = 0; i < n; ++i) rs.push_back(ring(i % (R + 1), 0xFFFFFFFFu - (uint32_t)i));
        expect(true, fq3_noise_fill_check_(n ? rs.data() : nullptr, n, R, FQ3_BF16, V, G, Vp), "valid rings");
        if (n) {
            rs.back().n_frames = R + 1;
            expect(false, fq3_noise_fill_check_(rs.data(), n, R, FQ3_F32, V, G, Vp), "n_frames above the ring in the last entry");
            rs.back().n_frames = -1;
            expect(false, fq3_noise_fill_check_(rs.data(), n, R, FQ3_F32, V, G, Vp), "negative n_frames in the last entry");
        }
    }
    fq3_noise_ring one = ring(R);
    expect(false, fq3_noise_fill_check_(nullptr, 1, R, FQ3_BF16, V, G, Vp), "NULL rings with n > 0");
    expect(false, fq3_noise_fill_check_(&one, -1, R, FQ3_BF16, V, G, Vp), "negative n");
    expect(false, fq3_noise_fill_check_(&one, 1, 0, FQ3_BF16, V, G, Vp), "ring_frames 0");
    expect(false, fq3_noise_fill_check_(&one, 1, R, FQ3_BF16, 0, G, Vp), "a context without a config");
    expect(false, fq3_noise_fill_check_(&one, 1, R, 7, V, G, Vp), "an unknown dtype");
    one.talker = (char*)talker + 2;
    expect(true, fq3_noise_fill_check_(&one, 1, R, FQ3_BF16, V, G, Vp), "a bf16 ring at 2-byte alignment");
    expect(false, fq3_noise_fill_check_(&one, 1, R, FQ3_F32, V, G, Vp), "an fp32 ring at 2-byte alignment");
    one.talker = nullptr; one.pred = nullptr;
    expect(true, fq3_noise_fill_check_(&one, 1, R, FQ3_F32, V, G, Vp), "an entry without rings");
    std::printf(failures ? "%d failures\n" : "noise_args_check ok\n", failures);
    return failures ? 1 : 0;
}
