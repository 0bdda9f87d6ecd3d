// Host only, no HIP: the argument check of fq3_noise_fill, kept apart from the launcher so that a stand-alone program can be built
// from it with the host sanitizers (tools/microbench/noise_args_check.cpp).  All-or-nothing: the launcher queues nothing unless this
// returns null for the whole call.
#pragma once
#include "../../include/fq3hip.h"

// null when the call may be queued, the complaint otherwise
inline const char* fq3_noise_fill_check_(const fq3_noise_ring* rings, int n, int ring_frames, int dtype, int V, int G, int Vp) {
    if (V < 1 || G < 1 || Vp < 1 || (dtype != FQ3_BF16 && dtype != FQ3_F32)) return "noise fill: the context has no config";
    if (n < 0) return "noise fill: n must not be negative";
    if (n > 0 && !rings) return "noise fill: rings is NULL";
    if (ring_frames < 1) return "noise fill: ring_frames must be at least 1";
    const unsigned align = dtype == FQ3_BF16 ? 1u : 3u;
    for (int i = 0; i < n; ++i) {
        if (rings[i].n_frames < 0 || rings[i].n_frames > ring_frames) return "noise fill: n_frames must be in [0, ring_frames]";
        if (((uintptr_t)rings[i].talker & align) || ((uintptr_t)rings[i].pred & align)) return "noise fill: a ring is not aligned to its element type";
    }
    return nullptr;
}
