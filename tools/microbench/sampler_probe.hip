// Conformance probe of the sampler kernels (csrc/sampler.cuh: sample_api_kernel, sample_pred_kernel, sample_talker_kernel;
// csrc/sampler_wave.cuh: sample_api_wave_kernel, sample_pred_wave_kernel, sample_talker_wave_kernel; csrc/batch_kernels.cuh:
// sample_pred_batch_kernel, sample_talker_batch_kernel): a shared library with a C ABI that launches exactly ONE named instantiation on
// caller-owned device buffers, so that tests/test_gpu_sampler_reference.py can compare every token and every byte the kernels write
// with the float64 reference of tests/_sampler_ref.py.  It includes the product headers (no sampling arithmetic of its own), takes the
// chunk count of the register kinds from the launchers' own rule (sampler_wave.cuh: dispatch_nc) unless the caller names one, and
// never links into libfq3hip.so.
//
// Anything that would make a kernel read or write outside the buffers the arguments describe is refused with kRefused and nothing is
// launched: V <= 0, V > kMaxVocab, V % 8; H % 8 for the register kinds; B outside 1..kMaxLanes; a null required pointer; a row that
// is not 16-byte aligned (the register kinds load 8 elements at once); sampling without noise; a noise ring shorter than
// noise_frames; a codes / teacher-forcing slot beyond codes_len / tf_len.  For the in-graph kinds the probe reads the DecodeState(s)
// back from the device to know the policy, the frame and the noise pointers the kernel will see.
#include "../../faster-qwen3-tts_amd/csrc/batch_kernels.cuh"
#include <cstddef>
#include <cstdint>
#include <vector>
using namespace fq3;

namespace {

constexpr int kProbeVersion = 1;
constexpr int kRefused = 100000;

enum Kind {
    K_API = 0,          // sample_api_kernel<T>: history list, LDS core
    K_API_WAVE,         // sample_api_wave_kernel<T, NC>: seen bitmap, register core
    K_PRED,             // sample_pred_kernel<T>
    K_PRED_WAVE,        // sample_pred_wave_kernel<T, NC>
    K_TALKER,           // sample_talker_kernel<T>
    K_TALKER_WAVE,      // sample_talker_wave_kernel<T, NC>
    K_PRED_BATCH,       // sample_pred_batch_kernel<T, NC> (NUCLEUS bodies)
    K_TALKER_BATCH,     // sample_talker_batch_kernel<T, NC> (NUCLEUS bodies)
    K_COUNT
};
enum Te { TE_BF16 = 0, TE_F32 = 2 };          // the storage-type codes of the other probes

int g_last_inst = -1;                          // id of the instantiation the last successful run launched

constexpr bool reg_kind(int kind) { return kind != K_API && kind != K_PRED && kind != K_TALKER; }
constexpr bool batch_kind(int kind) { return kind == K_PRED_BATCH || kind == K_TALKER_BATCH; }
constexpr bool pred_kind(int kind) { return kind == K_PRED || kind == K_PRED_WAVE || kind == K_PRED_BATCH; }
constexpr bool talker_kind(int kind) { return kind == K_TALKER || kind == K_TALKER_WAVE || kind == K_TALKER_BATCH; }
// nc = 0 for the LDS kinds, the chunk count for the register kinds
constexpr int inst_id(int kind, int te, int nc) { return (kind * 2 + (te ? 1 : 0)) * 3 + nc; }

}  // namespace

extern "C" {

// Everything one probe launch needs.  Device pointers unless said otherwise; T = the storage type of the call.
//   logits: [V] (batch kinds: [B] rows, logit_stride elements apart for the predictor, V apart for the talker)
//   noise: [V] Exp(1) variates for the api kinds and the predictor kinds without a state or with st->pred_noise null; the rings the
//   state(s) point to hold noise_rows rows of V each (talker: >= noise_frames; predictor: >= noise_frames * (G - 1))
//   seen: [V] bytes (api_wave, talker); history: [n_hist] ids (api)
//   st: DecodeState (predictor: may be null); codes: [codes_len] or null; out64: [G - 1] or null; next_emb: [rows >= every id][H] or
//   null; next_in: [H] (batch: [B][H]); tf: TeacherForcing whose arrays hold tf_len slots, or null
//   lane_st / lane_codes / lane_seen / lane_tf: HOST arrays of B device pointers (the probe builds LaneTab / LaneForced from them);
//   lane_codes, lane_seen, lane_tf and their entries may be null
struct SamplerProbeArgs {
    int V, H, G, B, cb;
    int nc;                         // register kinds: 0 = the launchers' rule, 1 or 2 = that instantiation (1 needs V <= 2048)
    int n_hist, noise_rows, codes_len, tf_len;
    long logit_stride;
    SampleCfg cfg;
    const void* logits; const void* noise; const unsigned char* seen; const long long* history;
    long long* out;
    void* st; int* codes; long long* out64; const void* next_emb; void* next_in; const void* tf;
    void* const* lane_st; int* const* lane_codes; unsigned char* const* lane_seen; const void* const* lane_tf;
};

int sampler_probe_version() { return kProbeVersion; }
int sampler_probe_kinds() { return K_COUNT; }
int sampler_probe_refused_code() { return kRefused; }
int sampler_probe_last_inst() { return g_last_inst; }
// the launchers' chunk rule (sampler_wave.cuh)
int sampler_probe_rule_nc(int V) {
    int nc = 0;
    dispatch_nc(V, [&](auto v) { nc = decltype(v)::value; });
    return nc;
}

// struct layouts for the ctypes mirrors: four groups of [sizeof, offsets of the fields in declaration order] -- DecodeState, SampleCfg,
// TeacherForcing, SamplerProbeArgs -- then kMaxVocab, kMaxLanes; returns the number of values written
int sampler_probe_layout(long* out, int cap) {
#define D(f) (long)offsetof(DecodeState, f)
#define S(f) (long)offsetof(SampleCfg, f)
#define F(f) (long)offsetof(TeacherForcing, f)
#define P(f) (long)offsetof(SamplerProbeArgs, f)
    const long v[] = {(long)sizeof(DecodeState),
                      D(token), D(frame), D(pos), D(gen_step), D(done), D(text_open), D(min_new), D(max_new), D(trailing_len), D(noise_frames),
                      D(eos_id), D(max_seq), D(sup_lo), D(sup_hi), D(t_temperature), D(t_top_k), D(t_top_p), D(t_do_sample), D(t_rep_penalty),
                      D(p_temperature), D(p_top_k), D(p_top_p), D(p_do_sample), D(trailing_text), D(tts_pad), D(talker_noise), D(pred_noise),
                      D(past_hidden_init), D(n_pad), D(rope_delta),
                      (long)sizeof(SampleCfg),
                      S(temperature), S(top_k), S(top_p), S(do_sample), S(rep_penalty), S(sup_lo), S(sup_hi), S(keep_id), S(sup_extra),
                      (long)sizeof(TeacherForcing), F(forced), F(decisions),
                      (long)sizeof(SamplerProbeArgs),
                      P(V), P(H), P(G), P(B), P(cb), P(nc), P(n_hist), P(noise_rows), P(codes_len), P(tf_len), P(logit_stride), P(cfg),
                      P(logits), P(noise), P(seen), P(history), P(out), P(st), P(codes), P(out64), P(next_emb), P(next_in), P(tf),
                      P(lane_st), P(lane_codes), P(lane_seen), P(lane_tf),
                      (long)kMaxVocab, (long)kMaxLanes};
#undef D
#undef S
#undef F
#undef P
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"

namespace {

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// the policy a launch will sample with must be served by the buffers: noise present, temperature positive
bool policy_ok(int do_sample, float temperature, const void* noise) {
    return !do_sample || (noise && temperature > 0.f);
}

// one lane's state, codes and forcing object against the described buffers
bool lane_ok(int kind, const SamplerProbeArgs& p, const void* st_dev, const int* codes, const void* tf, bool imm_noise) {
    DecodeState st;
    if (hipMemcpy(&st, st_dev, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (st.frame < 0 || st.frame > (1 << 20)) return false;
    const long slot = pred_kind(kind) ? (long)st.frame * p.G + 1 + p.cb : ((long)st.frame + 1) * p.G;
    if (tf && slot >= p.tf_len) return false;
    if (pred_kind(kind)) {
        if (codes && slot >= p.codes_len) return false;
        const void* nz = st.pred_noise ? st.pred_noise : (imm_noise ? p.noise : nullptr);
        if (!policy_ok(st.p_do_sample, st.p_temperature, nz)) return false;
        if (st.p_do_sample && st.pred_noise && (st.noise_frames < 1 || (long)p.noise_rows < (long)st.noise_frames * (p.G - 1))) return false;
        if (st.p_do_sample && reg_kind(kind) && !aligned(nz, 16)) return false;
    } else {
        if (!policy_ok(st.t_do_sample, st.t_temperature, st.talker_noise)) return false;
        if (st.t_do_sample && (st.noise_frames < 1 || p.noise_rows < st.noise_frames)) return false;
        if (st.t_do_sample && reg_kind(kind) && !aligned(st.talker_noise, 16)) return false;
    }
    return true;
}

bool admits(int kind, int te, const SamplerProbeArgs& p) {
    if ((te != TE_BF16 && te != TE_F32) || kind < 0 || kind >= K_COUNT) return false;
    const size_t esz = te == TE_BF16 ? 2 : 4;
    if (p.V <= 0 || p.V > kMaxVocab || p.V % 8 || !p.logits) return false;
    if (reg_kind(kind)) {
        if (p.nc < 0 || p.nc > 2 || (p.nc == 1 && p.V > 2048)) return false;
        if (!aligned(p.logits, 16)) return false;
    } else if (p.nc != 0) return false;
    if (kind == K_API || kind == K_API_WAVE) {
        if (!p.out || !policy_ok(p.cfg.do_sample, p.cfg.temperature, p.noise)) return false;
        if (kind == K_API) return p.n_hist >= 0 && (p.n_hist == 0 || p.history);
        return (!p.cfg.do_sample || aligned(p.noise, 16)) && aligned(p.seen, 8);
    }
    if (p.G < 2) return false;
    if (pred_kind(kind)) {
        if (p.cb < 0 || p.cb > p.G - 2) return false;
        if (p.next_emb && (!p.next_in || p.H <= 0)) return false;
        if (p.next_emb && reg_kind(kind) && (p.H % 8 || !aligned(p.next_emb, 16) || !aligned(p.next_in, 16))) return false;
    }
    if (!batch_kind(kind)) {
        if (talker_kind(kind)) {
            if (!p.st || (reg_kind(kind) && !aligned(p.seen, 8))) return false;
            return lane_ok(kind, p, p.st, nullptr, p.tf, false);
        }
        if (p.st) return lane_ok(kind, p, p.st, p.codes, p.tf, true);
        if (!policy_ok(p.cfg.do_sample, p.cfg.temperature, p.noise) || (p.cfg.do_sample && reg_kind(kind) && !aligned(p.noise, 16))) return false;
        return !p.codes || 1 + p.cb < p.codes_len;
    }
    if (p.B < 1 || p.B > kMaxLanes || !p.lane_st) return false;
    const long stride = kind == K_PRED_BATCH ? p.logit_stride : (long)p.V;
    if (stride < p.V || (stride * esz) % 16) return false;
    for (int l = 0; l < p.B; ++l) {
        if (!p.lane_st[l]) return false;
        if (kind == K_TALKER_BATCH && p.lane_seen && !aligned(p.lane_seen[l], 8)) return false;
        if (!lane_ok(kind, p, p.lane_st[l], p.lane_codes ? p.lane_codes[l] : nullptr, p.lane_tf ? p.lane_tf[l] : nullptr, false)) return false;
    }
    return true;
}

int finish(hipStream_t s) {
    const int rc = (int)hipGetLastError();
    const int rs = (int)hipStreamSynchronize(s);
    return rc ? rc : rs;
}

// the chunk count of a register-kind launch: the caller's, or the launchers' rule
template <typename F>
void with_nc(const SamplerProbeArgs& p, F&& f) {
    if (p.nc == 1) f(std::integral_constant<int, 1>{});
    else if (p.nc == 2) f(std::integral_constant<int, 2>{});
    else dispatch_nc(p.V, f);
}

// device copies of the per-lane tables for the duration of one launch
struct LaneTables {
    LaneTab* tab = nullptr;
    LaneForced* lf = nullptr;
    int make(const SamplerProbeArgs& p) {
        LaneTab t{};
        LaneForced f{};
        for (int l = 0; l < p.B; ++l) {
            t.st[l] = reinterpret_cast<DecodeState*>(p.lane_st[l]);
            t.codes[l] = p.lane_codes ? p.lane_codes[l] : nullptr;
            t.seen[l] = p.lane_seen ? p.lane_seen[l] : nullptr;
            f.tf[l] = p.lane_tf ? reinterpret_cast<const TeacherForcing*>(p.lane_tf[l]) : nullptr;
        }
        if (hipMalloc((void**)&tab, sizeof(t)) != hipSuccess || hipMalloc((void**)&lf, sizeof(f)) != hipSuccess) return (int)hipGetLastError();
        if (hipMemcpy(tab, &t, sizeof(t), hipMemcpyHostToDevice) != hipSuccess) return (int)hipGetLastError();
        if (hipMemcpy(lf, &f, sizeof(f), hipMemcpyHostToDevice) != hipSuccess) return (int)hipGetLastError();
        return 0;
    }
    ~LaneTables() { if (tab) (void)hipFree(tab); if (lf) (void)hipFree(lf); }
};

template <typename T>
int run(int kind, int te, const SamplerProbeArgs& p, hipStream_t s) {
    const T* lg = reinterpret_cast<const T*>(p.logits);
    const T* nz = reinterpret_cast<const T*>(p.noise);
    const T* emb = reinterpret_cast<const T*>(p.next_emb);
    T* nin = reinterpret_cast<T*>(p.next_in);
    DecodeState* st = reinterpret_cast<DecodeState*>(p.st);
    const TeacherForcing* tf = reinterpret_cast<const TeacherForcing*>(p.tf);
    int64_t* out = reinterpret_cast<int64_t*>(p.out);
    int64_t* out64 = reinterpret_cast<int64_t*>(p.out64);
    const dim3 one(1), blk(256);
    switch (kind) {
        case K_API:
            g_last_inst = inst_id(kind, te, 0);
            hipLaunchKernelGGL((sample_api_kernel<T>), one, blk, 0, s, lg, p.V, p.cfg, reinterpret_cast<const int64_t*>(p.history), p.n_hist, nz, out);
            break;
        case K_PRED:
            g_last_inst = inst_id(kind, te, 0);
            hipLaunchKernelGGL((sample_pred_kernel<T>), one, blk, 0, s, st, lg, p.V, p.cb, p.cfg, nz, p.codes, p.G, out64, emb, nin, p.H, tf);
            break;
        case K_TALKER:
            g_last_inst = inst_id(kind, te, 0);
            hipLaunchKernelGGL((sample_talker_kernel<T>), one, blk, 0, s, st, lg, p.V, p.seen, p.G, tf);
            break;
        case K_API_WAVE:
            with_nc(p, [&](auto nc) {
                constexpr int NC = decltype(nc)::value;
                g_last_inst = inst_id(kind, te, NC);
                hipLaunchKernelGGL((sample_api_wave_kernel<T, NC>), one, blk, 0, s, lg, p.V, p.cfg, p.seen, nz, out);
            });
            break;
        case K_PRED_WAVE:
            with_nc(p, [&](auto nc) {
                constexpr int NC = decltype(nc)::value;
                g_last_inst = inst_id(kind, te, NC);
                sample_pred_wave_launch<T, NC>(st, lg, p.V, p.cb, p.cfg, nz, p.codes, p.G, out64, emb, nin, p.H, tf, s);
            });
            break;
        case K_TALKER_WAVE:
            with_nc(p, [&](auto nc) {
                constexpr int NC = decltype(nc)::value;
                g_last_inst = inst_id(kind, te, NC);
                sample_talker_wave_launch<T, NC>(st, lg, p.V, p.seen, p.G, tf, s);
            });
            break;
        case K_PRED_BATCH:
        case K_TALKER_BATCH: {
            LaneTables lt;
            if (int r = lt.make(p)) return r;
            with_nc(p, [&](auto nc) {
                constexpr int NC = decltype(nc)::value;
                g_last_inst = inst_id(kind, te, NC);
                if (kind == K_PRED_BATCH)
                    hipLaunchKernelGGL((sample_pred_batch_kernel<T, NC>), dim3(p.B), blk, 0, s, lt.tab, lt.lf, lg, (size_t)p.logit_stride, p.V, p.cb, p.G,
                                       emb, nin, p.H);
                else
                    hipLaunchKernelGGL((sample_talker_batch_kernel<T, NC>), dim3(p.B), blk, 0, s, lt.tab, lt.lf, lg, p.V, p.G);
            });
            return finish(s);                     // (the tables are freed after the wait)
        }
        default: return kRefused;
    }
    return finish(s);
}

}  // namespace

extern "C" {

// 1 = these arguments stay inside the buffers they describe for kind `kind` in storage type te (0 bf16, 2 fp32)
int sampler_probe_admits(int kind, int te, const SamplerProbeArgs* p) { return p && admits(kind, te, *p) ? 1 : 0; }

// launch exactly one instantiation and wait for it; returns the HIP error of the launch or the wait, or kRefused (nothing launched)
int sampler_probe_run(int kind, int te, const SamplerProbeArgs* p, hipStream_t s) {
    if (!p || !admits(kind, te, *p)) return kRefused;
    return te == TE_F32 ? run<float>(kind, te, *p, s) : run<bf16_t>(kind, te, *p, s);
}

}  // extern "C"
