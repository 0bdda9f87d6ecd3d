"""CPU: every `__global__` definition under csrc/ has a reference test that launches it.

The census parses csrc/*.cuh and csrc/*.hip for kernel definitions (kernels are named *_kernel) and looks each one up in COVERAGE below:
kernel -> (the GPU test that launches it and compares it with a reference, the file in which that test names it).  The second file is
the test itself or the reference module it imports (tests/_*_ref.py: the probes' kind lists live there).  Both files must exist, the test
must import the module, and the file must name the kernel: by its full name, by its name without the `_kernel` suffix (the kind names of
the probes), or by the alias written into the table, which is then the family name the test uses for it.

Exemptions carry a reason and are limited to kernels that take no data.  A new kernel without an entry fails here: give it a kind in a
probe and a reference, then add the line."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faster-qwen3-tts_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

ATTN, GEMV, GEMM = "test_gpu_attn_reference.py", "test_gpu_gemv_reference.py", "test_gpu_gemm_reference.py"
PATTN, CONT, PACK = "test_gpu_prefill_attn_reference.py", "test_gpu_prefill_cont_reference.py", "test_gpu_prefill_pack_cont_reference.py"
SAMP, ROWS, STATE = "test_gpu_sampler_reference.py", "test_gpu_rows_reference.py", "test_gpu_state_reference.py"

# kernel -> (test, file that names it[, alias])
COVERAGE = {
    # decode and batch attention
    "attn_decode_kernel": (ATTN, ATTN), "attn_pred_kernel": (ATTN, ATTN), "attn_decode_batch_kernel": (ATTN, ATTN),
    "attn_decode_lane_kernel": (ATTN, ATTN), "attn_pred_batch_kernel": (ATTN, ATTN), "attn_pred_group_batch_kernel": (ATTN, ATTN),
    "combine_batch_kernel": (ATTN, ATTN),
    # decode GEMVs
    "gemv_kernel": (GEMV, GEMV), "gemv_batch_kernel": (GEMV, GEMV), "gemv_batch_mfma_norm_kernel": (GEMV, GEMV),
    "gemv_batch_mfma_plain_kernel": (GEMV, GEMV), "rmsnorm_batch_kernel": (GEMV, GEMV),
    # GEMM families (the test names the families of gemm_probe.hip)
    "conv_gemm_kernel": (GEMM, GEMM, "conv64x32"), "glds_gemm_kernel": (GEMM, GEMM, "glds4_128x64_s2"), "chain_gemm_kernel": (GEMM, GEMM, "chain8x8"),
    "big_gemm_kernel": (GEMM, GEMM, "big_ring"), "splitk_reduce_kernel": (GEMM, GEMM), "skinny_gemm_kernel": (GEMM, GEMM, "skinny"),
    "skinny_pack_kernel": (GEMM, GEMM, "gemm_probe_pack"), "resunit_kernel": (GEMM, GEMM),
    # prefill and windowed attention
    "qk_norm_rope_kv_kernel": (PATTN, PATTN), "qk_norm_rope_kv_pack_kernel": (PATTN, PATTN), "prefill_attn_kernel": (PATTN, PATTN),
    "flash_prefill_kernel": (PATTN, PATTN), "flash_prefill_small_kernel": (PATTN, PATTN), "swa_attn_kernel": (PATTN, PATTN),
    "win_attn_kernel": (PATTN, PATTN),
    "qk_norm_rope_kv_cont_kernel": (CONT, CONT), "prefill_attn_cont_kernel": (CONT, CONT), "flash_prefill_cont_kernel": (CONT, CONT),
    "flash_cont_merge_kernel": (CONT, "_prefill_cont_ref.py"),
    "qk_norm_rope_kv_cont_pack_kernel": (PACK, PACK), "flash_prefill_cont_pack_kernel": (PACK, PACK), "flash_cont_pack_merge_kernel": (PACK, PACK),
    # samplers
    "sample_api_kernel": (SAMP, SAMP), "sample_pred_kernel": (SAMP, SAMP), "sample_talker_kernel": (SAMP, SAMP),
    "sample_api_wave_kernel": (SAMP, SAMP), "sample_pred_wave_kernel": (SAMP, SAMP), "sample_talker_wave_kernel": (SAMP, SAMP),
    "sample_pred_batch_kernel": (SAMP, SAMP), "sample_talker_batch_kernel": (SAMP, SAMP), "build_seen_kernel": (SAMP, SAMP),
    "rep_penalty_kernel": (SAMP, SAMP, "fq3_apply_repetition_penalty"),
    # vocoder and analyser row kernels (kind names in _rows_ref.py)
    "rvq_gather_kernel": (ROWS, "_rows_ref.py"), "rvq_gather_new_kernel": (ROWS, "_rows_ref.py"), "prefix_rows_kernel": (ROWS, "_rows_ref.py"),
    "keep_rows_kernel": (ROWS, "_rows_ref.py"), "rmsnorm_rows_kernel": (ROWS, ROWS), "rmsnorm_rows_vec_kernel": (ROWS, ROWS, "rmsnorm_rows_vec"),
    "layernorm_rows_kernel": (ROWS, "_rows_ref.py"), "dwconv7_kernel": (ROWS, "_rows_ref.py"), "silu_mul_kernel": (ROWS, "_rows_ref.py"),
    "rope_rows_kernel": (ROWS, ROWS), "rope_rows_pos_kernel": (ROWS, "_rows_ref.py"), "final_conv_kernel": (ROWS, "_rows_ref.py"),
    "snake_consts_kernel": (ROWS, "_rows_ref.py"), "conv_in_kernel": (ROWS, "_rows_ref.py"), "pad_rows_kernel": (ROWS, "_rows_ref.py"),
    "codebook_prepare_kernel": (ROWS, "_rows_ref.py"), "rvq_encode_kernel": (ROWS, "_rows_ref.py", "rvq_encode_1_1"),
    "dft_mag_kernel": (ROWS, "_rows_ref.py"), "col_stats_kernel": (ROWS, "_rows_ref.py"), "se_scale_kernel": (ROWS, "_rows_ref.py"),
    # output stages: each has its own test against its own reference module, named by the header that holds the kernel
    "audio_out_kernel": ("test_gpu_audio_out.py", "test_gpu_audio_out.py", "audio_kernels.cuh"),
    "tsm_kernel": ("test_gpu_tsm.py", "test_gpu_tsm.py", "tsm_kernels.cuh"),
    "flac_encode_kernel": ("test_gpu_flac.py", "test_gpu_flac.py", "flac_kernels.cuh"),
    "flac_gather_kernel": ("test_gpu_flac.py", "test_gpu_flac.py", "flac_kernels.cuh"),
    "join_kernel": ("test_gpu_join.py", "test_gpu_join.py", "join_kernels.cuh"),
    "loud_push_kernel": ("test_gpu_loudness.py", "test_gpu_loudness.py", "loud_kernels.cuh"),
    "loud_finish_kernel": ("test_gpu_loudness.py", "test_gpu_loudness.py", "loud_kernels.cuh"),
    "loud_apply_kernel": ("test_gpu_loudness.py", "test_gpu_loudness.py", "loud_kernels.cuh"),
    "noise_fill_kernel": ("test_gpu_noise.py", "test_gpu_noise.py"), "noise_row_kernel": ("test_gpu_noise.py", "test_gpu_noise.py", "noise_first"),
    "noise_words_kernel": ("test_gpu_noise.py", "test_gpu_noise.py", "fq3_noise_words"),
    # decode-loop state, prompt and KV glue (kernel names in _state_ref.KERNEL)
    "frame_begin_kernel": (STATE, "_state_ref.py"), "embed_sum_kernel": (STATE, "_state_ref.py"), "rmsnorm_kernel": (STATE, "_state_ref.py"),
    "copy_kernel": (STATE, "_state_ref.py"), "frame_begin_batch_kernel": (STATE, "_state_ref.py"), "embed_sum_batch_kernel": (STATE, "_state_ref.py"),
    "text_gather_kernel": (STATE, "_state_ref.py"), "prompt_rows_kernel": (STATE, "_state_ref.py"), "text_open_kernel": (STATE, "_state_ref.py"),
    "text_publish_kernel": (STATE, "_state_ref.py"), "poll_gather_kernel": (STATE, "_state_ref.py"), "text_scatter_kernel": (STATE, "_state_ref.py"),
    "text_publish_lanes_kernel": (STATE, "_state_ref.py"), "kv_table_write_kernel": (STATE, "_state_ref.py"),
    "kv_paged_copy_kernel": (STATE, "_state_ref.py"), "kv_adopt_kernel": (STATE, "_state_ref.py"), "decode_arm_kernel": (STATE, "_state_ref.py"),
    "decode_set_forced_kernel": (STATE, "_state_ref.py"), "decode_cancel_kernel": (STATE, "_state_ref.py"), "codes_to_i64_kernel": (STATE, "_state_ref.py"),
}

# kernels that take no data: nothing to compare with a reference
EXEMPT = {
    "group_probe_spin_kernel": "a timing probe: spins on the wall clock for a given number of ticks, reads and writes no memory",
    "group_probe_touch_kernel": "a timing probe: an empty kernel",
}


def kernels():
    """{kernel name: source file} of every __global__ DEFINITION (a declaration ends in ';' before any '{')"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(path).read()
        src = re.sub(r"//[^\n]*", "", src)
        for m in re.finditer(r"\b__global__\b", src):
            rest = src[m.end():]
            brace, semi = rest.find("{"), rest.find(";")
            assert brace >= 0, path
            if 0 <= semi < brace:
                continue
            names = [n for n in re.findall(r"\b(\w+)\s*\(", rest[:brace]) if n.endswith("_kernel")]
            assert names, f"{os.path.basename(path)}: a __global__ function whose name does not end in _kernel: {rest[:brace].strip()[:120]}"
            out[names[0]] = os.path.basename(path)
    return out


def test_the_parser_sees_the_kernels():
    ks = kernels()
    assert len(ks) >= 90
    for name, where in (("frame_begin_kernel", "decode_kernels.cuh"), ("audio_out_kernel", "audio_kernels.cuh"), ("conv_gemm_kernel", "codec_kernels.cuh"),
                        ("silu_mul_kernel", "codec_kernels.cuh"), ("text_scatter_kernel", "state_kernels.cuh"), ("prompt_rows_kernel", "prompt_kernels.cuh"),
                        ("group_probe_touch_kernel", "fq3_batch.hip"), ("rep_penalty_kernel", "fq3_api.hip")):
        assert ks.get(name) == where, (name, ks.get(name))


def test_every_kernel_has_a_reference_test():
    ks = kernels()
    missing = sorted(set(ks) - set(COVERAGE) - set(EXEMPT))
    assert not missing, f"kernels without a reference test (give them a kind in a probe, then a line in COVERAGE): {missing}"
    stale = sorted((set(COVERAGE) | set(EXEMPT)) - set(ks))
    assert not stale, f"entries for kernels that no longer exist: {stale}"
    assert not set(COVERAGE) & set(EXEMPT)
    bad = []
    for name, entry in COVERAGE.items():
        test, where = entry[0], entry[1]
        alias = entry[2] if len(entry) > 2 else None
        tp, wp = os.path.join(TESTS, test), os.path.join(TESTS, where)
        if not (test.startswith("test_gpu_") and os.path.exists(tp) and os.path.exists(wp)):
            bad.append(f"{name}: {test} / {where} does not exist")
            continue
        ttext, wtext = open(tp).read(), open(wp).read()
        if "pytest.mark.gpu" not in ttext:
            bad.append(f"{name}: {test} is not a GPU test")
        if where != test and not re.search(r"^\s*(import|from)\s+%s\b" % re.escape(where[:-3]), ttext, re.M):
            bad.append(f"{name}: {test} does not import {where}")
        tokens = [name, name[:-len("_kernel")]] + ([alias] if alias else [])
        if not any(re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(t), wtext) for t in tokens):
            bad.append(f"{name}: {where} names none of {tokens}")
    assert not bad, "\n".join(bad)


def test_exemptions_take_no_data():
    assert set(EXEMPT) == {"group_probe_spin_kernel", "group_probe_touch_kernel"}
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "fq3_batch.hip")).read())
    for name, reason in EXEMPT.items():
        assert len(reason) > 20
        sig = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert "*" not in sig, f"{name} takes a pointer: it has data, and needs a reference test"
