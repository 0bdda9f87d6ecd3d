"""CPU: the C-ABI library loads and exports every symbol include/fq3hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
HDR = os.path.join(ROOT, "include", "fq3hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def _declared():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fq3_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = _declared()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_table_matches_header():
    from fq3hip import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_abi_version_and_error_string(lib):
    lib.fq3_abi_version.restype = ctypes.c_int
    assert lib.fq3_abi_version() == 5
    lib.fq3_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.fq3_last_error(), bytes)


def test_null_arguments_are_errors_not_crashes(lib):
    # argument validation happens before any HIP call, so this is safe without a GPU
    lib.fq3_ctx_create.restype = ctypes.c_int
    assert lib.fq3_ctx_create(None, None) == -1
    lib.fq3_bind_weights.restype = ctypes.c_int
    assert lib.fq3_bind_weights(None, None) == -1
    lib.fq3_codec_create.restype = ctypes.c_int
    assert lib.fq3_codec_create(None, None) == -1
    lib.fq3_codec_num_samples.restype = ctypes.c_int64
    assert lib.fq3_codec_num_samples(None, 10) == -1
    # batched decode: lane validation precedes every device call
    h = ctypes.c_void_p()
    lanes = (ctypes.c_void_p * 2)(None, None)
    lib.fq3_batch_create.restype = ctypes.c_int
    assert lib.fq3_batch_create(None, 2, ctypes.byref(h)) == -1
    assert lib.fq3_batch_create(lanes, 129, ctypes.byref(h)) == -1         # more than eight 16-column MFMA token tiles
    assert lib.fq3_batch_create(lanes, 2, ctypes.byref(h)) == -3          # FQ3_ESTATE: lanes without bound weights
    assert lib.fq3_batch_frames(None, 1, None) == -1 and lib.fq3_batch_graph_capture(None, None) == -1
    assert lib.fq3_batch_size(None) == 0 and lib.fq3_batch_destroy(None) == 0


def test_q_dim_above_2048_is_refused(lib):
    """The split-KV merge prologue of the o_proj GEMV stages q_dim = n_heads * 128 <= 2048 elements (one 8-element slice per thread of
    its workgroup): a wider stack is refused when the context is created -- the dims check precedes every HIP call -- and says why."""
    from fq3hip import _lib as L

    def dims(n_heads, n_kv):
        return L.StackDims(hidden=1024, inter=3072, n_layers=1, n_heads=n_heads, n_kv_heads=n_kv, head_dim=128, vocab=2048, rms_eps=1e-6)
    lib.fq3_ctx_create.restype = ctypes.c_int
    lib.fq3_last_error.restype = ctypes.c_char_p
    for talker, predictor in ((dims(17, 17), dims(16, 8)), (dims(16, 8), dims(48, 12)), (dims(20, 5), dims(16, 8))):
        cfg = L.Config(dtype=L.FQ3_BF16, talker=talker, predictor=predictor, num_code_groups=16, max_seq_len=64, codec_eos_token_id=1,
                       has_projection=0, max_frames=8)
        h = ctypes.c_void_p()
        assert lib.fq3_ctx_create(ctypes.byref(cfg), ctypes.byref(h)) == L.FQ3_EUNSUPPORTED
        assert b"n_heads * 128 <= 2048" in lib.fq3_last_error() and not h.value


def test_struct_layout_matches_header_sizes():
    from fq3hip import _lib as L
    assert ctypes.sizeof(L.StackDims) == 32
    assert ctypes.sizeof(L.Config) == 4 + 32 + 32 + 5 * 4
    assert ctypes.sizeof(L.LayerWeights) == 8 * 8
    assert ctypes.sizeof(L.Sampling) == 20


def test_product_never_imports_oracle():
    """The shipped package must not reference oracle/ (only tests, smoke() and bench's cpu leg may)."""
    pkg = os.path.join(ROOT, "faster-qwen3-tts_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h")):
                txt = open(os.path.join(d, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(d, f)


def test_no_kernel_uses_scratch():
    """Every gfx950 kernel embedded in the built library has an EMPTY private segment: no register spills, no stack arrays (a
    spilling GEMV instantiation runs at a fraction of its bandwidth; the round-3 review listed five).  tools/check_scratch.py unbundles
    the code objects of libfq3hip.so and reads their AMDGPU metadata notes."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_scratch", os.path.join(root, "tools", "check_scratch.py"))
    cs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cs)
    if not os.path.exists(cs.READELF):
        import pytest
        pytest.skip("llvm-readelf not found")
    ks = cs.kernels(os.path.join(root, "faster-qwen3-tts_amd", "lib", "libfq3hip.so"))
    assert len(ks) > 300, len(ks)
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] > 0]
    assert not bad, bad


# kernels that may need more than 256 arch + accumulation VGPRs (one wave per SIMD): none of them is on a DEFAULT path
_OVER_256_ALLOWED = (
    (r"gemv_batch_kernel<", "VALU batch GEMVs: fp32 contexts (parity mode) and fq3_batch_set_option('mfma', 0)"),
    (r"gemv_kernel<float", "fp32 single-stream GEMV (parity mode)"),
    (r"attn_decode_lane_kernel<float", "fp32 lane attention (parity mode; bf16 is the product path)"),
    (r"attn_decode_lane_kernel<unsigned short, 4, 4>", "the 16-key steps (attn_lane_keys 16: measurement switch) at four q heads per kv head"),
    (r"resunit_kernel<unsigned short, 192", "the 192-channel fused residual unit (fuse_units 2: measured slower, off)"),
    (r"gemv_batch_mfma_norm_kernel<16, 2, 0, false>", "K = 2048 SwiGLU panel kernel with a runtime tile count: only with norm_skinny 0 above 64 lanes (measurement switch)"),
)


def test_no_default_path_kernel_needs_more_than_256_vgprs():
    """Occupancy (round-5 review, carried twice): a wave64 kernel above 256 arch + accumulation VGPRs runs one wave per SIMD.  Every kernel
    of a default path must fit; the exceptions are the named non-default instantiations above.  (Round 6: the 1.7B gate | up panel kernel
    of <= 32 lanes, gemv_batch_mfma_norm_kernel<16, SwiGLU, 1..4>, went from 276-294 to <= 256 by normalising its tokens in two rounds.)"""
    import importlib.util
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_scratch", os.path.join(root, "tools", "check_scratch.py"))
    cs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cs)
    if not os.path.exists(cs.READELF):
        import pytest
        pytest.skip("llvm-readelf not found")
    ks = [k for k in cs.kernels(os.path.join(root, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")) if k["vgpr"] + k["agpr"] > 256]
    names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in ks), capture_output=True, text=True).stdout.split("\n")
    bad = []
    for k, n in zip(ks, names):
        n = n.replace("fq3::", "").replace("(anonymous namespace)::", "").replace("void ", "")
        if not any(re.search(re.escape(pat) if "\\" not in pat else pat, n) for pat, _why in _OVER_256_ALLOWED):
            bad.append((n[:120], k["vgpr"], k["agpr"]))
    assert not bad, bad
