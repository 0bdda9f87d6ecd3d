"""CPU: every kernel of the single-stream decode frame is built with its leading arguments preloaded into user SGPRs
(csrc/decode_kernels.cuh "kernel entry"; the Makefile's KERNARG_PRELOAD).  tools/check_preload.py reads the preload length from the
kernel descriptors of the built library: for each frame kernel, bf16 and fp32, it must equal the dword count of the leading run of
plain pointers / 32-bit scalars of its signature -- the count the header states -- and stay within the 14 dwords gfx950 can deliver.
(That no kernel gained a private segment is tests/test_abi.py::test_no_kernel_uses_scratch.)"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
CSRC = os.path.join(ROOT, "faster-qwen3-tts_amd", "csrc")

# kernel family -> the constant beside its definition that states the dwords of its leading arguments
LEAD_CONSTANT = {
    "gemv_kernel": "kGemvLeadDwords",
    "attn_decode_kernel": "kAttnDecodeLeadDwords",
    "attn_pred_kernel": "kAttnPredLeadDwords",
    "frame_begin_kernel": "kFrameBeginLeadDwords",
    "embed_sum_kernel": "kEmbedSumLeadDwords",
    "sample_pred_wave_kernel": "kSamplePredLeadDwords",
    "sample_talker_wave_kernel": "kSampleTalkerLeadDwords",
}


def _tool():
    spec = importlib.util.spec_from_file_location("check_preload", os.path.join(ROOT, "tools", "check_preload.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return _tool().frame_kernels(LIB)


def _stated():
    src = open(os.path.join(CSRC, "decode_kernels.cuh")).read() + open(os.path.join(CSRC, "sampler_wave.cuh")).read()
    return {fam: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for fam, name in LEAD_CONSTANT.items()}


def test_signature_arithmetic():
    """the helper's own dword count: pointers 2 (8-byte aligned: a hole counts), scalars 1, the run ends at a struct or at 14"""
    cp = _tool()
    assert cp.leading_dwords("void fq3::k<float>(void const*, int, int, fq3::Tail)") == 4
    assert cp.leading_dwords("void fq3::k<float, 2>(fq3::Args)") == 0
    assert cp.leading_dwords("void fq3::k<unsigned short>(float*, int, float*, int)") == 7            # hole in front of the 2nd pointer
    assert cp.leading_dwords("void fq3::k<float>(%s, int, int, int)" % ", ".join(["int*"] * 6)) == 14     # the 3rd int no longer fits
    assert cp.leading_dwords("void fq3::k<float>(%s, int, float*)" % ", ".join(["int*"] * 6)) == 13       # a pointer needs 2 more


def test_every_frame_kernel_preloads_its_leading_arguments(rows):
    cp = _tool()
    stated = _stated()
    assert set(stated) == set(cp.FRAME_KERNELS)
    seen = set()
    for sig, fam, length, lead in rows:
        assert lead == stated[fam], (sig, lead, stated[fam])
        assert length == lead and 0 < length <= cp.MAX_DWORDS, (sig, length, lead)
        seen.add((fam, "unsigned short" in sig.split("(")[0], ))
    # bf16 and fp32 instantiations of every family are in the library
    assert seen == {(fam, b) for fam in cp.FRAME_KERNELS for b in (False, True)}, seen
    # every GEMV the frame can launch: prologue x epilogue pairs, the two-token pass (M = 2) and both rows-per-wave forms
    gemv = [sig for sig, fam, _l, _d in rows if fam == "gemv_kernel"]
    assert len(gemv) >= 200, len(gemv)
    assert any(re.search(r"gemv_kernel<unsigned short, \d+, 2, 1, (true|false), 2, 1>", s) for s in gemv)     # PRO_COMBINE, M = 2
