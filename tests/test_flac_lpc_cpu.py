"""CPU: the LPC reference (tests/_flac_lpc_ref.py) against its own decoder, the host-only half of fq3_flac_set_option, the
``flac_lpc`` encoding's validation, and the census lines of flac_encode_lpc_kernel and flac_encode_lpc_group_kernel
(csrc/flac_kernels.cuh), added to the table of tests/test_kernel_census_cpu.py from here as tests/test_flac_group_census_cpu.py adds
the group kernels'; their reference test is tests/test_gpu_flac_lpc.py."""
import numpy as np
import pytest

import _flac_lpc_ref as L
import _flac_ref as R
import test_flac_group_census_cpu  # noqa: F401  (and, through it, the earlier add-ons' lines)
import test_kernel_census_cpu as census
from fq3hip import _lib
from fq3hip import audio_out as ao

try:
    import test_join_group_census_cpu  # noqa: F401
except ImportError:
    pass

TEST = "test_gpu_flac_lpc.py"
LINES = {"flac_encode_lpc_kernel": (TEST, TEST, "flac_kernels.cuh"), "flac_encode_lpc_group_kernel": (TEST, TEST, "flac_kernels.cuh")}
census.COVERAGE.update(LINES)


def test_the_lpc_kernels_are_in_the_census():
    ks = census.kernels()
    for name, line in LINES.items():
        assert ks.get(name) == line[2] and census.COVERAGE.get(name) == line and name not in census.EXEMPT
    census.test_every_kernel_has_a_reference_test()


@pytest.mark.parametrize("M,block", [(8, 1152), (3, 100), (8, 64)])
def test_reference_round_trips(M, block):
    x = np.concatenate(list(L.signals(block + block // 2).values()) + [L.signals(70)["ar2"]])
    stats = []
    data = R.stream_header(24000, block, len(x)) + L.encode_frames(x, 24000, block, M, stats)
    assert np.array_equal(L.decode(data), x)
    assert {"constant", "verbatim", "lpc"} <= {s[0] for s in stats} and any(s[0] in ("fixed", "lpc") and s[2] > 0 for s in stats)
    assert L.encode_frames(x, 24000, block, 0) == R.encode_frames(x, 24000, block)
    with pytest.raises(R.FlacError):
        L.decode(data[:-1] + bytes([data[-1] ^ 1]))


def test_lpc_wins_on_a_resonance():
    """a condition on the rule, not a measurement: an AR(2) resonance is what a linear predictor is for"""
    x, stats = L.signals(4 * 1152)["ar2"], []
    lpc, fixed = L.encode_frames(x, 24000, 1152, 8, stats), R.encode_frames(x, 24000, 1152)
    assert any(s[0] == "lpc" for s in stats) and len(lpc) < len(fixed)
    assert len(L.encode_frames(x[:63], 24000, 1152, 8)) == len(R.encode_frames(x[:63], 24000, 1152))      # below 64 samples: fixed-only


def test_set_option_and_the_encoding_without_a_gpu():
    assert _lib.load().fq3_flac_set_option(None, b"lpc_order", 8) == _lib.FQ3_EINVAL
    s = ao.AudioOutSpec(8000, "flac_lpc")
    assert s.validate(24000) is s and ao.is_flac("flac_lpc") and ao.is_flac("flac") and not ao.is_flac("s16")
    assert ao.NUMPY_DTYPES["flac_lpc"] == np.uint8 and ao.FLAC_LPC_ORDERS == {"flac": 0, "flac_lpc": 8}
    with pytest.raises(ValueError):
        ao.AudioOutSpec(None, "flac_lpc").validate(100000)
    with pytest.raises(ValueError):
        ao.AudioOutSpec(None, "flac_lpc8")
