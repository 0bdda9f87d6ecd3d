"""CPU: the watermark's reference (tests/_mark_ref.py) and the host half of ``fq3_mark_*``.

The three kernels of csrc/mark_kernels.cuh get their lines of the kernel census (tests/test_kernel_census_cpu.py) from here, as the
limiter's did from tests/test_limiter_census_cpu.py: their reference test is tests/test_gpu_watermark.py."""
import re

import numpy as np
import pytest

import _mark_ref as R
import _noise_ref
import test_kernel_census_cpu as census
from test_abi import HDR

census.COVERAGE.update({k: ("test_gpu_watermark.py", "test_gpu_watermark.py", "mark_kernels.cuh")
                        for k in ("mark_embed_kernel", "mark_detect_kernel", "mark_reduce_kernel")})
KEY = 0x0123456789ABCDEF


def test_chip_rows_are_the_philox_words():
    from fq3hip import watermark as W
    w = _noise_ref.words(KEY, 0, 0xFFFFFFFE, 256)
    c = R.chips(KEY)
    assert c.shape == (128, 64) and set(np.unique(c)) == {-1.0, 1.0} and abs(c.mean()) < 0.05
    for p, j in ((0, 0), (0, 31), (0, 32), (1, 63), (77, 40), (127, 5)):
        assert c[p, j] == (1.0 if (int(w[2 * p + (j >> 5)]) >> (j & 31)) & 1 else -1.0)
    a, lib_chips = W.design(KEY, 0.1)                                       # the library's host generator hands out the same rows
    assert a == np.float32(0.1) and np.array_equal(lib_chips, c)
    for n, final, want in ((0, 0, 0), (511, 0, 0), (512, 0, 256), (1023, 0, 512), (1000, 1, 1000)):
        assert W.count(n, bool(final)) == want
    with pytest.raises(ValueError):
        W.design(KEY, 0.5)


def test_zero_strength_is_the_identity():
    x = R.voiced(0.25)
    assert np.array_equal(R.embed(x, KEY, 0.0), x.astype(np.float64))
    assert np.array_equal(R.embed(x, KEY, 0.0, np.float32), x)


def test_reference_detects_its_mark_and_nothing_else():
    x = R.voiced(3.0)
    y = R.embed(x, KEY, float(np.float32(0.1)))
    s16 = np.round(y * 32767.0) / 32767.0
    z, _o, _ph, present = R.verdict(R.detect_table(s16, KEY))
    assert present and z >= 6.0 and len(y) == len(x)
    assert not R.verdict(R.detect_table(x, KEY))[3]
    assert not R.verdict(R.detect_table(s16, KEY + 1))[3]


def test_the_header_declares_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in ("design", "count", "create", "destroy", "reset", "push", "detect", "detect_workspace"):
        assert re.search(r"\bfq3_mark_%s\s*\(" % name, src), name
