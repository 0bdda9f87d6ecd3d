"""CPU: the watermark scan's reference (tests/_mark_scan_ref.py) and the host half of ``fq3_mark_scan*``.

The two scan kernels of csrc/mark_kernels.cuh get their lines of the kernel census (tests/test_kernel_census_cpu.py) from here, as the
other three did from tests/test_watermark_cpu.py: their reference test is tests/test_gpu_mark_scan.py."""
import numpy as np
import pytest

import _mark_ref as R
import _mark_scan_ref as S
import test_kernel_census_cpu as census

census.COVERAGE.update({k: ("test_gpu_mark_scan.py", "test_gpu_mark_scan.py", "mark_kernels.cuh")
                        for k in ("mark_scan_blocks_kernel", "mark_scan_windows_kernel")})
KEY = 0x0123456789ABCDEF


@pytest.mark.parametrize("win,hop", [(4, 2), (3, 3), (1, 1)])
def test_window_count_is_the_formula(win, hop):
    from fq3hip import watermark as W
    for nb in (1, win - 1, win, win + 1, win + hop, win + hop + 1):
        if nb < 1:                                                          # win = 1: a clip the ABI accepts has at least one block
            continue
        want = 1 if nb <= win else 1 + -(-(nb - win) // hop)
        for n in (max(256 * (16 * (nb - 1) + 1) + 1, 512), 256 * (16 * nb + 1)):   # the shortest and the longest clip of nb blocks
            assert W.scan_windows(n, win, hop) == want == len(S.windows(nb, win, hop)), (nb, n)
    spans = S.windows(win + hop + 1, win, hop)
    assert spans[0] == (0, win) and spans[-1] == (hop + 1, win + hop + 1) and all(e - s == win for s, e in spans)


@pytest.mark.parametrize("n,win,hop", [(511, 4, 2), ((1 << 27) + 1, 4, 2), (4096, 0, 1), (4096, 4097, 1), (4096, 4, 0), (4096, 4, 5)])
def test_out_of_range_arguments_are_refused(n, win, hop):
    from fq3hip import watermark as W
    with pytest.raises(ValueError):
        W.scan_windows(n, win, hop)


def test_one_window_is_the_whole_clip_detector():
    y = R.embed(R.voiced(0.5), KEY, float(np.float32(0.1)))[:11000]
    z = S.scan_tables(y, KEY, 4, 2)
    assert z.shape == (1, 32, 128) and np.max(np.abs(z[0] - R.detect_table(y, KEY))) < 1e-12
