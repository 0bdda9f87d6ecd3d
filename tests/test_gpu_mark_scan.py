"""GPU: the watermark scan (mark_scan_blocks_kernel and mark_scan_windows_kernel of csrc/mark_kernels.cuh, behind fq3_mark_scan;
DESIGN.md section 4.23) against the float64 reference tests/_mark_scan_ref.py.  The signals are marked by the float64 reference embed
on the CPU, so nothing here leans on the device embed.  The table bound is the rule of tests/test_gpu_watermark.py: 4 x the largest
deviation of the same formulas in numpy float32 from the float64 reference on the case's own input, with a floor of 2^-20 (an ulp of
a float32 z of the size seen here)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mark_ref as R
import _mark_scan_ref as S
from fq3hip import _lib
from fq3hip import watermark as W

KEY, A = 0x0123456789ABCDEF, float(np.float32(0.1))
_state = {}


def _marked(seconds, a=None, b=None):
    """`seconds` of the voiced signal, marked by the reference in [a, b) (all of it by default); computed once, never changed"""
    if (seconds, a, b) not in _state:
        x = R.voiced(seconds)
        a0, b0 = (0, len(x)) if a is None else (a, b)
        y = x.astype(np.float64)
        y[a0:b0] = R.embed(x[a0:b0], KEY, A)
        _state[(seconds, a, b)] = y.astype(np.float32)
    return _state[(seconds, a, b)]


def _bits(s):
    return [np.asarray(v).view(np.uint32) for v in (s.z, s.offset, s.phase, s.tables.cpu().numpy())]


# NB = 1, 3 (not a multiple of 256), 4 (whole blocks: the last block is closed by a tile of its own), 5 (a last block of two frames), 7
@pytest.mark.parametrize("n", [2000, 11000, 16640, 17000, 28900])
def test_tables_and_verdicts_against_the_reference(n):
    r = _marked(1.25)[:n]
    ref = S.scan_tables(r, KEY, 4, 2)
    bound = max(4.0 * float(np.max(np.abs(S.scan_tables(r, KEY, 4, 2, np.float32) - ref))), 2.0 ** -20)
    out, tab, ws = W.scan_blocks_device([torch.from_numpy(r).cuda()], [KEY], 4, 2, tables=True)
    z, rec = tab.cpu().numpy(), out.cpu().numpy().view(W._WINDOW)
    err = float(np.max(np.abs(z.astype(np.float64) - ref)))
    print(f"scan n={n}: W = {ws[0]}, max |device - ref64| = {err:.3e}, bound = {bound:.3e}, max z = {z.max():.3f}")
    # Measured: 1.49e-5 against 1.60e-5 (n = 2000, the thinnest), 2.05e-5 / 2.98e-5, 1.79e-5 / 2.98e-5, 2.05e-5 / 3.11e-5, 1.94e-5 / 3.11e-5.
    # As in test_gpu_watermark.py the error follows the forward product's summation order (four chains, as mark_forward).
    assert ws == [len(ref)] and z.shape == ref.shape and err < bound
    for w in range(len(ref)):                                                # the verdict is the argmax of the device's own table
        oi, ph = np.unravel_index(int(np.argmax(z[w])), z[w].shape)
        assert (rec["z"][w], rec["offset"][w], rec["phase"][w], rec["present"][w]) == (z[w, oi, ph], 8 * oi, ph, int(z[w, oi, ph] >= 6.0))


def test_rows_are_independent():
    """Three clips of different lengths under two keys in one call equal the same clips alone, bit for bit -- and the call cuts its
    grid differently each time (36 s alone: ranges of 4 blocks x 2 offsets; the short clips alone: 2 x 1; together: 4 x 4), so this
    also pins that no result depends on the cut."""
    clips = [np.tile(_marked(9.0, 72000, 168000), 4), _marked(9.0, 72000, 168000), _marked(1.25)[:28900]]
    keys = [KEY, KEY + 1, KEY]
    together = W.scan(clips, 24000, keys, tables=True)
    for clip, key, got in zip(clips, keys, together):
        alone = W.scan(clip, 24000, key, tables=True)
        assert len(alone.z) == W.scan_windows(len(clip), 18, 6)
        assert all(np.array_equal(p, q) for p, q in zip(_bits(got), _bits(alone)))


@pytest.mark.parametrize("seconds,a,b,inside,outside", [(9.0, 72000, 168000, 1, 0), (12.0, 84000, 196608, 2, 3)])
def test_localisation(seconds, a, b, inside, outside):
    """Default windows (3 s / 1 s = 18 / 6 blocks).  9 s marked in [3 s, 7 s): one window lies wholly inside the span and none wholly
    outside it (window 0 ends at 3.072 s).  12 s marked in [3.5 s, 8.192 s) adds the outside: windows 0, 8 and 9.  The float64
    reference alone (CPU) reads 12.84 inside for the first clip; 10.85 and 12.68 inside, at most 3.74 outside for the second (its
    straddling windows: 3.03 .. 9.75)."""
    s = W.scan(_marked(seconds, a, b), 24000, KEY)
    lo, hi = np.round(s.start_s * 24000), np.round(s.end_s * 24000)
    is_in, is_out = (lo >= a) & (hi <= b), (hi <= a) | (lo >= b)
    print(f"{seconds} s: z = {np.round(s.z, 3).tolist()}, inside {is_in.tolist()}, outside {is_out.tolist()}")
    assert (s.window_s, s.hop_s) == (18 * 4096 / 24000, 6 * 4096 / 24000)
    assert (int(is_in.sum()), int(is_out.sum())) == (inside, outside)
    assert s.present[is_in].all() and not s.present[is_out].any()


@pytest.mark.parametrize("case", ["33 rows", "a length of 511", "a null row"])
def test_errors_write_nothing(case):
    lib = _lib.load()
    x = torch.from_numpy(_marked(1.25)[:17000]).cuda()
    B = 33 if case == "33 rows" else 2
    ns = (C.c_int64 * B)(*[511 if case == "a length of 511" and b == 1 else 17000 for b in range(B)])
    ptrs = (C.c_void_p * B)(*[None if case == "a null row" and b == 1 else x.data_ptr() for b in range(B)])
    keys = (C.c_uint64 * B)(*[KEY] * B)
    work = torch.zeros(2 * 5 * (32 * 128 + 32), dtype=torch.float64, device="cuda")
    out = torch.full((2 * 2 * 16,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = lib.fq3_mark_scan(B, ptrs, ns, keys, 4, 2, C.c_void_p(work.data_ptr()), work.numel(), C.c_void_p(out.data_ptr()), None,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.FQ3_EINVAL and bool((out == 0x5A).all()) and not bool(work.any())
