"""GPU: the FLAC stage with LPC subframes (flac_encode_lpc_kernel and flac_encode_lpc_group_kernel in csrc/flac_kernels.cuh, behind
fq3_flac_set_option "lpc_order").

Every comparison is exact: the device's bytes ARE the bytes of the reference encoder (tests/_flac_lpc_ref.py: the rule of
include/fq3hip.h in numpy, Levinson-Durbin in float64 scalars), its decoder turns them back into the input, and the group form is
held to single pushes with the guard-byte harness of tests/test_gpu_flac_group.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _flac_lpc_ref as L
import _flac_ref as R
import test_gpu_flac_group as G
from fq3hip import _lib
from fq3hip import audio_out as ao
from test_gpu_flac import _Stage

RATE = 24000
_cache = {}


def _stream(block, tail):
    """1.5 blocks of each signal -- a whole block of each, and blocks that straddle two (partition orders above 0) -- then ``tail`` samples"""
    key = (block, tail)
    if key not in _cache:
        x = np.concatenate(list(L.signals(block + block // 2).values()))
        _cache[key] = np.concatenate([x, x[:tail]])
        _cache[key].setflags(write=False)
    return _cache[key]


def _stage(block, M=None):
    st = _Stage(RATE, block)
    if M is not None:
        assert st.lib.fq3_flac_set_option(st.h, b"lpc_order", M) == 0, st.lib.fq3_last_error()
    return st


@pytest.mark.parametrize("block", [1152, 576, 100, 64])        # 100: only p <= 2 is legal; 64: the smallest block with LPC candidates
@pytest.mark.parametrize("M", [1, 4, 8])
def test_device_bytes_equal_the_reference_whatever_the_cut(M, block):
    """the last block has 40 samples (fixed-only) for M = 4 and 70 (LPC candidates; 6 at block 64) otherwise"""
    x = _stream(block, 40 if M == 4 else 70)
    xd = torch.from_numpy(x.copy()).cuda()
    stats = []
    want = L.encode_frames(x, RATE, block, M, stats)
    kinds = {s[0] for s in stats}
    assert {"lpc", "constant", "verbatim"} <= kinds and max(s[1] for s in stats if s[0] == "lpc") <= M, stats
    got = _stage(block, M).push(xd, final=True).tobytes()
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1)
        raise AssertionError(f"{len(got)} bytes, reference {len(want)}; first difference at byte {at}; choices {stats}")
    assert np.array_equal(L.decode(R.stream_header(RATE, block, len(x)) + got), x)
    st, c = _stage(block, M), [block // 3, block // 3, 3 * block + 7, len(x) - 5]      # an empty push, a cut inside a block
    parts = [st.push(xd[a:b]) for a, b in zip([0] + c, c)] + [st.push(xd[c[-1]:]), st.push(xd[:0], final=True)]
    assert b"".join(p.tobytes() for p in parts) == want


def test_order_0_is_the_fixed_stage_and_the_option_keeps_its_contract():
    x = _stream(576, 70)
    xd = torch.from_numpy(x.copy()).cuda()
    want = R.encode_frames(x, RATE, 576)
    for M in (None, 0):
        assert _stage(576, M).push(xd, final=True).tobytes() == want
    st = _stage(576, 8)
    first = st.push(xd[:1000]).tobytes()
    assert st.lib.fq3_flac_set_option(st.h, b"lpc_order", 0) == _lib.FQ3_ESTATE          # the utterance has begun
    assert first + st.push(xd[1000:], final=True).tobytes() == L.encode_frames(x, RATE, 576, 8)
    st.reset()                                                                         # the option survives, and may change again
    assert st.push(xd, final=True).tobytes() == L.encode_frames(x, RATE, 576, 8)
    st.reset()
    assert st.lib.fq3_flac_set_option(st.h, b"lpc_order", 9) == _lib.FQ3_EINVAL
    assert st.lib.fq3_flac_set_option(st.h, b"lpc_order", 0) == 0 and st.push(xd, final=True).tobytes() == want


def _objs(n, block, M):
    objs = G._objs(n, RATE, block)
    for o, m in zip(objs, M if isinstance(M, list) else [M] * n):
        assert o.lib.fq3_flac_set_option(o.h, b"lpc_order", m) == 0
    return objs


def test_group_rows_equal_their_single_pushes():
    """four rows of unequal length in one fq3_flac_push_group against twins that see single pushes: bytes, counts, guards, and the
    next push (the objects' state); the rows' streams against the reference"""
    block, x = 64, _stream(64, 70)
    lens = [0, 200, 333, len(x)]
    dev = [torch.from_numpy(np.roll(x, -17 * b)[:n].copy()).cuda() for b, n in enumerate(lens)]
    objs, twins = _objs(4, block, 8), _objs(4, block, 8)
    a = G._both(objs, twins, [d[: n // 2] for d, n in zip(dev, lens)], [False] * 4)
    z = G._both(objs, twins, [d[n // 2:] for d, n in zip(dev, lens)], [True] * 4)
    for b, n in enumerate(lens):
        assert a[b] + z[b] == L.encode_frames(np.roll(x, -17 * b)[:n], RATE, block, 8), b
    # rows of different lpc_order: FQ3_EINVAL, nothing launched
    mixed = _objs(2, block, [8, 4])
    buf = torch.full((2 * 256,), G.GUARD, dtype=torch.uint8, device="cuda")
    nb = torch.full((2,), G.UNSET, dtype=torch.int64, device="cuda")
    rc, got = G._raw_group(mixed, [dev[1][:64]] * 2, [False] * 2, [buf.data_ptr(), buf.data_ptr() + 256], [256] * 2,
                           [nb.data_ptr(), nb.data_ptr() + 8])
    torch.cuda.synchronize()
    assert rc == _lib.FQ3_EINVAL and b"lpc_order" in _lib.load().fq3_last_error() and got == [G.UNSET] * 2
    assert bool((buf == G.GUARD).all()) and bool((nb == G.UNSET).all())


def test_audio_out_flac_lpc():
    """AudioOut("flac_lpc") from float PCM, cut into pushes: decodes to the s16 stage's samples, in fewer bytes than "flac"; a group of
    flac and flac_lpc stages goes through one bucket each"""
    rng = np.random.default_rng(5)
    t = np.arange(9000) / 24000.0
    pcm = (0.4 * np.sin(2 * np.pi * 220.0 * t) * np.hanning(9000) + 0.01 * rng.standard_normal(9000)).astype(np.float32)
    pd = torch.from_numpy(pcm).cuda()
    s16 = ao.AudioOut(ao.AudioOutSpec(None, "s16"), 24000, "cuda").push(pd, final=True).cpu().numpy()
    st = ao.AudioOut(ao.AudioOutSpec(None, "flac_lpc"), 24000, "cuda")
    body = b"".join(p.cpu().numpy().tobytes() for p in (st.push(pd[:100]), st.push(pd[100:5000]), st.push(pd[5000:], final=True)))
    assert st.n_out == len(body) and np.array_equal(L.decode(st.header() + body), s16)
    plain = ao.AudioOut(ao.AudioOutSpec(None, "flac"), 24000, "cuda").push_host(pd, final=True)
    assert len(body) < len(plain)
    specs = [ao.AudioOutSpec(None, e) for e in ("flac_lpc", "flac", "flac_lpc", "flac")]
    got = ao.push_group_host([ao.AudioOut(s, 24000, "cuda") for s in specs], [pd] * 4, [True] * 4)
    assert got[0].tobytes() == got[2].tobytes() == body and got[1].tobytes() == got[3].tobytes() == plain.tobytes()
