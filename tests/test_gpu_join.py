"""GPU: the segment join stage (csrc/join_kernels.cuh behind fq3_join_*) against the NumPy reference
(tests/_join_ref.py), bit for bit -- the arithmetic is comparisons and copies, so no tolerance applies -- for every way of cutting
the stream into pushes, at an odd output offset, chained into ``AudioOut``; and its state errors."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _join_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao
from fq3hip.long_form import SegmentJoin

RATE, H = 24000, 240
THR, LEAD, TAIL, HOLD = 0.25, 1, 2, 4
PAUSES = (0, 1, 2400)


def _tone(n, seed):
    rng = np.random.default_rng(seed)
    s = np.sign(rng.standard_normal(n))
    return (s * rng.uniform(0.3, 0.9, n)).astype(np.float32)          # every sample active


def _quiet(n, seed):
    return np.random.default_rng(seed).uniform(-0.2, 0.2, n).astype(np.float32)      # every sample below the threshold, not zero


def _segment(parts, seed=0):
    """parts: [('t' | 'q', samples), ...]"""
    return np.concatenate([(_tone if k == "t" else _quiet)(n, seed + i) for i, (k, n) in enumerate(parts)] or [np.zeros(0, np.float32)])


def _streams(h=H):
    """name -> three segments (1 000 .. 6 000 samples at H = 240) that reach every branch with hold 4, tail 2, lead 1"""
    at = _quiet(2 * h, 90)
    at[h + 7] = np.float32(THR)                                     # exactly at the threshold: active
    return {
        # silence-tone-silence | all silent (nothing, no pause) | no silence at all
        "basic": [_segment([("q", 5 * h), ("t", 6 * h), ("q", 7 * h)], 1), _segment([("q", 9 * h + 17)], 2), _segment([("t", 5 * h + 100)], 3)],
        # trailing silence shorter than / equal to / longer than tail_hops
        "tail": [_segment([("t", 4 * h), ("q", 1 * h)], 4), _segment([("q", h), ("t", 3 * h), ("q", 2 * h)], 5),
                 _segment([("t", 3 * h), ("q", 3 * h + 50)], 6)],
        # trailing silence equal to / longer than hold_hops, far longer
        "hold": [_segment([("t", 2 * h), ("q", 4 * h)], 7), _segment([("t", 2 * h), ("q", 5 * h)], 8), _segment([("t", 2 * h), ("q", 20 * h + 3)], 9)],
        # an internal silence of hold_hops + 3 hops comes out whole | a sample exactly at the threshold | a short last hop that is active
        "inner": [_segment([("q", 3 * h), ("t", 2 * h), ("q", (HOLD + 3) * h), ("t", 2 * h), ("q", 6 * h)], 10), at,
                  _segment([("q", 4 * h), ("t", h + 31)], 11)],
        # short last hops that are silent, a segment shorter than a hop, pre-roll shorter than lead_hops
        "short": [_segment([("t", 4 * h), ("q", 2 * h + 1)], 12), _segment([("t", 100)], 13) if h > 100 else _segment([("t", h // 2)], 13),
                  _segment([("q", h // 2), ("t", 4 * h), ("q", 239 if h == 240 else h - 1)], 14)],
    }


def _cuts(name, n, seed):
    """the push lengths of a segment of n samples"""
    if name == "whole":
        return [n]
    if name.startswith("fixed"):
        step = int(name[5:])
        return [min(step, n - i) for i in range(0, n, step)] or [0]
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left > 0:
        k = int(min(left, rng.integers(1, 1500)))
        out.append(k)
        left -= k
    return out or [0]


def _run(join, segs, pauses, cut, pad=0, empties=False):
    """Pushes the stream cut as ``cut`` says -> host array.  ``pad``: the output starts that many floats into its buffer."""
    got = []
    n_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    for k, x in enumerate(segs):
        xd = torch.from_numpy(x).cuda()
        end_k = 2 if k == len(segs) - 1 else 1
        lens = _cuts(cut, len(x), 100 + k)
        pushes, pos = [], 0
        for i, n in enumerate(lens):
            pushes.append((xd[pos: pos + n], end_k if i == len(lens) - 1 and not empties else 0))
            pos += n
        if empties:
            pushes.insert(len(pushes) // 2, (xd[:0], 0))           # an empty push inside the segment ...
            pushes.append((xd[:0], end_k))                         # ... and one that ends it (end 1, and end 2 on the last segment)
        for p, end in pushes:
            pause = pauses[k] if end == 1 else 0
            cap = join.bound(p.numel(), pause)
            buf = torch.full((pad + cap + 4,), -7.0, dtype=torch.float32, device="cuda")
            join.push_into(p, end, pause, buf[pad: pad + cap], n_dev)
            n = int(n_dev.item())
            assert 0 <= n <= cap
            host = buf.cpu().numpy()
            assert (host[:pad] == -7.0).all() and (host[pad + n:] == -7.0).all()       # nothing outside [0, n) was written
            got.append(host[pad: pad + n])
    return np.concatenate(got)


def _want(segs, pauses, rate=RATE):
    return R.join(list(zip(segs, pauses)), rate, THR, LEAD, TAIL, HOLD)


@pytest.mark.parametrize("cut", ["whole", "fixed1920", "fixed239", "fixed240", "fixed241", "random"])
def test_join_matches_reference_for_every_cut(cut):
    for name, segs in _streams().items():
        join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
        got = _run(join, segs, PAUSES, cut)
        want = _want(segs, PAUSES)
        assert want.size > 0 and np.array_equal(got, want), (name, cut, got.size, want.size)


def test_single_sample_pushes():
    segs = _streams()["basic"]
    segs = [segs[0][4 * H + 200: 6 * H + 5], segs[1][:H + 3], segs[2][:2 * H + 1]]      # short: one launch per sample
    join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
    assert np.array_equal(_run(join, segs, PAUSES, "fixed1"), _want(segs, PAUSES))


def test_empty_pushes_with_each_end_value():
    for name, segs in _streams().items():
        join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
        assert np.array_equal(_run(join, segs, PAUSES, "fixed1920", empties=True), _want(segs, PAUSES)), name


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_output_at_an_odd_float_offset(pad):
    segs = _streams()["inner"]
    for cut in ("whole", "fixed241"):
        join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
        assert np.array_equal(_run(join, segs, PAUSES, cut, pad=pad), _want(segs, PAUSES))


@pytest.mark.parametrize("rate", [8000, 48000])
def test_other_rates(rate):
    h = rate // 100
    segs = _streams(h)["inner"]
    join = SegmentJoin(rate, "cuda", THR, LEAD, TAIL, HOLD)
    for cut in ("whole", "random"):
        join.reset()
        assert np.array_equal(_run(join, segs, PAUSES, cut), _want(segs, PAUSES, rate)), (rate, cut)


def test_more_than_one_round_of_hops():
    """a push of more hops than one round of the workgroup takes (256), with a queue that straddles the rounds"""
    seg = _segment([("q", 250 * H), ("t", 3 * H), ("q", 3 * H), ("t", 260 * H + 9), ("q", 300 * H)], 40)
    segs = [seg, _segment([("t", 2 * H)], 41)]
    join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
    assert np.array_equal(_run(join, segs, (2400, 0), "whole"), _want(segs, (2400, 0)))


def test_push_and_push_host():
    segs, want = _streams()["tail"], _want(_streams()["tail"], PAUSES)
    a = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
    dev = [a.push(torch.from_numpy(x).cuda(), 2 if k == 2 else 1, PAUSES[k]) for k, x in enumerate(segs)]
    assert np.array_equal(torch.cat(dev).cpu().numpy(), want) and a.n_out == want.size and a.finished
    b = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
    host = [b.push_host(torch.from_numpy(x).cuda(), 2 if k == 2 else 1, PAUSES[k]) for k, x in enumerate(segs)]
    assert np.array_equal(np.concatenate(host), want)


def test_state_errors():
    lib = _lib.load()
    segs = _streams()["basic"]
    want = _want(segs, PAUSES)
    join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
    n_dev = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    x0 = torch.from_numpy(segs[0]).cuda()
    first = join.push(x0[:2000])
    # capacity below the bound: FQ3_EINVAL, nothing launched
    cap = join.bound(x0.numel() - 2000, PAUSES[0])
    assert cap == R.bound(RATE, LEAD, HOLD, x0.numel() - 2000, PAUSES[0])
    buf = torch.full((cap + 8,), -3.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.Fq3Error) as e:
        join.push_into(x0[2000:], 1, PAUSES[0], buf[:cap - 1], n_dev)
    assert e.value.code == _lib.FQ3_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == -3.0).all()) and int(n_dev.item()) == -5
    # ... and the stream goes on as if that call had not been made
    rest = [join.push(x0[2000:], 1, PAUSES[0]), join.push(torch.from_numpy(segs[1]).cuda(), 1, PAUSES[1]),
            join.push(torch.from_numpy(segs[2]).cuda(), 2, 0)]
    assert np.array_equal(torch.cat([first] + rest).cpu().numpy(), want)
    # a push after end == 2
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.fq3_join_push(join._h, C.c_void_p(x0.data_ptr()), 10, 0, 0, C.c_void_p(buf.data_ptr()), buf.numel(),
                           C.c_void_p(n_dev.data_ptr()), C.c_void_p(s))
    assert rc == _lib.FQ3_ESTATE
    with pytest.raises(_lib.Fq3Error) as e:
        join.push(x0[:10])
    assert e.value.code == _lib.FQ3_ESTATE
    # reset starts a new stream
    join.reset()
    again = _run(join, segs, PAUSES, "fixed1920")
    assert np.array_equal(again, want)


def test_chain_into_audio_out_flac():
    """join -> AudioOut (speed 1.25, 16 kHz, flac) == the same AudioOut fed the reference's joined array in one push, byte for byte"""
    segs = _streams()["inner"]
    want_pcm = _want(segs, PAUSES)
    spec = ao.AudioOutSpec(16000, "flac", speed=1.25)
    ref = ao.AudioOut(spec, RATE, "cuda")
    want = ref.push(torch.from_numpy(want_pcm).cuda(), final=True).cpu().numpy()
    join = SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD)
    chain = ao.AudioOut(spec, RATE, "cuda")
    got = []
    for k, x in enumerate(segs):
        xd = torch.from_numpy(x).cuda()
        end_k = 2 if k == 2 else 1
        for i in range(0, len(x), 1920):
            last = i + 1920 >= len(x)
            y = join.push(xd[i: i + 1920], end_k if last else 0, PAUSES[k] if last else 0)
            got.append(chain.push(y, final=last and end_k == 2).cpu().numpy())
    got = np.concatenate(got)
    assert want.size > 100 and got.dtype == np.uint8 and np.array_equal(got, want)
    assert chain.header() == ref.header()
