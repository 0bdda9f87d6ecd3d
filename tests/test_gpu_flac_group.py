"""GPU: the FLAC stage for a group of streams (fq3_flac_push_group: flac_encode_group_kernel and flac_gather_group_kernel in
csrc/flac_kernels.cuh).

Two yardsticks, both exact.  (1) A twin set of objects driven by single pushes (fq3_flac_push, itself pinned to the reference encoder by
tests/test_gpu_flac.py) with the same cuts: the group call's bytes, frame counts, device byte counts and the bytes AROUND its rows (a
guard pattern) are the twins', and so is what the next push gives -- which is how the objects' state is compared.  (2) The reference
encoder of tests/_flac_ref.py: a row's pushes, concatenated, are its frames of the row's whole stream.

Every row of a call lies in ONE buffer between guard bytes, so a write outside a row's frames shows in the comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _flac_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao

GUARD, UNSET = 0xA5, -7


class _Obj:
    """one fq3_flac object and the samples its stream has taken"""

    def __init__(self, rate, block):
        self.lib, self.rate, self.block, self.bound = _lib.load(), rate, block, 2 * block + 18
        self.h = C.c_void_p()
        cfg = _lib.FlacConfig(rate, block)
        assert self.lib.fq3_flac_create(C.byref(cfg), C.byref(self.h)) == 0, self.lib.fq3_last_error()
        self.n_in = 0

    def __del__(self):
        self.lib.fq3_flac_destroy(self.h)

    def frames(self, n, final):
        count = lambda m, f: self.lib.fq3_flac_count(self.rate, self.block, m, 1 if f else 0)
        return count(self.n_in + n, final) - count(self.n_in, False)


def _objs(n, rate, block):
    return [_Obj(rate, block) for _ in range(n)]


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _raw_group(objs, xs, finals, outs, caps, nbs):
    """fq3_flac_push_group on the current stream -> (code, the rows' frame counts)"""
    B = len(objs)
    got = (C.c_int64 * B)(*([UNSET] * B))
    rc = _lib.load().fq3_flac_push_group(
        (C.c_void_p * B)(*[o.h.value for o in objs]), B, (C.c_void_p * B)(*[_ptr(x) for x in xs]), (C.c_int64 * B)(*[x.numel() for x in xs]),
        (C.c_int * B)(*[int(f) for f in finals]), (C.c_void_p * B)(*outs), (C.c_int64 * B)(*caps), got, (C.c_void_p * B)(*nbs),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, list(got)


def _raw_single(o, x, final, out, cap, nb):
    got = C.c_int64(UNSET)
    rc = o.lib.fq3_flac_push(o.h, C.c_void_p(_ptr(x)), x.numel(), int(final), C.c_void_p(out), cap, C.byref(got), C.c_void_p(nb),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, got.value


def _push(objs, xs, finals, group=(), odd=False):
    """One push per object: the rows listed in ``group``, in that order, through ONE fq3_flac_push_group, the others through single pushes.
    Row b's frames go to a span of one buffer whatever path it takes (``odd``: at an odd byte offset), its byte count to nb[b].
    -> (the buffer, the byte counts, the frame counts, the spans) on the host."""
    spans, cursor = [], 1
    for o, x, f in zip(objs, xs, finals):
        cap = o.frames(x.numel(), f) * o.bound
        cursor += 5
        cursor = cursor | 1 if odd else (cursor + 7) // 8 * 8
        spans.append((cursor, cap))
        cursor += cap
    buf = torch.full((cursor + 16,), GUARD, dtype=torch.uint8, device="cuda")
    nb = torch.full((len(objs),), UNSET, dtype=torch.int64, device="cuda")
    out = lambda b: buf.data_ptr() + spans[b][0] if spans[b][1] else None
    frames = [None] * len(objs)
    group = list(group)
    if group:
        rc, got = _raw_group([objs[b] for b in group], [xs[b] for b in group], [finals[b] for b in group], [out(b) for b in group],
                             [spans[b][1] for b in group], [nb.data_ptr() + 8 * b for b in group])
        assert rc == 0, _lib.load().fq3_last_error()
        for b, n in zip(group, got):
            frames[b] = n
    for b, o in enumerate(objs):
        if b not in group:
            rc, frames[b] = _raw_single(o, xs[b], finals[b], out(b), spans[b][1], nb.data_ptr() + 8 * b)
            assert rc == 0, o.lib.fq3_last_error()
    for o, x in zip(objs, xs):
        o.n_in += x.numel()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), nb.cpu().numpy(), frames, spans


def _same(got, want):
    """the group's push against the twins': everything equal, the counts those the host can predict, the guards intact -> the rows' bytes"""
    (gb, gn, gf, spans), (wb, wn, wf, _) = got, want
    assert gf == wf
    assert np.array_equal(gn, wn), (gn, wn)
    untouched = np.ones(len(gb), dtype=bool)
    for (off, cap), n in zip(spans, gn):
        assert 0 <= n <= cap
        untouched[off: off + n] = False
    assert np.all(gb[untouched] == GUARD)
    assert np.array_equal(gb, wb)
    return [gb[off: off + n].tobytes() for (off, _), n in zip(spans, gn)]


def _both(objs, twins, xs, finals, group=None, odd=False):
    """a push on the objects (``group``: default all rows) and the same push, all single, on the twins"""
    want_frames = [o.frames(x.numel(), f) for o, x, f in zip(objs, xs, finals)]
    got = _push(objs, xs, finals, range(len(objs)) if group is None else group, odd)
    assert got[2] == want_frames
    return _same(got, _push(twins, xs, finals, (), odd))


def _signal(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full(n, -1234, dtype=np.int16)
    if kind == "noise":                                        # full scale and white: no predictor gets below 16 bits a sample
        return rng.integers(-32768, 32768, n).astype(np.int16)
    i = np.arange(n)
    x = np.where((i // 8) % 2 == 0, 150.0, 12000.0) * np.sin(2 * np.pi * i / 40.0)      # smooth, loud and soft by turns of 8 samples
    if kind != "sine":
        x = x + rng.integers(-40, 41, n)
    return np.round(x).astype(np.int16)


KINDS = ("constant", "noise", "sine", "empty", "tail_only", "final_short", "final_flush", "final_nothing")


def _plan(kind, block):
    """(samples of the first push, samples of the second push, the second push is final)"""
    return {"constant": (5, 3 * block, False), "noise": (block + 7, 2 * block + 1, False), "sine": (2, 4 * block - 2, False),
            "empty": (block + 3, 0, False),                    # n_in == 0
            "tail_only": (3, 5, False),                        # completes no frame, moves its tail
            "final_short": (2, 2 * block + 3, True),           # the last frame has 5 samples
            "final_flush": (block + 4, block - 4, True),       # final, and the samples end on a block: nothing is left over
            "final_nothing": (block, 0, True)}[kind]           # final with an empty tail and no samples: no frame at all


# ---- 1. every kind of row in one call, against the twins and the reference encoder -------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("rate", [8000, 24000])
@pytest.mark.parametrize("block", [16, 64])
def test_rows_of_every_kind(block, rate, B):
    """Three group calls per set of rows: the first leaves every row a tail of its own length, the second is the row's kind, the
    third ends the rows that go on (another membership).  B < 8: as many sets as it takes to see every kind at this B."""
    for shift in range(0, len(KINDS), B) if B < len(KINDS) else (0,):
        kinds = [KINDS[(shift + b) % len(KINDS)] for b in range(B)]
        plans = [_plan(k, block) for k in kinds]
        tails = [9 if b % 2 else 0 for b in range(B)]           # the third push: some samples and the end, or only the end
        streams = [_signal(k if k in ("constant", "noise", "sine") else "mixed", p[0] + p[1] + t, 100 * shift + b)
                   for b, (k, p, t) in enumerate(zip(kinds, plans, tails))]
        dev = [torch.from_numpy(s).cuda() for s in streams]
        objs, twins = _objs(B, rate, block), _objs(B, rate, block)
        parts = [[] for _ in range(B)]
        first = _both(objs, twins, [d[:p[0]] for d, p in zip(dev, plans)], [False] * B)
        second = _both(objs, twins, [d[p[0]: p[0] + p[1]] for d, p in zip(dev, plans)], [p[2] for p in plans])
        for b in range(B):
            parts[b] += [first[b], second[b]]
        assert all(len(second[b]) == 0 for b in range(B) if kinds[b] in ("empty", "tail_only", "final_nothing"))
        live = [b for b in range(B) if not plans[b][2]]
        if live:
            third = _both([objs[b] for b in live], [twins[b] for b in live], [dev[b][plans[b][0] + plans[b][1]:] for b in live], [True] * len(live))
            for b, got in zip(live, third):
                parts[b].append(got)
        for b in range(min(B, len(KINDS))):                     # one row of every kind against the reference encoder
            x = streams[b] if not plans[b][2] else streams[b][:plans[b][0] + plans[b][1]]
            stats = []
            assert b"".join(parts[b]) == R.encode_frames(x, rate, block, stats), (kinds[b], stats)
            if kinds[b] == "constant":
                assert all(s == ("constant",) for s in stats)
            if kinds[b] == "noise":
                assert all(s == ("verbatim",) for s in stats[:-1])
            if kinds[b] == "sine":
                assert any(s[0] == "fixed" and s[2] > 0 for s in stats)      # partitioned residuals


# ---- 2. more than 64 frames in a row: rounds ----------------------------------------------------------------------------------------
def test_rounds():
    """70, 1 and 65 frames of 16 samples in one call: two rounds, the second one without the middle row; every row has a tail to move,
    in ITS last round"""
    rate, block = 8000, 16
    lens = [1120, 16, 1040]
    streams = [_signal("mixed", 5 + n, 7 + b) for b, n in enumerate(lens)]
    dev = [torch.from_numpy(s).cuda() for s in streams]
    objs, twins = _objs(3, rate, block), _objs(3, rate, block)
    parts = [_both(objs, twins, [d[:5] for d in dev], [False] * 3),
             _both(objs, twins, [d[5:] for d in dev], [False] * 3),
             _both(objs, twins, [d[:0] for d in dev], [True] * 3)]
    assert [len(p) for p in parts[0]] == [0, 0, 0] and all(len(p) > 0 for p in parts[2])
    for b in range(3):
        got = b"".join(p[b] for p in parts)
        assert got == R.encode_frames(streams[b], rate, block), b
        y, info = R.decode(R.stream_header(rate, block) + got)
        assert np.array_equal(y, streams[b]) and len(info["frames"]) == lens[b] // block + 1


# ---- 3. any alignment of the output -------------------------------------------------------------------------------------------------
def test_unaligned_output():
    rate, block = 24000, 64
    streams = [_signal("mixed", 700 + 31 * b, 20 + b) for b in range(3)]
    dev = [torch.from_numpy(s).cuda() for s in streams]
    objs, twins = _objs(3, rate, block), _objs(3, rate, block)
    a = _both(objs, twins, [d[:300 + b] for b, d in enumerate(dev)], [False] * 3, odd=True)
    z = _both(objs, twins, [d[300 + b:] for b, d in enumerate(dev)], [True] * 3, odd=True)
    for b in range(3):
        assert a[b] + z[b] == R.encode_frames(streams[b], rate, block), b


# ---- 4. the state the objects are left in -------------------------------------------------------------------------------------------
def test_state_across_pushes():
    """group, then single pushes on half of the objects beside a group of the rest, then the group in reverse order; the push after
    that -- a single one everywhere -- gives what it gives the twins, which have seen single pushes only"""
    rate, block, B = 24000, 64, 6
    streams = [_signal("mixed", 700, 40 + b) for b in range(B)]
    dev = [torch.from_numpy(s).cuda() for s in streams]
    c1, c2, c3 = [10 + 37 * b for b in range(B)], [330 - 20 * b for b in range(B)], [520 + 11 * b for b in range(B)]
    assert all(a < z < e < 700 for a, z, e in zip(c1, c2, c3))
    objs, twins = _objs(B, rate, block), _objs(B, rate, block)
    ends = [b < 2 for b in range(B)]                           # rows 0 and 1 end with the third push
    parts = [_both(objs, twins, [d[:c] for d, c in zip(dev, c1)], [False] * B),
             _both(objs, twins, [d[a:z] for d, a, z in zip(dev, c1, c2)], [False] * B, group=[1, 3, 5]),
             _both(objs, twins, [d[a:z] for d, a, z in zip(dev, c2, c3)], ends, group=list(reversed(range(B))))]
    live = list(range(2, B))
    parts.append([b""] * 2 + _both([objs[b] for b in live], [twins[b] for b in live], [dev[b][c3[b]:] for b in live], [True] * len(live), group=[]))
    for b in range(B):
        assert b"".join(p[b] for p in parts) == R.encode_frames(streams[b][:c3[b] if ends[b] else 700], rate, block), b
    buf = torch.zeros(8, dtype=torch.int64, device="cuda")
    for o in objs + twins:                                      # every stream has ended, for both paths
        assert _raw_single(o, dev[0][:0], False, None, 0, buf.data_ptr())[0] == _lib.FQ3_ESTATE
    rc, _ = _raw_group(objs[2:4], [dev[0][:0]] * 2, [False] * 2, [None] * 2, [0] * 2, [buf.data_ptr(), buf.data_ptr() + 8])
    assert rc == _lib.FQ3_ESTATE


# ---- 5. all or nothing --------------------------------------------------------------------------------------------------------------
def test_all_or_nothing():
    lib = _lib.load()
    rate, block, B = 8000, 16, 4
    streams = [_signal("mixed", 200, 60 + b) for b in range(B)]
    dev = [torch.from_numpy(s).cuda() for s in streams]
    objs, twins = _objs(B, rate, block), _objs(B, rate, block)
    other = _Obj(rate, 64)
    _both(objs, twins, [d[:5 + b] for b, d in enumerate(dev)], [b == 2 for b in range(B)])      # row 2 has ended; the others hold a tail
    xs = [d[5 + b: 45 + b] for b, d in enumerate(dev)]
    need = [o.frames(40, False) * o.bound if b != 2 else 0 for b, o in enumerate(objs)]
    buf = torch.full((B * 256,), GUARD, dtype=torch.uint8, device="cuda")
    nb = torch.full((40,), UNSET, dtype=torch.int64, device="cuda")
    outs, nbs = [buf.data_ptr() + 256 * b for b in range(B)], [nb.data_ptr() + 8 * b for b in range(40)]
    assert max(need) <= 256

    def refused(code, names, rows, caps=None, group_objs=None):
        group_objs = group_objs or [objs[b] for b in rows]
        n = len(group_objs)
        rc, got = _raw_group(group_objs, [xs[b % B] for b in rows], [False] * n, [outs[b % B] for b in rows],
                             caps or [256] * n, nbs[:n])
        assert rc == code and names in lib.fq3_last_error(), (rc, lib.fq3_last_error())
        assert got == [UNSET] * n
        torch.cuda.synchronize()
        assert bool((buf == GUARD).all()) and bool((nb == UNSET).all())      # nothing was launched

    refused(_lib.FQ3_ESTATE, b"row 2", [0, 1, 2, 3])                                             # one row has ended
    refused(_lib.FQ3_EINVAL, b"row 1", [0, 1, 3], caps=[256, need[1] - 1, 256])                   # one row lacks a byte of capacity
    refused(_lib.FQ3_EINVAL, b"same object", [0, 1, 0])                                           # one object twice
    refused(_lib.FQ3_EINVAL, b"32", list(range(33)), group_objs=[objs[b % 2] for b in range(33)])      # B = 33
    refused(_lib.FQ3_EINVAL, b"another design", [0, 1, 3], group_objs=[objs[0], objs[1], other])       # two block sizes
    # no object has moved: the next single push gives what it gives the untouched twins
    live = [0, 1, 3]
    _both([objs[b] for b in live], [twins[b] for b in live], [xs[b] for b in live], [False] * 3, group=[])
    _both([objs[b] for b in live], [twins[b] for b in live], [dev[b][45 + b:] for b in live], [True] * 3)
    assert _raw_single(objs[2], xs[2], False, outs[2], 256, nbs[2])[0] == _lib.FQ3_ESTATE
    assert _both([other], [_Obj(rate, 64)], [dev[0][:100]], [True])[0] == R.encode_frames(streams[0][:100], rate, 64)


# ---- 6. through the Python stage ----------------------------------------------------------------------------------------------------
def test_push_group_host_with_flac_rows():
    """four flac rows and two s16 rows of one rate in ``push_group_host``: the arrays of per-row ``push_host`` on twin stages"""
    rng = np.random.default_rng(9)
    t = np.arange(9000) / 24000.0
    pcm = (0.4 * np.sin(2 * np.pi * 220.0 * t) * np.hanning(9000) + 0.01 * rng.standard_normal(9000)).astype(np.float32)
    x = torch.from_numpy(pcm).cuda()
    specs = [ao.AudioOutSpec(8000, "flac")] * 4 + [ao.AudioOutSpec(8000, "s16")] * 2
    stages, twins = [ao.AudioOut(s, 24000, "cuda") for s in specs], [ao.AudioOut(s, 24000, "cuda") for s in specs]
    starts, cuts = [0, 100, 200, 300, 0, 500], [4000, 100, 2500, 6000, 4000, 3000]       # rows 0 and 4 take the same samples
    pushes = [([x[a:c] for a, c in zip(starts, cuts)], [False] * 6),
              ([x[c:c + 3000] if b != 2 else None for b, c in enumerate(cuts)], [True] * 6)]
    parts = [[] for _ in specs]
    for pcms, finals in pushes:
        got = ao.push_group_host(stages, pcms, finals)
        want = [tw.push_host(p, f) for tw, p, f in zip(twins, pcms, finals)]
        for b, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and np.array_equal(g, w), b
            parts[b].append(np.asarray(g).copy())
    assert [s.n_out for s in stages] == [s.n_out for s in twins] and all(s.finished for s in stages)
    y, info = R.decode(stages[0].header() + np.concatenate(parts[0]).tobytes())
    assert info["rate"] == 8000 and np.array_equal(np.asarray(y, dtype=np.int16), np.concatenate(parts[4]))
