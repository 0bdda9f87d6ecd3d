"""GPU: the group form of the segment join (join_group_kernel behind fq3_join_push_group).  Every row of a
group call is compared bit for bit -- samples, count, and what the object does afterwards -- with (i) a twin object driven by
fq3_join_push alone and (ii) the NumPy reference (tests/_join_ref.py) of the whole stream.  The arithmetic is comparisons and copies,
so no tolerance applies; arrays are compared as bit patterns, because one row carries NaNs.  24 kHz: H = 240."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _join_ref as R
from fq3hip import _lib
from fq3hip import long_form as lf
from fq3hip.long_form import SegmentJoin

RATE, H = 24000, 240
THR, LEAD, TAIL, HOLD = 0.25, 1, 2, 4
CUTS = [0, 1, 239, 240, 241, 3 * H + 5, 485, 1920]
BIG = 257 * H + 7                                                   # one push that crosses kJoinSlice = 256 hops


def _tone(n, seed):
    rng = np.random.default_rng(seed)
    return (np.sign(rng.standard_normal(n)) * rng.uniform(0.3, 0.9, n)).astype(np.float32)


def _quiet(n, seed):
    return np.random.default_rng(seed).uniform(-0.2, 0.2, n).astype(np.float32)


def _segment(parts, seed):
    return np.concatenate([(_tone if k == "t" else _quiet)(n, seed + i) for i, (k, n) in enumerate(parts)])


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _stream(b):
    """-> (segments, pauses, pushes [(segment, first, stop, end, pause)]) of stream ``b``: the recipes turn with ``b``"""
    s = 1000 * b
    seg0 = _segment([("q", 3 * H), ("t", 2 * H + b), ("q", (b % 7) * H + 5)], s)
    if b % 8 == 0:
        seg0[7] = np.nan                                            # in a quiet hop: compares false, stays inactive
        seg0[3 * H + 3] = np.nan                                    # in an active hop: copied bit for bit
    seg1 = _segment([("q", 9 * H + 17)], s + 10) if b % 4 == 1 else _segment([("t", H + 31), ("q", 6 * H)], s + 10)      # all silent: no pause
    if b % 8 == 2:
        seg2 = _segment([("q", 100 * H), ("t", 3 * H), ("q", 3 * H), ("t", 160 * H + 9), ("q", 40 * H)], s + 20)
    else:
        seg2 = _segment([("q", H // 2), ("t", 4 * H), ("q", 239)], s + 20)
    segs, pauses = [seg0, seg1, seg2], [0 if b % 2 else 1200, 2400, 0]
    pushes, c = [], b
    for k, x in enumerate(segs):
        end = 2 if k == 2 else 1
        pos, cuts = 0, []
        if len(x) > BIG:
            cuts.append(BIG)
            pos = BIG
        while pos < len(x):
            n = min(CUTS[c % len(CUTS)], len(x) - pos)
            c += 1
            cuts.append(n)
            pos += n
        if b % 5 == 3:
            cuts.append(0)                                          # the segment is ended by an empty push
        pos = 0
        for i, n in enumerate(cuts):
            last = i == len(cuts) - 1
            pushes.append((k, pos, pos + n, end if last else 0, pauses[k] if last and end == 1 else 0))
            pos += n
    return segs, pauses, pushes


class _Driver:
    """raw C calls: inputs and outputs one float into their buffers, outputs guarded by a fill value"""

    def __init__(self):
        self.lib = _lib.load()
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def dev(x):
        buf = torch.empty(len(x) + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(np.ascontiguousarray(x))
        return buf[1:]                                              # the pointer is offset by one float

    def rooms(self, joins, xs, ends, pauses, short=None):
        # (the reference's bound: it does not check its arguments, so a call that is to be refused gets its rooms as well)
        caps = [R.bound(j.in_rate, j.cfg.lead_hops, j.cfg.hold_hops, int(x.numel()), p if e == 1 else 0) - (1 if short == i else 0)
                for i, (j, x, e, p) in enumerate(zip(joins, xs, ends, pauses))]
        bufs = [torch.full((1 + cap + 4,), -7.0, dtype=torch.float32, device="cuda") for cap in caps]
        return caps, bufs, torch.full((len(joins),), -5, dtype=torch.int64, device="cuda")

    def group(self, joins, xs, ends, pauses, short=None):
        B = len(joins)
        caps, bufs, n_dev = self.rooms(joins, xs, ends, pauses, short)
        rc = self.lib.fq3_join_push_group(
            (C.c_void_p * B)(*[j._h.value for j in joins]), B, (C.c_void_p * B)(*[x.data_ptr() if x.numel() else None for x in xs]),
            (C.c_int64 * B)(*[int(x.numel()) for x in xs]), (C.c_int * B)(*ends), (C.c_int64 * B)(*pauses),
            (C.c_void_p * B)(*[b.data_ptr() + 4 for b in bufs]), (C.c_int64 * B)(*caps),
            (C.c_void_p * B)(*[n_dev.data_ptr() + 8 * i for i in range(B)]), self.sp)
        return rc, self.read(bufs, caps, n_dev)

    def single(self, j, x, end, pause):
        caps, bufs, n_dev = self.rooms([j], [x], [end], [pause])
        rc = self.lib.fq3_join_push(j._h, C.c_void_p(x.data_ptr() if x.numel() else None), int(x.numel()), end, pause,
                                    C.c_void_p(bufs[0].data_ptr() + 4), caps[0], C.c_void_p(n_dev.data_ptr()), self.sp)
        return rc, self.read(bufs, caps, n_dev)[0]

    @staticmethod
    def read(bufs, caps, n_dev):
        """-> per row (count, samples or None when the row was not written); nothing outside [0, count) may have been touched"""
        out = []
        for buf, cap, n in zip(bufs, caps, n_dev.cpu().tolist()):
            host = buf.cpu().numpy()
            if n == -5:
                assert (host == -7.0).all()
                out.append((n, None))
                continue
            assert 0 <= n <= cap and host[0] == -7.0 and (host[1 + n:] == -7.0).all()
            out.append((n, host[1: 1 + n]))
        return out


@pytest.mark.parametrize("B", [1, 2, 32])
def test_group_rows_equal_single_pushes_and_the_reference(B):
    """membership changes from call to call (late starters: a fresh row beside running ones; rows that sit out every other call; rows
    that run out), and now and then a member takes a single push on the SAME object between two group calls"""
    d = _Driver()
    streams = [_stream(b) for b in range(B)]
    data = [[d.dev(x) for x in segs] for segs, _p, _q in streams]
    grp = [SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD) for _ in range(B)]
    twin = [SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD) for _ in range(B)]
    pos, got, calls, sizes = [0] * B, [[] for _ in range(B)], 0, set()
    for step in range(400):
        if all(pos[b] >= len(streams[b][2]) for b in range(B)):
            break
        members = [b for b in range(B) if pos[b] < len(streams[b][2]) and step >= (2 if b % 3 == 1 else 0)
                   and not (b % 4 == 3 and step % 2 == 1)]
        if not members:
            continue
        args = {}
        for b in members:
            k, i0, i1, end, pause = streams[b][2][pos[b]]
            args[b] = (data[b][k][i0:i1], end, pause)
            pos[b] += 1
        alone = [members.pop(0)] if step % 5 == 4 and len(members) > 1 else []
        for b in alone:                                             # a single push on the object the groups drive
            rc, row = d.single(grp[b], *args[b])
            assert rc == 0
            args[b] = args[b] + (row,)
        rc, rows = d.group([grp[b] for b in members], [args[b][0] for b in members], [args[b][1] for b in members],
                           [args[b][2] for b in members])
        assert rc == 0, d.lib.fq3_last_error()
        calls += 1
        sizes.add(len(members))
        for b, row in zip(members, rows):
            args[b] = args[b] + (row,)
        for b in alone + members:
            x, end, pause, (n, y) = args[b]
            rc, (n1, y1) = d.single(twin[b], x, end, pause)
            assert rc == 0 and n == n1 and _same(y, y1), (B, step, b)
            got[b].append(y)
    assert all(pos[b] == len(streams[b][2]) for b in range(B)) and max(sizes) == B
    assert B == 1 or len(sizes) > 1                                 # the membership did change
    for b, (segs, pauses, _pushes) in enumerate(streams):
        want = R.join(list(zip(segs, pauses)), RATE, THR, LEAD, TAIL, HOLD)
        assert want.size > 0 and _same(np.concatenate(got[b]), want), (B, b)
    # the streams have ended: every object answers as its twin does
    x = data[0][0][:10]
    assert d.single(grp[0], x, 0, 0)[0] == _lib.FQ3_ESTATE == d.single(twin[0], x, 0, 0)[0]


def test_all_or_nothing_and_state_errors_in_the_middle_of_a_group():
    d = _Driver()
    streams = [_stream(b) for b in (4, 5, 6)]
    grp = [SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD) for _ in range(3)]
    twin = [SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD) for _ in range(3)]
    xs = [d.dev(s[0][0]) for s in streams]
    heads = []
    for j, t, x in zip(grp, twin, xs):                              # running streams: a partial hop and a queue are pending
        rc, (_n, head) = d.single(j, x[:1000], 0, 0)
        assert rc == 0 and d.single(t, x[:1000], 0, 0)[0] == 0
        heads.append(head)
    rest, ends, pauses = [x[1000:] for x in xs], [1, 1, 1], [1200, 7, 0]
    rc, rows = d.group(grp, rest, ends, pauses, short=1)            # row 1: capacity one below the bound
    assert rc == _lib.FQ3_EINVAL and b"row 1" in d.lib.fq3_last_error() and b"below the bound" in d.lib.fq3_last_error()
    assert all(n == -5 and y is None for n, y in rows)              # nothing was launched
    for bad_end in (-1, 3):
        assert d.group(grp, rest, [1, 1, bad_end], pauses)[0] == _lib.FQ3_EINVAL and b"row 2" in d.lib.fq3_last_error()
    assert d.group(grp, rest, ends, [0, 0, 5 * RATE + 1])[0] == _lib.FQ3_EINVAL and b"row 2" in d.lib.fq3_last_error()
    rc, rows = d.group(grp, rest, ends, pauses)                     # the correct call: nothing had moved
    assert rc == 0
    for t, x, e, p, (n, y), s, head in zip(twin, rest, ends, pauses, rows, streams, heads):
        rc, (n1, y1) = d.single(t, x, e, p)
        assert rc == 0 and n == n1 and _same(y, y1)
        assert _same(np.concatenate([head, y]), R.join([(s[0][0], p)], RATE, THR, LEAD, TAIL, HOLD, last_pause=True))
    # row 1 ends its stream; the next group has it in the middle: FQ3_ESTATE, and rows 0 and 2 have not moved
    e = torch.zeros(0, dtype=torch.float32, device="cuda")
    assert d.single(grp[1], e, 2, 0)[0] == 0 and d.single(twin[1], e, 2, 0)[0] == 0
    nxt = [d.dev(s[0][1]) for s in streams]
    rc, rows = d.group(grp, nxt, [1, 0, 2], [2400, 0, 0])
    assert rc == _lib.FQ3_ESTATE and b"row 1" in d.lib.fq3_last_error() and all(n == -5 for n, _y in rows)
    rc, rows = d.group([grp[0], grp[2]], [nxt[0], nxt[2]], [1, 2], [2400, 0])
    assert rc == 0
    for t, x, e_, p, (n, y) in zip([twin[0], twin[2]], [nxt[0], nxt[2]], [1, 2], [2400, 0], rows):
        rc, (n1, y1) = d.single(t, x, e_, p)
        assert rc == 0 and n == n1 and _same(y, y1)


def test_two_configurations_in_one_group():
    d = _Driver()
    cfgs = [(0.25, 1, 2, 4), (0.5, 2, 1, 2)]                        # threshold and hold_hops differ (and lead / tail with them)
    segs = [_segment([("q", 4 * H), ("t", 2 * H), ("q", 3 * H + 9), ("t", H), ("q", 8 * H)], 77), _segment([("t", 3 * H), ("q", 5 * H)], 78)]
    segs[0][4 * H: 5 * H] *= np.float32(0.5)                        # a hop that is active at 0.25 and inactive at 0.5
    xs = [d.dev(x) for x in segs]
    grp = [SegmentJoin(RATE, "cuda", *c) for c in cfgs]
    twin = [SegmentJoin(RATE, "cuda", *c) for c in cfgs]
    got = [[], []]
    for k, x in enumerate(xs):
        for i in range(0, x.numel(), 1000):
            last = i + 1000 >= x.numel()
            end = 0 if not last else (2 if k == 1 else 1)
            rc, rows = d.group(grp, [x[i: i + 1000]] * 2, [end] * 2, [480 if end == 1 else 0] * 2)
            assert rc == 0
            for r, (n, y) in enumerate(rows):
                rc, (n1, y1) = d.single(twin[r], x[i: i + 1000], end, 480 if end == 1 else 0)
                assert rc == 0 and n == n1 and _same(y, y1)
                got[r].append(y)
    want = [R.join([(segs[0], 480), (segs[1], 0)], RATE, *c) for c in cfgs]
    assert not _same(want[0], want[1])
    assert _same(np.concatenate(got[0]), want[0]) and _same(np.concatenate(got[1]), want[1])


def test_python_push_group_equals_push():
    """``long_form.push_group``: the device tensors and the counters of ``SegmentJoin.push``; 33 rows go out in two calls; a lone row"""
    n_rows = lf.GROUP_MAX + 1
    streams = [_stream(b) for b in range(n_rows)]
    grp = [SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD) for _ in range(n_rows)]
    twin = [SegmentJoin(RATE, "cuda", THR, LEAD, TAIL, HOLD) for _ in range(n_rows)]
    got = [[] for _ in range(n_rows)]
    for k in range(3):
        end = 2 if k == 2 else 1
        xs = [torch.from_numpy(s[0][k]).cuda() for s in streams]
        rows = range(n_rows) if k != 1 else [0]                     # segment 1: a lone row through the group call, the others singly
        ys = lf.push_group([grp[b] for b in rows], [xs[b] for b in rows], [end] * len(rows), [streams[b][1][k] for b in rows])
        assert len(ys) == len(rows)
        for b in range(n_rows):
            y1 = twin[b].push(xs[b], end, streams[b][1][k])
            y = ys[b] if k != 1 else (ys[0] if b == 0 else grp[b].push(xs[b], end, streams[b][1][k]))
            assert y.is_cuda and y.dtype == torch.float32 and _same(y.cpu().numpy(), y1.cpu().numpy()), (k, b)
            assert (grp[b].n_in, grp[b].n_out, grp[b].finished) == (twin[b].n_in, twin[b].n_out, twin[b].finished)
            got[b].append(y.cpu().numpy())
    for b, (segs, pauses, _p) in enumerate(streams):
        assert _same(np.concatenate(got[b]), R.join(list(zip(segs, pauses)), RATE, THR, LEAD, TAIL, HOLD)), b
    with pytest.raises(ValueError):
        lf.push_group([grp[0], grp[0]], [None, None], [0, 0], [0, 0])
    with pytest.raises(_lib.Fq3Error) as e:                         # ended streams: the library's own answer
        lf.push_group(grp[:2], [None, None], [0, 0], [0, 0])
    assert e.value.code == _lib.FQ3_ESTATE
    # all or nothing across the calls of one push_group: 33 rows whose LAST one (the second call's only row) is refused -- an ended
    # stream, then a pause out of range -- leave the 32 rows of the first call where they were
    for j in grp[:-1] + twin[:-1]:
        j.reset()
    x = torch.from_numpy(streams[0][0][0]).cuda()
    before = [(j.n_in, j.n_out) for j in grp]
    with pytest.raises(_lib.Fq3Error) as e:
        lf.push_group(grp, [x] * n_rows, [0] * n_rows, [0] * n_rows)
    assert e.value.code == _lib.FQ3_ESTATE
    grp[-1].reset()
    twin[-1].reset()
    with pytest.raises(_lib.Fq3Error) as e:
        lf.push_group(grp, [x] * n_rows, [1] * n_rows, [0] * (n_rows - 1) + [5 * RATE + 1])
    assert e.value.code == _lib.FQ3_EINVAL and [(j.n_in, j.n_out) for j in grp[:-1]] == before[:-1]
    ys = lf.push_group(grp, [x] * n_rows, [2] * n_rows, [0] * n_rows)       # the correct call: nothing had moved
    for b in range(n_rows):
        assert _same(ys[b].cpu().numpy(), twin[b].push(x, 2, 0).cpu().numpy()), b
