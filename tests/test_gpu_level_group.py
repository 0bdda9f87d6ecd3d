"""GPU: the group form of the leveller and the limiter: loud_push_group_kernel (csrc/loud_kernels.cuh),
level_target_group_kernel and level_apply_group_kernel (csrc/level_kernels.cuh) behind fq3_leveller_push_group, and
limit_push_group_kernel (csrc/limit_kernels.cuh) behind fq3_limit_push_group.

The reference is always a TWIN object driven by single pushes only: tests/test_gpu_leveller.py and tests/test_gpu_limiter.py check the
single push against the numpy references bit for bit, and a group row has to be that push -- output, count and the state the object is
left in.  Every comparison is exact (``torch.equal`` on the bit patterns, ``np.array_equal``); nothing here has a tolerance."""
import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip import _lib
from fq3hip import audio_out as ao
from fq3hip import leveller as M
from fq3hip import limiter as LM

RATES = (8000, 24000)
SPEC = M.LevelSpec(target_lufs=-20.0, smooth_hops=3, min_blocks=2)       # a measured gain from the sixth hop on: the targets get to work
_cache = {}


def _signal(rate):
    """30 s of noise bursts at changing levels, peaks above the limiter's ceiling (a device tensor, made once per rate)"""
    if rate not in _cache:
        rng = np.random.default_rng(rate)
        n = 30 * rate
        env = np.repeat(rng.uniform(0.02, 0.6, n // (rate // 20) + 1), rate // 20)[:n]
        x = (rng.standard_normal(n) * env).astype(np.float32)
        x[:: 997] *= np.float32(3.0)
        _cache[rate] = torch.from_numpy(x).cuda()
    return _cache[rate]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    """bit for bit (a NaN equals the same NaN)"""
    return got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _ptrs(values):
    return (C.c_void_p * len(values))(*values)


def _ptr(t, n=None):
    return t.data_ptr() if (t is not None and (t.numel() if n is None else n)) else None


def _sync_check(rc, want=0):
    torch.cuda.synchronize()
    assert rc == want, (rc, _lib.load().fq3_last_error())


# ---- the leveller ---------------------------------------------------------------------------------------------------------------------
def _level_pair(rate, spec=SPEC, capacity=0):
    return M.Leveller(spec, rate, "cuda", capacity_hops=capacity), M.Leveller(spec, rate, "cuda", capacity_hops=capacity)


def _level_raw(levs, xs, finals, outs, B=None):
    """fq3_leveller_push_group itself on the current stream -> its return code; the host counters move as ``push`` moves them"""
    lib, B = _lib.load(), len(levs) if B is None else B
    ns = [0 if x is None else int(x.numel()) for x in xs]
    rc = lib.fq3_leveller_push_group(_ptrs([l._h.value for l in levs]), B, _ptrs([_ptr(x) for x in xs]), (C.c_int64 * len(ns))(*ns),
                                  (C.c_int * len(ns))(*[int(f) for f in finals]), _ptrs([_ptr(o) for o in outs]),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == 0:
        for l, n, f in zip(levs, ns, finals):
            l.n_in += n
            l.finished = l.finished or bool(f)
    return rc


def _level_state_equal(a, b, where=""):
    ta, tb = a.trace(), b.trace()
    for key in ("energy", "peak", "bad", "target"):
        assert ta[key].dtype == tb[key].dtype and ta[key].tobytes() == tb[key].tobytes(), (where, key)
    sa, sb = a.stats_buffer(), b.stats_buffer()
    assert torch.equal(sa, sb), (where, M.LevelStats.from_bytes(sa.cpu().numpy().tobytes()), M.LevelStats.from_bytes(sb.cpu().numpy().tobytes()))
    assert (a.n_in, a.finished) == (b.n_in, b.finished), where


@pytest.mark.parametrize("rate", RATES)
def test_level_group_equals_single_pushes(rate):
    H, x = rate // 10, _signal(rate)
    names = ["fresh", "mid", "wide", "empty", "empty_final", "partial_final", "nan", "odd_in_place", "g0", "g6", "cuts"]
    specs = {n: SPEC for n in names}
    specs["g6"] = M.LevelSpec(target_lufs=-20.0, smooth_hops=3, min_blocks=2, initial_gain_db=6.0)
    pairs = {n: _level_pair(rate, specs[n]) for n in names}
    pos = {n: 1000 * i for i, n in enumerate(names)}               # every row walks its own part of the signal

    def take(name, n):
        a = x[pos[name]:pos[name] + n].clone()
        pos[name] += n
        return a

    # streams that are already running (single pushes on both objects: group and single pushes mix on one object)
    for name, n in (("mid", 2 * H + H // 2), ("empty", H + H // 2), ("empty_final", 3 * H + 5), ("partial_final", 2 * H)):
        p = take(name, n)
        for lev in pairs[name]:
            lev.push(p.clone())
    nan_row = take("nan", 6 * H + 11)
    nan_row[2 * H + 5] = float("nan")
    plan = [("fresh", take("fresh", H - 1), False),                 # no hop completes: only the history workgroup has work
            ("mid", take("mid", H + 1), False),                     # crosses one border and starts in the history buffer
            ("wide", take("wide", 65 * H + 7), False),              # 65 hops: two meter workgroups, so the rows' grids differ
            ("empty", None, False),
            ("empty_final", None, True),
            ("partial_final", take("partial_final", 2 * H + H // 3), True),
            ("nan", nan_row, False),
            ("odd_in_place", None, False),                          # (filled in below: one float off 16 bytes, out == pcm)
            ("g0", take("g0", 8 * H), False),
            ("g6", take("g6", 8 * H), False),
            ("cuts", take("cuts", 1), False)]
    n_odd = 5 * H + 3
    odd_src = take("odd_in_place", n_odd)
    odd_a, odd_b = torch.zeros(n_odd + 8, device="cuda"), torch.zeros(n_odd + 8, device="cuda")
    odd_a[1:1 + n_odd], odd_b[1:1 + n_odd] = odd_src, odd_src
    assert odd_a.data_ptr() % 16 == 0 and odd_a[1:].data_ptr() % 16 == 4
    xs = [odd_a[1:1 + n_odd] if name == "odd_in_place" else p for name, p, _f in plan]
    outs = [q if name == "odd_in_place" else None if q is None else torch.full_like(q, -7.0) for q, (name, _p, _f) in zip(xs, plan)]
    rc = _level_raw([pairs[name][0] for name, _p, _f in plan], xs, [f for _n, _p, f in plan], outs)
    _sync_check(rc)
    for i, (name, p, final) in enumerate(plan):
        twin = pairs[name][1]
        if name == "odd_in_place":
            want = twin.push(odd_b[1:1 + n_odd], out=odd_b[1:1 + n_odd])
            assert want.data_ptr() == odd_b[1:].data_ptr() and _same(odd_a, odd_b), name       # (the floats around the row included)
        else:
            want = twin.push(p, final)
            assert (outs[i] is None and len(want) == 0) or _same(outs[i], want), name
        _level_state_equal(pairs[name][0], twin, name)
    # a second call: a subset in another order, through the Python function; the cut sequence goes on with it and four more calls
    cuts = [H - 1, H, H + 1, 2 * H + 3, 0]
    second = ["g6", "cuts", "wide", "fresh", "nan", "empty"]
    for call, cut in enumerate(cuts):
        members = second if call == 0 else ["cuts", "mid"]
        pcms = [take(n, cut) if n == "cuts" else take(n, H // 2 + 17 * call) for n in members]
        pcms = [p if len(p) else None for p in pcms]
        got = M.push_group([pairs[n][0] for n in members], pcms, [False] * len(members))
        for n, p, g in zip(members, pcms, got):
            assert _same(g, pairs[n][1].push(p)), (call, n)
            _level_state_equal(pairs[n][0], pairs[n][1], (call, n))
    # single pushes to the end of every stream that still runs
    for name, (a, b) in pairs.items():
        if not a.finished:
            p = take(name, H + 17)
            assert _same(a.push(p, final=True), b.push(p, final=True)), name
        _level_state_equal(a, b, name)
    st = pairs["wide"][0].stats()
    assert st.valid and st.n_hops >= 66 and st.target_gain != 1.0    # the stage had work to do


# ---- the limiter ----------------------------------------------------------------------------------------------------------------------
def _limit_pair(rate, tile=0, spec=None):
    return LM.Limiter(spec, rate, "cuda", tile=tile), LM.Limiter(spec, rate, "cuda", tile=tile)


def _limit_raw(lims, xs, finals, outs, caps, B=None):
    """fq3_limit_push_group itself on the current stream -> (its return code, the counts); the host counters move as ``push`` moves them"""
    lib, B = _lib.load(), len(lims) if B is None else B
    ns = [0 if x is None else int(x.numel()) for x in xs]
    n_out = (C.c_int64 * len(ns))(*([-1] * len(ns)))
    rc = lib.fq3_limit_push_group(_ptrs([l._h.value for l in lims]), B, _ptrs([_ptr(x) for x in xs]), (C.c_int64 * len(ns))(*ns),
                                  (C.c_int * len(ns))(*[int(f) for f in finals]), _ptrs(outs), (C.c_int64 * len(ns))(*caps), n_out,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc == 0:
        for l, n, f, c in zip(lims, ns, finals, n_out):
            l.n_in, l.n_out, l.finished = l.n_in + n, l.n_out + int(c), l.finished or bool(f)
    return rc, [int(c) for c in n_out]


def _limit_state_equal(a, b, where=""):
    assert a.stats() == b.stats() and (a.n_in, a.n_out, a.finished) == (b.n_in, b.n_out, b.finished), (where, a.stats(), b.stats())


def _room(lim, n, final):
    total = lim.n_in + n
    return max((total if final else max(0, total - lim.latency)) - lim.n_out, 0)


@pytest.mark.parametrize("rate,tile", [(24000, 0), (8000, 256)])
def test_limit_group_equals_single_pushes(rate, tile):
    x = _signal(rate)
    latency = LM.design(rate).latency
    plan = [("short", 0, latency - 9, False),                      # a first push shorter than the latency: n_out = 0
            ("one", 3000, 1, False), ("odd", 3000, 777, False), ("tiles", 3000, 4099, False), ("chunk", 3000, 15360, False),
            ("empty", 3000, 0, False),
            ("tail", 3000, 0, True)]                               # final only: the held-back A + 6 samples
    pairs = {name: _limit_pair(rate, tile) for name, *_ in plan}
    xs, at = [], 0
    for name, before, n, _final in plan:
        if before:
            for lim in pairs[name]:
                lim.push(x[at:at + before].clone())
        xs.append(x[at + before:at + before + n].clone() if n else None)
        at += before + n + 13
    rooms = [_room(pairs[name][0], n, final) for name, _b, n, final in plan]
    assert rooms[0] == 0 and rooms[-1] == latency and rooms[-2] == 0
    # the outputs packed at odd float offsets into a buffer full of a sentinel
    SENT = -123.25
    buf = torch.full((sum(rooms) + 3 * len(rooms) + 8,), SENT, device="cuda")
    offs, cursor = [], 1
    for r in rooms:
        offs.append(cursor)
        cursor += r + (2 if (cursor + r) % 2 else 3)               # the next row starts at an odd offset again
    assert all(o % 2 == 1 for o in offs)
    rc, got = _limit_raw([pairs[name][0] for name, *_ in plan], xs, [f for *_, f in plan],
                         [buf.data_ptr() + 4 * o if r else None for o, r in zip(offs, rooms)], rooms)
    _sync_check(rc)
    assert got == rooms
    untouched = torch.ones(len(buf), dtype=torch.bool, device="cuda")
    for (name, _b, _n, final), p, o, r in zip(plan, xs, offs, rooms):
        want = pairs[name][1].push(p, final)
        assert len(want) == r and _same(buf[o:o + r], want), name
        untouched[o:o + r] = False
        _limit_state_equal(pairs[name][0], pairs[name][1], name)
    assert bool((buf[untouched] == SENT).all())                    # nothing outside the rows' counts changed
    assert pairs["chunk"][0].stats().n_limited > 0                 # the stage had work to do
    # the Python function: another subset in another order, rows as views of one buffer; then single pushes to the end
    members = ["chunk", "short", "empty", "one"]
    pcms = [x[50000 + 100 * i:50000 + 100 * i + n].clone() if n else None for i, n in enumerate((2048, 300, 0, 513))]
    finals = [False, False, True, False]
    outs = LM.push_group([pairs[n][0] for n in members], pcms, finals)
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base for o in outs)
    for n, p, f, g in zip(members, pcms, finals, outs):
        assert _same(g, pairs[n][1].push(p, f)), n
        _limit_state_equal(pairs[n][0], pairs[n][1], n)
    for name, (a, b) in pairs.items():
        if not a.finished:
            assert _same(a.push(x[:1234].clone(), final=True), b.push(x[:1234].clone(), final=True)), name
        _limit_state_equal(a, b, name)


# ---- limits and refusals --------------------------------------------------------------------------------------------------------------
def test_group_of_32_and_the_row_limit():
    rate, x = 8000, _signal(8000)
    levs, lims = [_level_pair(rate) for _ in range(33)], [_limit_pair(rate) for _ in range(33)]
    pcms = [x[37 * b:37 * b + 900 + 61 * b].clone() for b in range(33)]
    outs = [torch.empty_like(p) for p in pcms]
    assert _level_raw([p[0] for p in levs], pcms, [False] * 33, outs) == _lib.FQ3_EINVAL           # B = 33
    assert b"32" in _lib.load().fq3_last_error()
    rooms = [_room(p[0], len(q), False) for p, q in zip(lims, pcms)]
    louts = [torch.empty(r, device="cuda") for r in rooms]
    rc, _got = _limit_raw([p[0] for p in lims], pcms, [False] * 33, [_ptr(o) for o in louts], rooms)
    assert rc == _lib.FQ3_EINVAL and all(p[0].n_in == 0 for p in lims)
    _sync_check(_level_raw([p[0] for p in levs[:32]], pcms[:32], [False] * 32, outs[:32]))         # B = 32 in one call
    rc, got = _limit_raw([p[0] for p in lims[:32]], pcms[:32], [False] * 32, [_ptr(o) for o in louts[:32]], rooms[:32])
    _sync_check(rc)
    assert got == rooms[:32]
    for b in range(32):
        assert _same(outs[b], levs[b][1].push(pcms[b])) and _same(louts[b], lims[b][1].push(pcms[b])), b
        _level_state_equal(*levs[b], b)
        _limit_state_equal(*lims[b], b)
    _level_state_equal(*levs[32])                                    # the 33rd objects never moved
    _limit_state_equal(*lims[32])


def test_forty_rows_make_two_calls(monkeypatch):
    rate, x = 8000, _signal(8000)
    lib, calls = _lib.load(), {"level": [], "limit": []}
    for key, name in (("level", "fq3_leveller_push_group"), ("limit", "fq3_limit_push_group")):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, key: lambda *a: (calls[key].append(int(a[1])), real(*a))[1])(real, key))
    levs, lims = [_level_pair(rate) for _ in range(40)], [_limit_pair(rate) for _ in range(40)]
    pcms = [x[11 * b:11 * b + 1500 + 7 * b].clone() for b in range(40)]
    got_v = M.push_group([p[0] for p in levs], pcms, [b % 3 == 0 for b in range(40)])
    got_m = LM.push_group([p[0] for p in lims], pcms, [b % 3 == 0 for b in range(40)])
    assert calls == {"level": [32, 8], "limit": [32, 8]}
    for b in range(40):
        assert _same(got_v[b], levs[b][1].push(pcms[b], b % 3 == 0)) and _same(got_m[b], lims[b][1].push(pcms[b], b % 3 == 0)), b
        _level_state_equal(*levs[b], b)
        _limit_state_equal(*lims[b], b)
    # the Python functions refuse a repeated object, other devices or streams, and lists of different lengths
    with pytest.raises(ValueError, match="twice"):
        M.push_group([levs[1][0], levs[1][0]], pcms[:2], [False, False])
    with pytest.raises(ValueError, match="twice"):
        LM.push_group([lims[1][0], lims[1][0]], pcms[:2], [False, False])
    other = torch.cuda.Stream()
    with pytest.raises(ValueError, match="stream"):
        M.push_group([levs[1][0], M.Leveller(SPEC, rate, "cuda", stream=other)], pcms[:2], [False, False])
    with pytest.raises(ValueError, match="stream"):
        LM.push_group([lims[1][0], LM.Limiter(None, rate, "cuda", stream=other)], pcms[:2], [False, False])
    with pytest.raises(ValueError):
        M.push_group([levs[1][0]], pcms[:2], [False, False])
    assert M.push_group([], [], []) == [] and LM.push_group([], [], []) == []
    # rows of two designs in one Python call: bucketed, one library call each
    calls["level"].clear(), calls["limit"].clear()
    la, lb = _level_pair(24000), _limit_pair(24000, spec=LM.LimiterSpec(-6.0))
    y = _signal(24000)[:5000].clone()
    got_v = M.push_group([levs[1][0], la[0], levs[2][0]], [pcms[1], y, pcms[2]], [False] * 3)
    got_m = LM.push_group([lims[1][0], lb[0], lims[2][0]], [pcms[1], y, pcms[2]], [False] * 3)
    assert sorted(calls["level"]) == [1, 2] and sorted(calls["limit"]) == [1, 2]
    for g, twin, p in zip(got_v + got_m, (levs[1][1], la[1], levs[2][1], lims[1][1], lb[1], lims[2][1]), [pcms[1], y, pcms[2]] * 2):
        assert _same(g, twin.push(p))


def test_refusals_leave_every_object_where_it_was():
    rate, x = 8000, _signal(8000)
    H = rate // 10
    lib = _lib.load()
    levs, lims = [_level_pair(rate) for _ in range(3)], [_limit_pair(rate) for _ in range(3)]
    small = _level_pair(rate, capacity=4)
    mixed_v = _level_pair(rate, M.LevelSpec(target_lufs=-23.0, smooth_hops=3, min_blocks=2))
    mixed_m = _limit_pair(rate, tile=512)
    everyone_v, everyone_m = levs + [small, mixed_v], lims + [mixed_m]
    first = [x[100 * i:100 * i + 2 * H + 31 * i].clone() for i in range(6)]
    for i, pair in enumerate(everyone_v + everyone_m):
        for obj in pair:
            obj.push(first[i % 6].clone())
    # the object in the middle has ended
    for pair in (levs[1], lims[1]):
        for obj in pair:
            obj.push(None, final=True)
    p3 = [x[7000 + 50 * i:7000 + 50 * i + H + 5].clone() for i in range(3)]
    o3 = [torch.full_like(p, 9.0) for p in p3]
    rooms = [_room(l[0], len(p), False) for l, p in zip(lims, p3)]
    m3 = [torch.full((max(r, 1),), 9.0, device="cuda") for r in rooms]

    def level(members, pcms, outs, finals=None):
        return _level_raw([m[0] for m in members], pcms, finals or [False] * len(members), outs)

    def limit(members, pcms, outs, caps, finals=None):
        return _limit_raw([m[0] for m in members], pcms, finals or [False] * len(members), [_ptr(o) for o in outs], caps)[0]

    assert level(levs, p3, o3) == _lib.FQ3_ESTATE and b"row 1" in lib.fq3_last_error()
    assert limit(lims, p3, m3, rooms) == _lib.FQ3_ESTATE and b"row 1" in lib.fq3_last_error()
    # beyond the hop capacity (4 hops; the object holds 2 H already) in the last row
    assert level([levs[0], levs[2], small], p3[:2] + [x[:3 * H].clone()], o3[:2] + [torch.empty(3 * H, device="cuda")]) == _lib.FQ3_ETOOLONG
    # a limiter row whose capacity is too small
    assert limit([lims[0], lims[2]], [p3[0], p3[2]], [m3[0], m3[2]], [rooms[0], rooms[2] - 1]) == _lib.FQ3_EINVAL
    # mixed designs, the same object twice, a null object
    assert level([levs[0], mixed_v], p3[:2], o3[:2]) == _lib.FQ3_EINVAL and b"design" in lib.fq3_last_error()
    assert limit([lims[0], mixed_m], p3[:2], m3[:2], rooms[:2]) == _lib.FQ3_EINVAL and b"design" in lib.fq3_last_error()
    assert level([levs[0], levs[2], levs[0]], p3, o3) == _lib.FQ3_EINVAL and b"same object" in lib.fq3_last_error()
    assert limit([lims[0], lims[2], lims[0]], p3, m3, [rooms[0], rooms[2], rooms[0]]) == _lib.FQ3_EINVAL and b"same object" in lib.fq3_last_error()
    # the Python function gives a refused row its single push's error, before any object moves
    with pytest.raises(_lib.Fq3Error):
        M.push_group([m[0] for m in levs], p3, [False] * 3)
    with pytest.raises(RuntimeError, match="capacity"):
        M.push_group([levs[0][0], small[0]], [p3[0], x[:3 * H].clone()], [False] * 2)
    with pytest.raises(_lib.Fq3Error):
        LM.push_group([m[0] for m in lims], p3, [False] * 3)
    torch.cuda.synchronize()
    assert all(bool((o == 9.0).all()) for o in o3 + m3)              # nothing was launched
    # nothing moved: valid pushes go on and still match the twins
    live_v, live_m = [levs[0], levs[2], small], [lims[0], lims[2]]
    pcms = [p3[0], p3[2], x[:H].clone()]
    got = M.push_group([m[0] for m in live_v], pcms, [False, True, False])
    for m, p, f, g in zip(live_v, pcms, [False, True, False], got):
        assert _same(g, m[1].push(p, f))
    got = LM.push_group([m[0] for m in live_m] + [mixed_m[0]], pcms, [False, True, False])
    for m, p, f, g in zip(live_m + [mixed_m], pcms, [False, True, False], got):
        assert _same(g, m[1].push(p, f))
    for pair in everyone_v:
        _level_state_equal(*pair)
    for pair in everyone_m:
        _limit_state_equal(*pair)


# ---- the lock-step batch ----------------------------------------------------------------------------------------------------------------
TEXTS = ["The quick brown fox jumps. Over the lazy dog it goes!", "A second line, somewhat shorter.", "Three words here."]
LEVEL = dict(target_lufs=-20.0, smooth_hops=3, min_blocks=2)           # a 22-frame utterance has 17 hops: the stage must get to work in it


def _model():
    """the small synthetic model, greedy; this file's own (the pools a model keeps are part of what other files assert on theirs)"""
    if "m" not in _cache:
        from fq3hip.config import tiny_test_config
        from fq3hip.model import FasterQwen3TTS
        from fq3hip.weights import synth_weights
        cfg = copy.deepcopy(tiny_test_config())
        cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "1b7"
        cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
        W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "text", "codec"))
        m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, max_frames=48, codec_max_frames=64)
        m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
        _cache["m"] = (m, dict(do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0, max_new_tokens=22, min_new_tokens=22))
    return _cache["m"]


def _raise(*_a, **_kw):
    raise AssertionError("the lock-step batch pushes its levellers and limiters through the group functions")


@pytest.mark.parametrize("exact", [False, True], ids=["windowed", "exact"])
@pytest.mark.parametrize("output", [None, ao.AudioOutSpec(8000, "mulaw")], ids=["f32", "mulaw"])
def test_batch_streaming_goes_through_the_group_functions(output, exact, monkeypatch):
    m, kw = _model()
    skw = dict(kw, chunk_size=4, non_streaming_mode=False)

    def batch():
        got = {i: [] for i in range(len(TEXTS))}
        extra = {} if output is None else dict(output=output)
        with monkeypatch.context() as mp:                            # around the batch call only
            mp.setattr(M.Leveller, "push", _raise)
            mp.setattr(LM.Limiter, "push", _raise)
            for i, a, _sr, _tm in m.generate_custom_voice_batch_streaming(TEXTS, "bob", "English", lanes=3, **extra, **skw):
                got[i].append(np.asarray(a).copy())
        return [np.concatenate(v) for _i, v in sorted(got.items())]

    def single(text):
        with (contextlib.nullcontext() if output is None else m.audio_output(output.sample_rate, output.encoding)):
            return np.concatenate([np.asarray(a).copy() for a, _sr, _tm in m.generate_custom_voice_streaming(text, "bob", "English", **skw)])

    with (m.exact_streaming() if exact else contextlib.nullcontext()), m.seeded(0):
        with m.fixed_gain(6.0), m.leveller(**LEVEL), m.limiter():
            got = batch()
            want = [single(t) for t in TEXTS]
        plain = single(TEXTS[0])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == (np.float32 if output is None else np.uint8) and np.array_equal(g, w), (i, len(g), len(w))
    assert len(plain) == len(want[0]) and not np.array_equal(plain, want[0])          # the stages had work to do
