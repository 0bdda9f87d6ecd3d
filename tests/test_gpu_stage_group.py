"""GPU: the output stages for a GROUP of streams -- fq3_audio_out_push_group (audio_out_group_kernel, csrc/audio_kernels.cuh) and
fq3_tsm_push_group (tsm_group_kernel, csrc/tsm_kernels.cuh), ``audio_out.push_group`` above them and the ``output=`` keyword of the
lock-step batch entry points on top.

The contract is equality with the single pushes, bit for bit: every comparison here is against TWIN objects that are driven by single
pushes only (whose own accuracy tests/test_gpu_audio_out.py and tests/test_gpu_tsm.py check), with ``torch.equal`` /
``np.array_equal`` -- there is no tolerance anywhere.  State that cannot be read back (the history buffers, the time-scale stage's
last delta on the device) is compared through what it does to the pushes that follow.

Bank forms: with the default 16 zero crossings every rate pair of tests/test_gpu_audio_out.py stages its bank in LDS (L K is at most
10560 floats against the 12288 that are staged), so the form that reads the bank from global memory is reached here with 64 zero
crossings on the (147, 80) pair of that file: 147 rows of 129 taps."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _flac_ref as R
from fq3hip import _lib
from fq3hip import audio_out as ao
from test_gpu_audio_out import _tiny_model

FORMATS = {"f32": (0, torch.float32), "s16": (1, torch.int16), "mulaw": (2, torch.uint8), "alaw": (3, torch.uint8)}
EINVAL, ESTATE = _lib.FQ3_EINVAL, _lib.FQ3_ESTATE

_cache = {}


def _noise():
    """40000 samples in [-1, 1] on the device (made once, never modified)"""
    if "x" not in _cache:
        _cache["x"] = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, 40000).astype(np.float32)).cuda()
    return _cache["x"]


def _speech():
    """40000 samples with a pitch, so that the time-scale stage's search has something to find (made once, never modified)"""
    if "s" not in _cache:
        t = np.arange(40000) / 24000.0
        rng = np.random.default_rng(6)
        s = 0.5 * np.sin(2 * np.pi * 140.0 * t + 3.0 * np.sin(2 * np.pi * 2.0 * t)) + 0.2 * np.sin(2 * np.pi * 700.0 * t) + 0.05 * rng.standard_normal(40000)
        _cache["s"] = torch.from_numpy(s.astype(np.float32)).cuda()
    return _cache["s"]


def _ptr_array(values):
    return (C.c_void_p * len(values))(*values)


class _Audio:
    """fq3_audio_out_* through ctypes, on the current stream"""

    def __init__(self, i, o, fmt, zero=0):
        self.lib, self.i, self.o, self.zero = _lib.load(), i, o, zero
        self.dtype = FORMATS[fmt][1]
        self.h = C.c_void_p()
        assert self.lib.fq3_audio_out_create(C.byref(_lib.AudioOutConfig(i, o, FORMATS[fmt][0], zero)), C.byref(self.h)) == 0, self.lib.fq3_last_error()
        self.n_in = self.n_out = 0

    def __del__(self):
        self.lib.fq3_audio_out_destroy(self.h)

    def due(self, n, final):
        """outputs a push of n samples completes"""
        return self.lib.fq3_audio_out_count(self.i, self.o, self.zero, self.n_in + n, 1 if final else 0) - self.n_out

    def moved(self, n, cnt):
        self.n_in, self.n_out = self.n_in + n, self.n_out + cnt

    def push(self, x, final=False):
        cap = self.due(x.numel(), final)
        out = torch.empty(cap, dtype=self.dtype, device="cuda")
        n = C.c_int64(-1)
        rc = self.lib.fq3_audio_out_push(self.h, C.c_void_p(x.data_ptr() if x.numel() else None), x.numel(), 1 if final else 0,
                                         C.c_void_p(out.data_ptr() if cap else None), cap, C.byref(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and n.value == cap, (rc, n.value, cap, self.lib.fq3_last_error())
        self.moved(x.numel(), cap)
        return out


class _Tsm(_Audio):
    """fq3_tsm_* through ctypes, on the current stream"""

    def __init__(self, rate, permille):
        self.lib, self.rate, self.p, self.dtype = _lib.load(), rate, permille, torch.float32
        self.h = C.c_void_p()
        assert self.lib.fq3_tsm_create(C.byref(_lib.TsmConfig(rate, permille)), C.byref(self.h)) == 0, self.lib.fq3_last_error()
        self.n_in = self.n_out = 0

    def __del__(self):
        self.lib.fq3_tsm_destroy(self.h)

    def due(self, n, final):
        return self.lib.fq3_tsm_count(self.rate, self.p, self.n_in + n, 1 if final else 0) - self.n_out

    def push(self, x, final=False):
        cap = self.due(x.numel(), final)
        out = torch.empty(cap, dtype=torch.float32, device="cuda")
        n = C.c_int64(-1)
        rc = self.lib.fq3_tsm_push(self.h, C.c_void_p(x.data_ptr() if x.numel() else None), x.numel(), 1 if final else 0,
                                   C.c_void_p(out.data_ptr() if cap else None), cap, C.byref(n), None, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and n.value == cap, (rc, n.value, cap, self.lib.fq3_last_error())
        self.moved(x.numel(), cap)
        return out


def _raw_group(stages, xs, finals, outs, caps, B=None):
    """the group call as it is -> (return code, n_out[])"""
    lib = _lib.load()
    fn = lib.fq3_tsm_push_group if isinstance(stages[0], _Tsm) else lib.fq3_audio_out_push_group
    B = len(stages) if B is None else B
    n_out = (C.c_int64 * len(stages))(*([-7] * len(stages)))
    rc = fn(_ptr_array([s.h.value for s in stages]), B, _ptr_array([x.data_ptr() if x.numel() else None for x in xs]),
            (C.c_int64 * len(xs))(*[x.numel() for x in xs]), (C.c_int * len(finals))(*[int(f) for f in finals]), _ptr_array(outs),
            (C.c_int64 * len(caps))(*caps), n_out, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, list(n_out)


def _group(stages, xs, finals, lead=1):
    """One group push with the rows' outputs PACKED back to back from element ``lead`` of a sentinel-filled buffer (rows start at
    whatever element offset they fall on) -> the rows' outputs; nothing but they may have been written."""
    esz = torch.empty(0, dtype=stages[0].dtype).element_size()
    caps = [s.due(x.numel(), f) for s, x, f in zip(stages, xs, finals)]
    total = lead + sum(caps)
    buf = torch.full(((total + 16) * esz,), 0xA5, dtype=torch.uint8, device="cuda")
    offs = [lead + sum(caps[:b]) for b in range(len(caps))]
    rc, n_out = _raw_group(stages, xs, finals, [buf.data_ptr() + o * esz if c else None for o, c in zip(offs, caps)], caps)
    assert rc == 0 and n_out == caps, (rc, n_out, caps, _lib.load().fq3_last_error())
    for s, x, c in zip(stages, xs, caps):
        s.moved(x.numel(), c)
    host = buf.cpu()
    assert bool((host[:lead * esz] == 0xA5).all()) and bool((host[total * esz:] == 0xA5).all())
    return [buf[o * esz:(o + c) * esz].clone().view(s.dtype) for s, o, c in zip(stages, offs, caps)]


def _same(got, want):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (b, g.shape, w.shape)


# ---- 1. fq3_audio_out_push_group against single pushes ---------------------------------------------------------------------------
AUDIO_CASES = [(24000, 8000, "mulaw", 0),       # L = 1, the telephony pair; bank in LDS
               (8000, 14700, "s16", 0),         # 147 / 80: bank in LDS
               (8000, 14700, "f32", 64),        # 147 rows of 129 taps: bank in global memory
               (8000, 14700, "alaw", 64),       # the same, four samples to a word
               (24000, 24000, "alaw", 0),       # the encoder alone, K = 1
               (24000, 24000, "f32", 0)]


@pytest.mark.parametrize("case", AUDIO_CASES, ids=lambda c: f"{c[0]}to{c[1]}-{c[2]}-z{c[3]}")
def test_audio_group_equals_single_pushes(case):
    x = _noise()
    E = x[:0]
    # (what the row has seen before the group push, its new samples, final)
    plan = [([], x[100:15460], 0),                                   # fresh; one 8-frame chunk
            ([x[7:8]], x[8:9], 0),                                   # after one sample: the history is shorter than K - 1
            ([x[20:3020], x[3020:5020]], x[5020:9119], 0),           # after pushes longer than the history; 4099 new
            ([x[30:530]], E, 0),                                     # nothing to do
            ([x[40:2540]], E, 1),                                    # the tail alone
            ([x[50:150]], x[150:927], 0)]                            # 777 new
    rows, twins = [_Audio(*case) for _ in plan], [_Audio(*case) for _ in plan]
    for r, t, (before, _new, _f) in zip(rows, twins, plan):
        for part in before:
            _same([r.push(part)], [t.push(part)])
    got = _group(rows, [p[1] for p in plan], [p[2] for p in plan])
    _same(got, [t.push(new, bool(f)) for t, (_b, new, f) in zip(twins, plan)])
    assert [r.n_out for r in rows] == [t.n_out for t in twins]
    # another membership, another order: rows 2 and 0 swapped, row 5; one of them ends here
    order, new, fin = [2, 0, 5], [x[9119:9120], x[15460:16237], E], [0, 0, 1]
    got = _group([rows[b] for b in order], new, fin, lead=3)
    _same(got, [twins[b].push(n, bool(f)) for b, n, f in zip(order, new, fin)])
    # to the end by single pushes: the state the group pushes left is the state single pushes leave
    for b in (0, 1, 2, 3):
        _same([rows[b].push(x[20000 + b:20300 + 2 * b], True)], [twins[b].push(x[20000 + b:20300 + 2 * b], True)])
    assert [r.n_out for r in rows] == [t.n_out for t in twins] and [r.n_in for r in rows] == [t.n_in for t in twins]


# ---- 2. limits and atomicity ------------------------------------------------------------------------------------------------------
def test_audio_group_limits_and_atomicity():
    x = _noise()
    case = (24000, 8000, "mulaw", 0)
    rows, twins = [_Audio(*case) for _ in range(33)], [_Audio(*case) for _ in range(33)]
    xs = [x[b:b + 500 + b] for b in range(33)]                        # the rows' lengths differ by one sample each
    caps = [r.due(v.numel(), 0) for r, v in zip(rows, xs)]
    buf = torch.full((sum(caps) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [buf.data_ptr() + sum(caps[:b]) for b in range(33)]
    rc, _n = _raw_group(rows, xs, [0] * 33, outs, caps)              # B = 33
    assert rc == EINVAL
    other = _Audio(24000, 8000, "alaw", 0)
    for stages in ([rows[0], other, rows[2]], [rows[0], rows[1], rows[0]]):      # another design; the same object twice
        rc, _n = _raw_group(stages, xs[:3], [0] * 3, outs[:3], [c + 64 for c in caps[:3]])
        assert rc == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    got = _group(rows[:32], xs[:32], [0] * 32, lead=1)               # B = 32
    _same(got, [t.push(v) for t, v in zip(twins[:32], xs[:32])])
    # a finished row / a row whose capacity is one sample short: that row's code, and no object has moved
    done, done_twin = rows[5], twins[5]
    _same([done.push(x[:0], True)], [done_twin.push(x[:0], True)])
    part, more = [rows[3], rows[5], rows[4]], [x[900:1700], x[:10], x[1700:2001]]
    caps = [part[0].due(800, 0), 64, part[2].due(301, 0)]             # (past its end the finished row has no count: any room will do)
    buf = torch.full((sum(caps) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [buf.data_ptr() + sum(caps[:b]) for b in range(3)]
    rc, _n = _raw_group(part, more, [0] * 3, outs, caps)
    assert rc == ESTATE
    part[1] = rows[6]
    caps = [r.due(v.numel(), 0) for r, v in zip(part, more)]
    rc, _n = _raw_group(part, more, [0] * 3, outs, caps[:2] + [caps[2] - 1])
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    for b in (3, 4, 6):                                              # the twins never saw the refused calls
        _same([rows[b].push(x[3000:3400 + b], True)], [twins[b].push(x[3000:3400 + b], True)])
        assert rows[b].n_out == twins[b].n_out


# ---- 3. fq3_tsm_push_group against single pushes ----------------------------------------------------------------------------------
def test_tsm_group_equals_single_pushes():
    x = _speech()
    E = x[:0]
    speeds = (500, 1250, 2000, 4000)
    rows, twins = [_Tsm(24000, p) for p in speeds], [_Tsm(24000, p) for p in speeds]
    before = [[x[0:100]], [x[200:5200]], [x[300:15660], x[15660:16000]], [x[400:8400]]]      # row 0: below one hop, before segment 0
    for r, t, parts in zip(rows, twins, before):
        for part in parts:
            _same([r.push(part)], [t.push(part)])
    new = [x[100:239], x[5200:20560], x[16000:16777], x[8400:23760]]                           # row 0 stays below Hs = 240
    _same(_group(rows, new, [0] * 4), [t.push(n) for t, n in zip(twins, new)])
    # reordered; row 3 ends in the group, row 1 gets one sample, row 2 nothing, row 0 its first segments
    order, new, fin = [3, 1, 0, 2], [x[23760:23999], x[20560:20561], x[239:15599], E], [1, 0, 0, 0]
    _same(_group([rows[b] for b in order], new, fin, lead=0), [twins[b].push(n, bool(f)) for b, n, f in zip(order, new, fin)])
    new = [x[15599:15899], x[20561:21561]]                           # ragged short pushes, mid-stream
    _same(_group(rows[:2], new, [0, 0]), [t.push(n) for t, n in zip(twins[:2], new)])
    for b in (0, 1, 2):                                              # the tails by single pushes
        _same([rows[b].push(x[30000:30500 + b], True)], [twins[b].push(x[30000:30500 + b], True)])
    assert [r.n_out for r in rows] == [t.n_out for t in twins]
    # limits, as for the other stage
    rc, _n = _raw_group([rows[3], rows[0]], [E, E], [0, 0], [None, None], [0, 0])
    assert rc == ESTATE
    a, b8 = _Tsm(24000, 1250), _Tsm(8000, 1250)
    out = torch.empty(4096, dtype=torch.float32, device="cuda")
    assert _raw_group([a, b8], [x[:1000], x[:1000]], [0, 0], [out.data_ptr(), out.data_ptr() + 8192], [2048, 2048])[0] == EINVAL
    assert _raw_group([a, a], [x[:1000], x[:1000]], [0, 0], [out.data_ptr(), out.data_ptr() + 8192], [2048, 2048])[0] == EINVAL
    _same([a.push(x[:3000], True)], [_Tsm(24000, 1250).push(x[:3000], True)])


# ---- 4. audio_out.push_group ------------------------------------------------------------------------------------------------------
def test_python_push_group_mixed_specs():
    x = _speech()
    specs = [ao.AudioOutSpec(16000, "s16"), ao.AudioOutSpec(8000, "mulaw", 1.25), ao.AudioOutSpec(24000, "flac"), ao.AudioOutSpec(None, "f32", 0.8),
             ao.AudioOutSpec(8000, "mulaw")]
    rows, twins = [ao.AudioOut(s, 24000, "cuda") for s in specs], [ao.AudioOut(s, 24000, "cuda") for s in specs]
    hosts, htwins = [ao.AudioOut(s, 24000, "cuda") for s in specs], [ao.AudioOut(s, 24000, "cuda") for s in specs]
    pushes = [([x[0:15360], x[100:7001], x[200:15560], x[300:5077], x[400:1401]], [False] * 5),
              ([x[15360:15361], None, x[15560:20000], x[5077:20437], x[1401:9000]], [False, False, False, True, False]),
              ([None, x[7001:9000], x[20000:20100], None, None], [True, True, True, False, True])]
    flac_bytes, s16 = [], []
    for k, (pcms, finals) in enumerate(pushes):
        live = [b for b in range(5) if not (k == 2 and b == 3)]      # row 3 ended in the second call
        got = ao.push_group([rows[b] for b in live], [pcms[b] for b in live], [finals[b] for b in live])
        want = [twins[b].push(pcms[b], finals[b]) for b in live]
        torch.cuda.synchronize()
        _same(got, want)
        flac_bytes.append(got[live.index(2)].cpu().numpy())
        hgot = ao.push_group_host([hosts[b] for b in live], [pcms[b] for b in live], [finals[b] for b in live])
        hwant = [htwins[b].push_host(pcms[b], finals[b]) for b in live]
        for g, w in zip(hgot, hwant):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        for r, t in zip(rows + hosts, twins + htwins):
            assert (r.n_in, r.n_mid, r.n_samples, r.n_out, r.finished) == (t.n_in, t.n_mid, t.n_samples, t.n_out, t.finished)
    with pytest.raises(_lib.Fq3Error):
        ao.push_group(rows[:2], [x[:4], x[:4]], [False, False])      # finished stages
    with pytest.raises(ValueError):
        ao.push_group([twins[0], twins[0]], [None, None], [False, False])
    # the flac row's bytes decode to the s16 samples of its stream
    pcm = torch.cat([x[200:15560], x[15560:20000], x[20000:20100]])
    want16 = ao.AudioOut(ao.AudioOutSpec(24000, "s16"), 24000, "cuda").push(pcm, final=True).cpu().numpy()
    y, info = R.decode(rows[2].header() + np.concatenate(flac_bytes).tobytes())
    assert np.array_equal(np.asarray(y, dtype=np.int16), want16)
    # 40 rows of one design take two calls of the library
    many, mtw = [ao.AudioOut(specs[1], 24000, "cuda") for _ in range(40)], [ao.AudioOut(specs[1], 24000, "cuda") for _ in range(40)]
    pcms = [x[b:b + 3000 + 7 * b] for b in range(40)]
    _same(ao.push_group(many, pcms, [True] * 40), [t.push(p, True) for t, p in zip(mtw, pcms)])


# ---- 5. the batch entry points' output= --------------------------------------------------------------------------------------------
def test_batch_entry_points_take_output():
    m = _tiny_model()
    texts = ["One.", "A second, longer line to speak.", "Three words here."]
    a, b = ao.AudioOutSpec(8000, "mulaw", 1.25), ao.AudioOutSpec(None, "flac")
    kw = dict(temperature=0.9, top_k=20, repetition_penalty=1.05, min_new_tokens=10, max_new_tokens=22)
    seed = 40

    def batch_stream(output=None):
        ev = {i: [] for i in range(3)}
        extra = {} if output is None else dict(output=output)
        for i, arr, sr, tm in m.generate_custom_voice_batch_streaming(texts, "bob", "English", non_streaming_mode=False, lanes=3, chunk_size=4,
                                                                       seeds=seed, **extra, **kw):
            ev[i].append((np.asarray(arr).copy(), sr, bool(tm["is_final"])))
        return ev

    def single_stream(i, spec):
        with m.seeded(seed + i), m.audio_output(spec.sample_rate, spec.encoding, spec.speed):
            return [(np.asarray(arr).copy(), sr) for arr, sr, _tm in
                    m.generate_custom_voice_streaming(texts[i], "bob", "English", non_streaming_mode=False, chunk_size=4, **kw)]

    def check_streaming():
        plain, got = batch_stream(), batch_stream([a, b, None])
        for i, spec in ((0, a), (1, b)):
            want = single_stream(i, spec)
            cat, wcat = np.concatenate([e[0] for e in got[i]]), np.concatenate([w[0] for w in want])
            assert cat.dtype == wcat.dtype and np.array_equal(cat, wcat), (i, len(cat), len(wcat))
            assert all(e[1] == spec.out_rate(24000) for e in got[i]) and all(w[1] == spec.out_rate(24000) for w in want)
        assert got[0][0][0].dtype == np.uint8 and got[1][0][0][:4].tobytes() == b"fLaC"
        assert len(got[2]) == len(plain[2])                          # the row without a spec: today's float32 chunks
        for e, p in zip(got[2], plain[2]):
            assert e[0].dtype == np.float32 and e[1] == 24000 and np.array_equal(e[0], p[0])
        for i in range(3):
            assert [e[2] for e in got[i]] == [False] * (len(got[i]) - 1) + [True], i       # is_final: once, on the last event

    def check_full():
        spec = ao.AudioOutSpec(16000, "s16", 0.8)
        plain = m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=seed, **kw)
        got = m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=seed, output=spec, **kw)
        flac = m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, seeds=seed, output=[None, b, None], **kw)
        for i, ((w, sr), (g, gsr)) in enumerate(zip(plain, got)):
            want = ao.AudioOut(spec, 24000, "cuda").push_host(torch.from_numpy(w[0]).cuda(), final=True)
            assert sr == 24000 and gsr == 16000 and g[0].dtype == want.dtype and np.array_equal(g[0], want), i
        assert np.array_equal(flac[0][0][0], plain[0][0][0]) and flac[0][1] == 24000 and flac[1][1] == 24000
        y, info = R.decode(flac[1][0][0].tobytes())                  # a whole file: the header carries the sample count
        want16 = ao.AudioOut(ao.AudioOutSpec(None, "s16"), 24000, "cuda").push_host(torch.from_numpy(plain[1][0][0]).cuda(), final=True)
        assert info["total"] == len(want16) and np.array_equal(y, want16)

    check_streaming()
    check_full()
    with m.fixed_gain(6.0), m.limiter():
        check_streaming()
        check_full()
    with m.audio_output(16000, "s16"):
        with pytest.raises(ValueError, match="output="):
            m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, output=a, **kw)
        with pytest.raises(ValueError, match="batch entry points"):
            m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, **kw)
    with pytest.raises(ValueError):
        m.generate_custom_voice_batch(texts, "bob", "English", lanes=3, output=[a, b], **kw)
