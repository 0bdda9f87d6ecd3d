"""GPU: the seeded-noise kernels alone, on caller-owned buffers, against the NumPy contract of tests/_noise_ref.py
(DESIGN.md section 4.12): the raw Philox words must be exact; the variates within 1 ulp of their storage type with at most 1 element
in 10^5 not identical (a correctly rounded-to-under-1-ulp fp64 logarithm changes the fp32 rounding with probability about 2^-28: the
cap only keeps a wrong transform from hiding).  Guard rows around every ring and the rows outside the written range stay intact."""
import ctypes as C

import numpy as np
import pytest
import torch

import _noise_ref as R

pytestmark = pytest.mark.gpu

from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_weights

DTYPES = [torch.float32, torch.bfloat16]
SENT = -7.0            # exact in bf16 and fp32; no variate is negative
GUARD = 2              # sentinel rows before and after every ring


@pytest.fixture(scope="module")
def engines():
    from fq3hip.engine import Fq3Engine
    cfg = tiny_test_config()
    return {dt: Fq3Engine(cfg, synth_weights(cfg, 0, dt), device="cuda", dtype=dt, max_seq_len=32, max_frames=8) for dt in DTYPES}


def _dims(eng):
    return eng.cfg.talker.vocab_size, eng.cfg.num_code_groups - 1, eng.cfg.predictor.vocab_size


def _bits(t: torch.Tensor) -> np.ndarray:
    """Storage bit patterns as int64 (positive finite values of one sign order like their bit patterns)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    return t.view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF


def _ref_bits(x32: np.ndarray, dtype) -> np.ndarray:
    if dtype == torch.bfloat16:
        return R.to_bf16_bits(x32).astype(np.int64)
    return np.asarray(x32, np.float32).view(np.uint32).astype(np.int64)


class Ring:
    """A lane's two rings inside guarded buffers, with the expectation kept beside them."""

    def __init__(self, eng, ring_frames, talker=True, pred=True, offset=0):
        V, G1, Vp = _dims(eng)
        self.eng, self.R, self.dims = eng, ring_frames, (V, G1, Vp)
        rows = ring_frames + 2 * GUARD

        def make(width):
            # `offset` elements off the allocation's alignment: the element-wise store path
            flat = torch.full((rows * width + offset,), SENT, dtype=eng.dtype, device="cuda")
            buf = flat[offset:].view(rows, width)
            return flat, buf, buf[GUARD:GUARD + ring_frames]
        self.t_flat, self.t_buf, self.tn = make(V) if talker else (None, None, None)
        self.p_flat, self.p_buf, pn = make(G1 * Vp) if pred else (None, None, None)
        self.pn = pn.view(ring_frames, G1, Vp) if pred else None
        self.want_t = np.full((rows, V), SENT, np.float32)
        self.want_p = np.full((rows, G1, Vp), SENT, np.float32)

    def expect(self, seed, first_frame, n_frames):
        V, G1, Vp = self.dims
        for j in range(n_frames):
            f = first_frame + j
            self.want_t[GUARD + f % self.R] = R.talker_row(seed, f, V)
            self.want_p[GUARD + f % self.R] = R.pred_rows(seed, f, G1, Vp)

    def check(self, what):
        """-> (elements compared, elements not identical); asserts 1 ulp, sentinels intact."""
        total = diff = 0
        for buf, flat, want in ((self.t_buf, self.t_flat, self.want_t), (self.p_buf, self.p_flat, self.want_p)):
            if buf is None:
                continue
            got, ref = _bits(buf).reshape(-1), _ref_bits(want.reshape(-1), self.eng.dtype)
            sent = want.reshape(-1) == SENT
            assert np.array_equal(got[sent], ref[sent]), f"{what}: a guard row or a row outside the written range was touched"
            d = np.abs(got[~sent] - ref[~sent])
            assert d.size == 0 or d.max() <= 1, f"{what}: {int((d > 1).sum())} elements beyond 1 ulp (max {int(d.max())} ulp)"
            total += d.size
            diff += int((d != 0).sum())
            lead = _bits(flat)[:flat.numel() - buf.numel()]
            assert (lead == _ref_bits(np.full(1, SENT, np.float32), self.eng.dtype)[0]).all(), f"{what}: the elements before the buffer were touched"
        return total, diff


def _cap(total, diff, what):
    print(f"{what}: {diff} of {total} elements not identical to the reference")
    assert diff * 100000 <= total, f"{what}: {diff} of {total} elements differ from the reference (cap: 1 in 10^5)"


def test_words_exact():
    from fq3hip import _lib as L
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    bad = []
    for V in (1, 7, 8, 1280, 1283):
        for frame in (0, 1, 2 ** 32 - 1):
            for slot in (0, 1, 15, 0xFFFFFFFF):
                for seed in (0, 1234, 2 ** 64 - 1):
                    out = torch.full((V + 8,), -1, dtype=torch.int32, device="cuda")
                    L.check(lib.fq3_noise_words(seed, frame, slot, V, out.data_ptr(), stream))
                    got = out.cpu().numpy().view(np.uint32)
                    if not (np.array_equal(got[:V], R.words(seed, frame, slot, V)) and (got[V:] == 0xFFFFFFFF).all()):
                        bad.append((V, frame, slot, seed))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("ring_frames,first_frame,n_frames,talker,pred,offset", [
    (16, 13, 7, True, True, 0),           # wraps
    (64, 0, 64, True, True, 0),           # a whole ring of the product's size
    (64, 1_000_003, 64, True, True, 0),   # a whole ring from a late frame: starts inside the ring
    (16, 5, 1, True, True, 0),
    (16, 3, 0, True, True, 0),            # nothing to write
    (16, 13, 7, True, False, 0),          # talker ring only
    (16, 13, 7, False, True, 0),          # predictor ring only
    (16, 2, 16, True, True, 1),           # rings one element off 16-byte alignment: element-wise stores
    (8, 2 ** 32 - 9, 8, True, True, 0),   # the last frames a 32-bit counter can name
], ids=["wrap", "ring64", "ring64_late", "one_row", "no_row", "talker_only", "pred_only", "misaligned", "frame_max"])
def test_fill_one_lane(dtype, ring_frames, first_frame, n_frames, talker, pred, offset, engines):
    eng = engines[dtype]
    seed = 0x9E3779B97F4A7C15 ^ first_frame
    r = Ring(eng, ring_frames, talker, pred, offset)
    eng.noise_fill(r.tn, r.pn, seed, first_frame, n_frames, ring_frames)
    r.expect(seed, first_frame, n_frames)
    _cap(*r.check("fill"), f"fill ring {ring_frames} first {first_frame} n {n_frames} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("lanes", [1, 3, 33])
def test_fill_many_lanes_one_call(dtype, lanes, engines):
    """Distinct seeds, first frames and row counts per lane in ONE call; 33 lanes take more than one launch (32 rings per descriptor).
    Lanes 1 and 2 of a call name no talker / no predictor ring."""
    from fq3hip.engine import Fq3Engine
    eng = engines[dtype]
    ring_frames = 8
    rings, items = [], []
    for i in range(lanes):
        r = Ring(eng, ring_frames, talker=i % 7 != 1, pred=i % 7 != 2)
        seed, first, n = (2 ** 64 - 1 - i * 0x1234567) if i % 2 else 77 + i, 5 * i + (61 if i == 4 else 0), 1 + i % 4
        items.append((eng, r.tn, r.pn, seed, first, n))
        r.expect(seed, first, n)
        rings.append(r)
    Fq3Engine.noise_fill_many(items, ring_frames)
    total = diff = 0
    for i, r in enumerate(rings):
        t, d = r.check(f"lane {i} of {lanes}")
        total, diff = total + t, diff + d
    _cap(total, diff, f"{lanes} lanes {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_split_calls_lane_slot_and_ring_size_do_not_matter(dtype, engines):
    """Bit for bit: two calls that split a range equal one call; the same (seed, frame) in another lane slot of a call and in a ring of
    another size gives the same rows."""
    from fq3hip.engine import Fq3Engine
    eng = engines[dtype]
    seed, first, n = 424242, 29, 11
    one, two = Ring(eng, 16), Ring(eng, 16)
    eng.noise_fill(one.tn, one.pn, seed, first, n, 16)
    eng.noise_fill(two.tn, two.pn, seed, first, 4, 16)
    eng.noise_fill(two.tn, two.pn, seed, first + 4, n - 4, 16)
    assert torch.equal(one.t_buf, two.t_buf) and torch.equal(one.p_buf, two.p_buf)
    # lane slot 2 of a three-lane call, ring of 24 rows
    other = [Ring(eng, 24) for _ in range(3)]
    Fq3Engine.noise_fill_many([(eng, r.tn, r.pn, s, f, n) for r, s, f in zip(other, (1, 2, seed), (0, 7, first))], 24)
    for j in range(n):
        f = first + j
        assert torch.equal(one.tn[f % 16], other[2].tn[f % 24]) and torch.equal(one.pn[f % 16], other[2].pn[f % 24]), f"frame {f}"
    # and it is not the trivial identity: a neighbouring seed differs
    assert not torch.equal(other[0].tn[0], other[1].tn[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_first_token_row(dtype, engines):
    eng = engines[dtype]
    V = _dims(eng)[0]
    buf = torch.full((3, V), SENT, dtype=dtype, device="cuda")
    eng.noise_first(1234, buf[1])
    got, want = _bits(buf), np.full((3, V), SENT, np.float32)
    want[1] = R.first_row(1234, V)
    d = np.abs(got - _ref_bits(want.reshape(-1), dtype).reshape(3, V))
    assert d.max() <= 1 and (d[0] == 0).all() and (d[2] == 0).all()
    _cap(V, int((d != 0).sum()), f"first-token row {dtype}")
    if dtype == torch.float32:
        assert np.array_equal(buf[1, :4].cpu().numpy(), R.first_row(1234, 4))


def test_errors_are_einval_and_launch_nothing(engines):
    from fq3hip import _lib as L
    eng = engines[torch.float32]
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    good, other = Ring(eng, 16), Ring(eng, 16)

    def ring(r, n_frames, first=0):
        return L.NoiseRing(r.tn.data_ptr(), r.pn.data_ptr(), 99, first, n_frames)
    arr = lambda *rs: (L.NoiseRing * len(rs))(*rs)
    cases = {
        "NULL rings with n > 0": lambda: lib.fq3_noise_fill(eng.ctx, None, 1, 16, stream),
        "n_frames above the ring": lambda: lib.fq3_noise_fill(eng.ctx, arr(ring(good, 16), ring(other, 17)), 2, 16, stream),
        "negative n_frames": lambda: lib.fq3_noise_fill(eng.ctx, arr(ring(good, 16), ring(other, -1)), 2, 16, stream),
        "negative n": lambda: lib.fq3_noise_fill(eng.ctx, arr(ring(good, 16)), -1, 16, stream),
        "ring_frames 0": lambda: lib.fq3_noise_fill(eng.ctx, arr(ring(good, 0)), 1, 0, stream),
        "a context without a config": lambda: lib.fq3_noise_fill(None, arr(ring(good, 16)), 1, 16, stream),
        "first: NULL out": lambda: lib.fq3_noise_first(eng.ctx, 1, None, stream),
        "first: NULL context": lambda: lib.fq3_noise_first(None, 1, good.tn.data_ptr(), stream),
        "words: NULL out": lambda: lib.fq3_noise_words(1, 0, 0, 8, None, stream),
        "words: V 0": lambda: lib.fq3_noise_words(1, 0, 0, 0, good.tn.data_ptr(), stream),
    }
    for what, call in cases.items():
        assert call() == L.FQ3_EINVAL, what
        assert lib.fq3_last_error()
    torch.cuda.synchronize()
    for r in (good, other):                      # all or nothing: the valid first entry of a refused call was not written either
        assert r.check("after the refused calls") == (0, 0)
    assert lib.fq3_noise_fill(eng.ctx, None, 0, 16, stream) == L.FQ3_OK          # nothing to do is not an error
    with pytest.raises(ValueError):
        eng.noise_fill(good.tn[:8], good.pn, 1, 0, 16, 16)                      # the Python wrapper checks the rings' sizes
