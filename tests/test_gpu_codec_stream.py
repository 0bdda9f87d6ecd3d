"""GPU: the codec's rolling stream states (``fq3_codec_stream_*``).  The samples a stream has produced after any sequence of pushes
are, bit for bit, the one-pass decode of all its codes -- for every split of the frames into pushes, behind a reference prefix, for
lanes of one call that stand at different positions, in all three precisions.  Every comparison is ``torch.equal``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip import _lib as L
from fq3hip.config import tiny_test_config
from fq3hip.weights import synth_weights

PRECISIONS = ["fp32", "bf16", "bf16x2"]


def _tok(cfg, precision, max_frames, normalized=False, **kw):
    from fq3hip.codec import HipSpeechTokenizer
    dt = torch.float32 if precision == "fp32" else torch.bfloat16
    W = synth_weights(cfg, 0, dt, parts=("codec",), **(dict(codec_normalized=True) if normalized else {}))
    return HipSpeechTokenizer(cfg.codec, W, "cuda", max_frames=max_frames, precision=precision, **kw)


def _codes(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.codec.codebook_size, (n, cfg.codec.num_quantizers), generator=g).cuda()


@pytest.fixture(scope="module", params=PRECISIONS)
def tiny(request):
    cfg = tiny_test_config()
    tok = _tok(cfg, request.param, 128)
    assert tok.stream_ctx_max == 48 and cfg.codec.sliding_window == 8
    codes = _codes(cfg, 64, 5)
    yield cfg, tok, codes, tok.decode_tensor(codes).clone()          # the one-pass reference: computed once, never written
    tok.close()


def _stream_all(tok, st, codes, sizes):
    parts, i = [], 0
    for n in sizes:
        want = tok.stream_samples(st.frames, n)
        a = tok.stream_push([st], codes[i:i + n].unsqueeze(0))
        assert a.shape == (1, want), (i, n, a.shape, want)
        parts.append(a[0])
        i += n
    assert i == codes.shape[0]
    return torch.cat(parts)


@pytest.mark.parametrize("sizes", [[1] * 64, [3] * 21 + [1], [8] * 8, [5, 1, 12, 2, 8, 7, 29]], ids=["by1", "by3", "by8", "ragged"])
def test_pushes_concatenate_to_the_one_pass_decode_tiny(tiny, sizes):
    """64 frames in pushes of 1 / 3 / 8 / a ragged list: together they cross rows 2|3 (pre_conv context), 7|8|9 (window) and 47|48|49
    (cached output rows)."""
    _cfg, tok, codes, full = tiny
    st = tok.stream_open()
    assert st.frames == 0
    got = _stream_all(tok, st, codes, sizes)
    assert st.frames == 64
    assert got.shape == full.shape and torch.equal(got, full)
    st.close()


@pytest.mark.parametrize("ref_len", [1, 2, 21, 60])
def test_stream_behind_a_prefix_tiny(tiny, ref_len):
    """a stream that begins behind a reference of 1 / 2 / 21 / 60 frames continues decode(ref + gen) after the reference's samples; the
    prefix object is shared (the stream took a copy) and still decodes bit-identically afterwards"""
    cfg, tok, _codes64, _full = tiny
    ref, gen = _codes(cfg, ref_len, 100 + ref_len), _codes(cfg, 24, 7)
    both = torch.cat([ref, gen])
    full = tok.decode_tensor(both)
    pf = tok.prefix_for(ref)
    assert pf is not None
    st = tok.stream_open(ref)
    assert st.frames == ref_len
    got = _stream_all(tok, st, gen, [8, 8, 8])
    assert st.frames == ref_len + 24
    assert torch.equal(got, full[tok.num_samples(ref_len):])
    assert tok.prefix_for(ref) is pf
    first = tok.num_samples(ref_len + 24) - 8 * cfg.codec.total_upsample
    assert torch.equal(tok.decode_tensor(both, first, prefix=pf), full[first:])
    st.close()


def test_lanes_at_different_positions_and_errors_tiny(tiny):
    """five streams at F = 48, 51, 64, 77, 100 are one class (min(F, 48) = 48): one push of 8 frames for all five equals each pushed
    alone on a twin state, and two calls over equal twin states give equal bits.  Mixed classes, a repeated state, B = 0 and a push past
    the RoPE table return their documented errors; after the table error the state is untouched."""
    cfg, tok, _codes64, _full = tiny
    Fs = [48, 51, 64, 77, 100]
    hist = [_codes(cfg, F, 200 + F) for F in Fs]
    new = torch.stack([_codes(cfg, 8, 300 + F) for F in Fs])

    def advanced():
        out = []
        for h in hist:
            st = tok.stream_open()
            for i in range(0, h.shape[0], 16):
                tok.stream_push([st], h[i:i + 16].unsqueeze(0))
            out.append(st)
        return out
    a, b, c = advanced(), advanced(), advanced()
    assert [s.frames for s in a] == Fs
    ga, gb = tok.stream_push(a, new), tok.stream_push(b, new)
    assert torch.equal(ga, gb)
    for i, st in enumerate(c):
        alone = tok.stream_push([st], new[i:i + 1])
        assert torch.equal(alone[0], ga[i]), Fs[i]
        # ... which is the one-pass decode of that lane's frames
        full = tok.decode_tensor(torch.cat([hist[i], new[i]]))
        assert torch.equal(alone[0], full[tok.num_samples(Fs[i]):]), Fs[i]
    assert [s.frames for s in a] == [F + 8 for F in Fs]

    def code_of(fn):
        with pytest.raises(L.Fq3Error) as e:
            fn()
        return e.value.code
    lo, hi = tok.stream_open(), tok.stream_open()
    tok.stream_push([lo], _codes(cfg, 5, 1).unsqueeze(0))
    for i in range(0, 60, 20):
        tok.stream_push([hi], _codes(cfg, 20, 2 + i).unsqueeze(0))
    two = torch.stack([_codes(cfg, 4, 3), _codes(cfg, 4, 4)])
    assert code_of(lambda: tok.stream_push([lo, hi], two)) == L.FQ3_EINVAL            # min(5, 48) != min(60, 48)
    assert code_of(lambda: tok.stream_push([hi, hi], two)) == L.FQ3_EINVAL            # the same state twice
    assert code_of(lambda: tok.stream_push([], two[:0])) == L.FQ3_EINVAL              # B = 0
    assert (lo.frames, hi.frames) == (5, 60)
    for s in a + b + c + [lo, hi]:
        s.close()


def test_push_past_the_rope_table_is_refused_and_leaves_the_state(tiny):
    cfg, _tok128, _codes64, _full = tiny
    tok = _tok(cfg, _tok128.precision, 128, stream_positions=160)       # a table of max(128, 160) rows
    codes = _codes(cfg, 176, 9)
    full = tok.decode_tensor(codes[:128])                                # (one pass holds max_frames = 128 frames)
    st = tok.stream_open()
    got = [tok.stream_push([st], codes[i:i + 32].unsqueeze(0))[0] for i in range(0, 96, 32)]
    with pytest.raises(RuntimeError, match="passes the RoPE table of 160 rows"):      # FQ3_ETOOLONG (the binding raises it as RuntimeError)
        tok.stream_push([st], codes[96:176].unsqueeze(0))                # 96 + 80 = 176 > 160
    assert st.frames == 96
    got.append(tok.stream_push([st], codes[96:128].unsqueeze(0))[0])     # the next valid push is still exact
    assert st.frames == 128 and torch.equal(torch.cat(got), full)
    # positions beyond max_frames: rows 128 .. 159 of the stream's own table
    twin = tok.stream_open()
    for i in range(0, 128, 64):
        tok.stream_push([twin], codes[i:i + 64].unsqueeze(0))
    x = tok.stream_push([st], codes[128:160].unsqueeze(0))[0]
    y = torch.cat([tok.stream_push([twin], codes[i:i + 8].unsqueeze(0))[0] for i in range(128, 160, 8)])
    assert st.frames == twin.frames == 160 and torch.equal(x, y)
    tok.close()


def test_reset_gives_a_fresh_state(tiny):
    cfg, tok, codes, full = tiny
    ref = _codes(cfg, 21, 121)
    st = tok.stream_open()
    _stream_all(tok, st, codes[:40], [8] * 5)
    st.reset()
    assert st.frames == 0
    assert torch.equal(_stream_all(tok, st, codes, [16] * 4), full)
    st.reset(ref)
    assert st.frames == 21
    fresh = tok.stream_open(ref)
    assert torch.equal(_stream_all(tok, st, codes[:16], [8, 8]), _stream_all(tok, fresh, codes[:16], [8, 8]))
    st.close(), fresh.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pushes_concatenate_to_the_one_pass_decode_real_shapes(precision):
    """the real codec shapes (window 72, head_dim 64): 88 frames in pushes of 8 cross 48 and 71|72"""
    from fq3hip.config import qwen3_tts_0p6b
    cfg = qwen3_tts_0p6b()
    tok = _tok(cfg, precision, 96, normalized=True)
    assert tok.stream_ctx_max == 71
    codes = _codes(cfg, 88, 13)
    full = tok.decode_tensor(codes)
    st = tok.stream_open()
    got = _stream_all(tok, st, codes, [8] * 11)
    assert got.shape == full.shape and torch.equal(got, full)
    tok.close()
