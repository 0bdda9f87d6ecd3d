"""CPU: incremental text without a device -- the three entry points are exported and bound and refuse NULL / bad ranges before any
HIP call; TextFeeder never releases half a word and loses nothing; the generator's gate never queues a frame before its text row and
refills the noise rings once per NOISE_RING launched frames.

State errors (FQ3_ESTATE: before fq3_decode_begin, table not open, no prompt weights) need a context, and a context needs a device:
tests/test_gpu_text_stream.py::test_state_and_range_errors checks them."""
import ctypes
import math
import os
import random
import threading
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faster-qwen3-tts_amd", "lib", "libfq3hip.so")
NEW = ("fq3_decode_text_open", "fq3_decode_text_append", "fq3_decode_text_rows", "fq3_decode_text_read")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def test_symbols_exported_and_bound(lib):
    from fq3hip import _lib
    hdr = open(os.path.join(ROOT, "include", "fq3hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert f"int {n}(" in hdr, n
    lib.fq3_abi_version.restype = ctypes.c_int
    assert lib.fq3_abi_version() == 5                       # additive: the ABI version stays


def test_null_and_range_errors_without_a_device(lib):
    for n in NEW:
        getattr(lib, n).restype = ctypes.c_int
    rows, closed = ctypes.c_int(-7), ctypes.c_int(-7)
    ids = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    assert lib.fq3_decode_text_open(None, 16, None) == -1
    assert lib.fq3_decode_text_open(None, 0, None) == -1
    assert lib.fq3_decode_text_open(None, -5, None) == -1
    assert lib.fq3_decode_text_append(None, ids, 4, 0, None) == -1
    assert lib.fq3_decode_text_append(None, None, 0, 1, None) == -1
    assert lib.fq3_decode_text_append(None, ids, -1, 0, None) == -1
    assert lib.fq3_decode_text_rows(None, ctypes.byref(rows), ctypes.byref(closed)) == -1
    assert (rows.value, closed.value) == (-7, -7)           # nothing is written on an error
    assert lib.fq3_decode_text_read(None, 0, 1, None, None) == -1
    lib.fq3_last_error.restype = ctypes.c_char_p
    assert b"null" in lib.fq3_last_error()


def test_engine_and_model_surface():
    from fq3hip.engine import Fq3Engine
    from fq3hip.model import FasterQwen3TTS
    import faster_qwen3_tts
    for n in ("decode_text_open", "decode_text_append", "decode_text_rows", "decode_poll_state"):
        assert callable(getattr(Fq3Engine, n))
    for n in ("stream_custom_voice", "stream_voice_design", "stream_voice_clone"):
        assert callable(getattr(FasterQwen3TTS, n))
    assert faster_qwen3_tts.FasterQwen3TTS is FasterQwen3TTS
    from faster_qwen3_tts.text_stream import TextFeeder, fast_generate_text_streaming      # noqa: F401


TEXT = ("Grüße aus Köln!  The quick brown fox\tjumps over the lazy dog, 你好 世界 -- naïve café, "
        "déjà vu;\nsecond line: 12345 done… end")


def test_feeder_any_cut_gives_the_ids_of_the_whole_text():
    """200 seeded random cuts of a mixed ASCII / multi-byte text: the concatenated ids are the ByteTokenizer ids of the whole text,
    no piece is released before its word is complete, close() releases the tail."""
    from fq3hip.native_model import ByteTokenizer
    from fq3hip.text_stream import TextFeeder
    tok = ByteTokenizer(512)
    body = lambda s: tok(s)[3:-5]
    whole = body(TEXT)
    rng = random.Random(2024)
    for trial in range(200):
        f = TextFeeder(body)
        got, at, fed = [], 0, ""
        while at < len(TEXT):
            n = rng.choice((1, 1, 2, 3, 5, 8, 13, 40))
            piece = TEXT[at:at + n]
            at += n
            fed += piece
            f.feed(piece)
            ids, closed = f.take()
            assert not closed
            got += ids
            out = "".join(f.released)
            assert fed.startswith(out)
            # what has been released ends where a word ends: the next character the feeder has SEEN is whitespace
            if out:
                assert len(out) < len(fed) and fed[len(out)].isspace(), (trial, out[-10:], fed[len(out):len(out) + 3])
            # and nothing complete is held back: the held tail has no whitespace behind its first character
            assert not any(ch.isspace() for ch in fed[len(out) + 1:]), (trial, fed[len(out):])
            assert got == body(out)
        assert got != whole                                  # the last word is still held
        f.close()
        ids, closed = f.take()
        assert closed and got + ids == whole, trial
        assert "".join(f.released) == TEXT
        f.close()                                            # idempotent
        with pytest.raises(ValueError):
            f.feed("more")


def test_feeder_blocks_until_fed_or_closed():
    from fq3hip.text_stream import TextFeeder
    f = TextFeeder()
    assert f.take() == ([], False)
    assert f.take(block=True, timeout=0.05) == ([], False)
    threading.Timer(0.05, lambda: f.feed_ids([5, 6, 7])).start()
    t0 = time.time()
    assert f.take(block=True, limit=1) == ([5], False) and time.time() - t0 < 5
    assert f.t_first is not None
    assert f.take(block=True) == ([6, 7], False)
    threading.Timer(0.05, f.close).start()
    assert f.take(block=True) == ([], True)
    with pytest.raises(ValueError):
        TextFeeder().feed("no tokeniser here ")


class _StubEngine:
    """Records the order of appends and launches."""

    def __init__(self):
        self.rows, self.closed, self.frames, self.log = 0, False, 0, []

    def decode_text_append(self, ids, final=False):
        assert not self.closed, "append after the table was closed"
        self.rows += len(ids)
        self.closed = bool(final)
        self.log.append(("append", list(ids), bool(final)))

    def decode_frames(self, k):
        assert k > 0
        for g in range(self.frames, self.frames + k):
            assert g < self.rows or self.closed, f"frame {g} launched with {self.rows} rows and the table open"
        self.frames += k
        self.log.append(("frames", k))


@pytest.mark.parametrize("frames,n_ids", [(150, 149), (150, 40), (64, 200), (130, 129), (7, 0)])
def test_gate_never_launches_a_frame_before_its_row(frames, n_ids):
    """The host gate against a stub engine, with a producer on another thread and with a starved single-threaded one: no frame g is
    launched before row g exists (or the table is closed), every id arrives once and in order, tts_eos closes the table, and the
    noise rings are refilled ceil(frames / NOISE_RING) times."""
    from fq3hip.generate import NOISE_RING
    from fq3hip.text_stream import TextFeeder, TextSession
    EOS = 9999
    ids = list(range(100, 100 + n_ids))
    for mode in ("thread", "up front", "chunked targets"):
        eng, f, refills = _StubEngine(), TextFeeder(), []
        sess = TextSession(eng, f, EOS, frames + 1, refill=lambda e, tn, pn: refills.append(eng.frames))
        if mode == "thread":
            rng = random.Random(frames * 1000 + n_ids)

            def produce():
                at = 0
                while at < len(ids):
                    n = rng.randint(1, 11)
                    f.feed_ids(ids[at:at + n])
                    at += n
                    if rng.random() < 0.3:
                        time.sleep(0.001)
                f.close()
            th = threading.Thread(target=produce, daemon=True)
            th.start()
            assert sess.pump(frames, block=True) == frames
            th.join(10)
        elif mode == "up front":
            f.feed_ids(ids)
            f.close()
            assert sess.pump(frames, block=True) == frames
        else:
            # the generator's pattern: a blocking pump per chunk and a non-blocking look-ahead, ids trickling in between
            at, target = 0, 0
            while sess.issued < frames:
                target = min(frames, target + 12)
                got = sess.pump(target, block=False)
                assert got <= target
                while sess.issued < target:
                    if at < len(ids):
                        f.feed_ids(ids[at:at + 5])
                        at += 5
                    else:
                        f.close()
                    sess.pump(target, block=False)
        assert eng.frames == frames and sess.issued == frames
        appended = [i for kind, *rest in eng.log if kind == "append" for i in rest[0]]
        want = (ids + [EOS])[:frames + 1]                    # rows beyond the capacity (max_frames + 1) cannot be read: dropped
        assert appended == want[:len(appended)] and (eng.closed or len(appended) == len(want)), (mode, len(appended))
        if n_ids < frames:
            assert appended == ids + [EOS] and eng.closed
        assert len(refills) == math.ceil(frames / NOISE_RING) == sess.refills, (mode, refills)
        assert refills == [k * NOISE_RING for k in range(len(refills))]      # each at its ring boundary, before the frame that reads it


def test_gate_non_blocking_pump_returns_when_starved():
    from fq3hip.text_stream import TextFeeder, TextSession
    eng, f = _StubEngine(), TextFeeder()
    sess = TextSession(eng, f, 1, 50, refill=lambda *a: None)
    assert sess.pump(12, block=False) == 0 and eng.log == []
    f.feed_ids([7, 8, 9])
    assert sess.pump(12, block=False) == 3
    assert sess.pump(12, block=False) == 3
    f.close()
    assert sess.pump(12, block=False) == 12 and eng.closed
    assert eng.log == [("append", [7, 8, 9], False), ("frames", 3), ("append", [1], True), ("frames", 9)]


def test_cli_text_stdin_flag():
    from fq3hip.cli import build_parser
    a = build_parser().parse_args(["custom", "--text-stdin", "--speaker", "bob", "--output", "o.wav"])
    assert a.text_stdin and a.text is None
    a = build_parser().parse_args(["design", "--text", "hi", "--instruct", "calm", "--output", "o.wav"])
    assert not a.text_stdin and a.text == "hi"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["clone", "--text-stdin", "--output", "o.wav"])
