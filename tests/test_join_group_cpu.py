"""CPU: the host half of the group form of the segment join: the symbol and its binding, the ABI version, the
range checks that are answered before any HIP call (there is no GPU here, so an answer at all shows where they sit), the ordered set
over scripted joins, the signatures of the four many-text entry points, and the CLI.

The per-row checks against an object's state need objects, and fq3_join_create allocates device memory: they are left to
tests/test_gpu_join_group.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from fq3hip import _lib
from fq3hip import long_form as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fq3_join_push_group"


def test_symbol_and_binding():
    lib = _lib.load()
    ptrs, i64s, ints = C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    res, got = _lib.SIGNATURES[NAME]
    assert res is C.c_int and got == [ptrs, C.c_int, ptrs, i64s, ints, i64s, ptrs, i64s, ptrs, C.c_void_p]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fq3hip.h")).read(), flags=re.S)
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, hdr).group(1).split(",")
    assert len(declared) == len(got) and declared[1].split() == ["int", "B"] and declared[-1].split() == ["void*", "stream"]
    assert declared[0].split() == ["fq3_join*", "const*", "objs"]
    assert declared[-2].split() == ["int64_t*", "const*", "n_out_dev"]         # host array of device pointers
    assert _lib.FQ3_STAGE_GROUP_MAX == lf.GROUP_MAX == 32
    lib.fq3_abi_version.restype = C.c_int
    assert lib.fq3_abi_version() == 5                                # additive: the version stays


def test_range_checks_come_before_any_hip_call():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    one_p, one_l, one_i = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0), (C.c_int * 1)(0)
    full = [one_p, 1, one_p, one_l, one_i, one_l, one_p, one_l, one_p, None]
    for B in (-1, 33, 1 << 20):
        assert fn(*(full[:1] + [B] + full[2:])) == _lib.FQ3_EINVAL, B
        assert b"32" in lib.fq3_last_error() and NAME.encode() in lib.fq3_last_error()
    for at in (0, 2, 3, 4, 5, 6, 7, 8):                              # every array
        args = list(full)
        args[at] = None
        assert fn(*args) == _lib.FQ3_EINVAL, at
        assert b"null array" in lib.fq3_last_error()
    assert fn(*full) == _lib.FQ3_EINVAL and b"row 0: null object" in lib.fq3_last_error()      # a null object in the array
    assert fn(*([None, 0] + [None] * (len(full) - 2))) == 0          # B == 0: nothing to do


def test_the_same_object_twice_is_refused_before_it_is_read():
    """the duplicate check compares pointers only, so any two equal non-null entries reach it -- here the address of a host buffer
    that is large enough to be read as an object, should the order of the checks ever change"""
    lib = _lib.load()
    fake = (C.c_uint8 * 256)()
    two_p = (C.c_void_p * 2)(C.addressof(fake), C.addressof(fake))
    none_p, two_l, two_i = (C.c_void_p * 2)(None, None), (C.c_int64 * 2)(0, 0), (C.c_int * 2)(0, 0)
    assert getattr(lib, NAME)(two_p, 2, none_p, two_l, two_i, two_l, none_p, two_l, none_p, None) == _lib.FQ3_EINVAL
    assert b"rows 0 and 1 are the same object" in lib.fq3_last_error()


def test_python_group_path_answers_without_a_gpu():
    assert lf.push_group([], [], [], []) == []
    with pytest.raises(ValueError):
        lf.push_group([], [None], [], [])


# ---- the ordered set over scripted joins ---------------------------------------------------------------------------------------
class _Join:
    """a join that lets everything through and notes what it was given"""
    stream = None

    def __init__(self, name):
        self.name, self.pushed = name, []


class _Rounds:
    def __init__(self):
        self.calls = []

    def __call__(self, joins, pcms, ends, pauses):
        assert len(set(map(id, joins))) == len(joins)                # no join twice in one round
        self.calls.append([(j.name, e, p) for j, e, p in zip(joins, ends, pauses)])
        for j, x, e in zip(joins, pcms, ends):
            j.pushed.append((None if x is None else x.tolist(), e))
        return [torch.zeros(0) if x is None else x.clone() for x in pcms]


def _chunk(t, k, i, n=2):
    """n samples that say where they come from: text t, segment k, chunk i"""
    return torch.full((n,), float(100 * t + 10 * k + i))


def _set(n_segments):
    rounds = _Rounds()
    ordered = [lf.OrderedJoin(_Join(t), [7 + k for k in range(n)]) for t, n in enumerate(n_segments)]
    return lf.OrderedJoinSet(ordered, push_group=rounds), rounds


def test_ordered_set_yields_every_text_in_text_order_for_an_interleaved_feed():
    s, rounds = _set([3, 1, 2])
    out = []
    # group 1: text 0 gets chunks of segments 0 AND 1 (1 ends, 0 goes on), text 2 only its segment 1 (waits), text 1 its only chunk
    out.append(s.feed_group([(0, 1, _chunk(0, 1, 0), True), (0, 0, _chunk(0, 0, 0), False), (2, 1, _chunk(2, 1, 0), False),
                             (1, 0, _chunk(1, 0, 0), True)]))
    assert [(t, k, y.tolist(), e) for t, k, y, e in out[0]] == [(0, 0, _chunk(0, 0, 0).tolist(), False), (1, 0, _chunk(1, 0, 0).tolist(), True)]
    assert rounds.calls == [[(0, 0, 0), (1, 2, 0)]]                  # one round, one group call: texts 0 and 1
    assert s.ordered[2].max_waiting == 1 and s.ordered[0].max_waiting == 1
    # group 2: segment 0 of text 0 ends -> its waiting segment 1 is flushed behind it (a second round); text 2 still waits; two chunks
    # of text 0's segment 2 arrive as well, the second one final: they go out as ONE push in a third round
    out.append(s.feed_group([(0, 0, _chunk(0, 0, 1), True), (2, 1, _chunk(2, 1, 1), True), (0, 2, _chunk(0, 2, 0), False),
                             (0, 2, _chunk(0, 2, 1), True)]))
    assert [(t, k, e) for t, k, _y, e in out[1]] == [(0, 0, False), (0, 1, False), (0, 2, True)]
    assert out[1][2][2].tolist() == _chunk(0, 2, 0).tolist() + _chunk(0, 2, 1).tolist()
    assert rounds.calls[1:] == [[(0, 1, 7)], [(0, 1, 8)], [(0, 2, 0)]]      # end 1 with the segment's pause, end 2 without one
    # group 3: text 2's segment 0 arrives whole: both its segments leave, the waiting chunks of segment 1 as one push
    out.append(s.feed_group([(2, 0, _chunk(2, 0, 0), True)]))
    assert [(t, k, e) for t, k, _y, e in out[2]] == [(2, 0, False), (2, 1, True)]
    assert out[2][1][2].tolist() == _chunk(2, 1, 0).tolist() + _chunk(2, 1, 1).tolist()
    assert s.finished and s.rounds == len(rounds.calls) == 6
    # every text's pieces, in the order they left, are its chunks in text order
    for t, n in enumerate([3, 1, 2]):
        ks = [k for group in out for tt, k, _y, _e in group if tt == t]
        assert ks == sorted(ks) and set(ks) == set(range(n))
        vals = [v for group in out for tt, _k, y, _e in group if tt == t for v in y.tolist()]
        assert vals == sorted(vals) and len(vals) == 2 * [5, 1, 3][t]       # every chunk that was fed, once
    assert [e for _x, e in s.ordered[0].join.pushed] == [0, 1, 1, 2]


def test_ordered_set_takes_one_push_per_text_and_round():
    """four texts of one segment each fed together: ONE group call of four rows"""
    s, rounds = _set([1, 1, 1, 1])
    got = s.feed_group([(t, 0, _chunk(t, 0, 0), True) for t in (3, 1, 0, 2)])
    assert [t for t, _k, _y, _e in got] == [0, 1, 2, 3] and all(e for _t, _k, _y, e in got)
    assert len(rounds.calls) == 1 and [name for name, _e, _p in rounds.calls[0]] == [0, 1, 2, 3]


def test_ordered_set_argument_errors_move_nothing():
    s, rounds = _set([2, 1])
    with pytest.raises(ValueError):
        s.feed_group([(0, 0, _chunk(0, 0, 0), False), (2, 0, None, True)])          # no such text
    with pytest.raises(ValueError):
        s.feed_group([(0, 0, _chunk(0, 0, 0), False), (1, 1, None, True)])          # no such segment
    assert rounds.calls == [] and all(not any(oj._wait) for oj in s.ordered)
    s.feed_group([(0, 0, None, True)])
    with pytest.raises(ValueError):
        s.feed_group([(0, 0, None, True)])                                          # segment 0 of text 0 has ended
    j = _Join("x")
    with pytest.raises(ValueError):
        lf.OrderedJoinSet([lf.OrderedJoin(j, [0]), lf.OrderedJoin(j, [0])])


def test_ordered_set_refuses_a_chunk_behind_a_last_chunk_before_anything_moves():
    s, rounds = _set([2, 1])
    with pytest.raises(ValueError, match="after its last chunk"):      # inside one call ...
        s.feed_group([(1, 0, _chunk(1, 0, 0), True), (0, 0, _chunk(0, 0, 0), True), (0, 1, _chunk(0, 1, 0), True), (0, 1, _chunk(0, 1, 1), False)])
    assert rounds.calls == [] and all(not any(oj._wait) and oj.cur == 0 for oj in s.ordered)
    s.feed_group([(0, 1, _chunk(0, 1, 0), True)])                       # ... and behind a last chunk that still waits
    with pytest.raises(ValueError, match="after its last chunk"):
        s.feed_group([(0, 0, _chunk(0, 0, 0), True), (0, 1, _chunk(0, 1, 1), False)])
    assert rounds.calls == [] and s.ordered[0].cur == 0 and [len(w) for w in s.ordered[0]._wait] == [0, 1]
    got = s.feed_group([(0, 0, _chunk(0, 0, 0), True)])                 # nothing was lost: the stream goes on
    assert [(t, k, e) for t, k, _y, e in got] == [(0, 0, False), (0, 1, True)]


# ---- the public entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", ["generate_long_voice_clone", "generate_long_custom_voice", "generate_long_voice_clone_streaming",
                                    "generate_long_custom_voice_streaming"])
def test_signatures_are_the_single_twins_with_texts_seeds_and_output(single):
    from fq3hip.model import FasterQwen3TTS
    batch = single.replace("_streaming", "") + "_batch" + ("_streaming" if single.endswith("_streaming") else "")
    assert hasattr(FasterQwen3TTS, batch), batch
    one = inspect.signature(getattr(FasterQwen3TTS, single)).parameters
    many = inspect.signature(getattr(FasterQwen3TTS, batch)).parameters
    assert list(many) == ["texts" if n == "text" else n for n in one] + ["seeds", "output"]
    assert many["seeds"].default is None and many["output"].default is None
    for n, p in one.items():
        if n not in ("self", "text"):
            assert many[n].default == p.default and many[n].kind == p.kind, n
    assert inspect.isgeneratorfunction(getattr(FasterQwen3TTS, batch)) == single.endswith("_streaming")


# ---- the CLI: serve --long --lanes N takes the waiting lines through the many-text entry point --------------------------------
def test_cli_serve_long_lines_go_through_the_batch_entry_point(tmp_path):
    from fq3hip import audio_io, cli

    class M:
        sample_rate = 24000

        def __init__(self):
            self.calls = []

        def generate_long_voice_clone_batch(self, texts, lanes=16, long_form=None, seeds=None, **kw):
            self.calls.append(("batch", list(texts), lanes, long_form.max_chars, kw.get("ref_audio")))
            return [([np.full(240 * len(t), 0.1, np.float32)], 24000) for t in texts]

        def generate_long_voice_clone(self, text, lanes=16, long_form=None, **kw):
            self.calls.append(("single", text, lanes, long_form.max_chars))
            return [np.full(240 * len(text), 0.1, np.float32)], 24000
    m = M()
    args = cli.build_parser().parse_args(["serve", "--ref-audio", "r.wav", "--ref-text", "t", "--output-dir", str(tmp_path), "--long",
                                          "--lanes", "2", "--max-chars", "30"])
    cli.cmd_serve(args, model=m, lines=["One. Two.\n", "Three.\n", "Four and more.\n", "quit\n"])
    assert m.calls == [("batch", ["One. Two.", "Three."], 2, 30, "r.wav"), ("single", "Four and more.", 2, 30)]
    for i, text in enumerate(["One. Two.", "Three.", "Four and more."]):
        y, sr = audio_io.read_wav(str(tmp_path / f"out_{i + 1:04d}.wav"))
        assert sr == 24000 and len(y) == 240 * len(text)
    # without --long the lines take the path they took
    assert cli.build_parser().parse_args(["serve", "--ref-audio", "r.wav"]).long is False
