"""CPU: the host half of long-form synthesis (fq3hip/long_form.py): the text splitter, ``LongFormSpec``,
the ordered hand-over, the new public methods' signatures and refusals over a fake model, the CLI flags and the server's
``long_form`` field over scripted models."""
import contextlib
import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest

from fq3hip.long_form import LongFormSpec, OrderedJoin, Segment, split_text
from fq3hip.model import FasterQwen3TTS


def _texts(segs):
    return [s.text for s in segs]


# ---- splitter ---------------------------------------------------------------------------------------------------------------------
def test_sentences_and_terminators():
    segs = split_text("Hello there. How are you? Fine! Well… yes.", max_chars=12)
    assert _texts(segs) == ["Hello there.", "How are you?", "Fine! Well…", "yes."]
    assert [s.pause for s in segs] == ["sentence", "sentence", "sentence", "end"]
    # closing quotes and brackets stay with their sentence; runs of terminators stay together
    assert _texts(split_text('He said "Stop." Then (really?!) Gone... Yes.', 16)) == ['He said "Stop."', "Then (really?!)", "Gone... Yes."]
    # a terminator without whitespace behind it is no break
    assert _texts(split_text("See example.com now. Ok.", 20)) == ["See example.com now.", "Ok."]


def test_decimals_abbreviations_and_initials():
    assert _texts(split_text("Pi is 3.14 and e is 2.71. Next one.", 26)) == ["Pi is 3.14 and e is 2.71.", "Next one."]
    assert _texts(split_text("Dr. Smith met Mrs. Jones vs. Prof. Lee, etc. and left. Done.", 55)) == \
        ["Dr. Smith met Mrs. Jones vs. Prof. Lee, etc. and left.", "Done."]
    assert _texts(split_text("Use a tool, e.g. a saw, i.e. a blade. Then stop.", 40)) == ["Use a tool, e.g. a saw, i.e. a blade.", "Then stop."]
    assert _texts(split_text("J. K. Rowling and St. John wrote it. Mr. X. agreed.", 40)) == ["J. K. Rowling and St. John wrote it.", "Mr. X. agreed."]
    # a number at a sentence's end still ends it
    assert _texts(split_text("It was 1999. Then came 2000.", 15)) == ["It was 1999.", "Then came 2000."]


def test_cjk_terminators_need_no_whitespace():
    segs = split_text("你好。世界！这是测试？好；再见", max_chars=6)
    assert _texts(segs) == ["你好。世界！", "这是测试？", "好；再见"]
    assert _texts(split_text("他说：「好。」然后走了。", 7)) == ["他说：「好。」", "然后走了。"]
    # merged without a space that the text did not have
    assert _texts(split_text("你好。世界！", 40)) == ["你好。世界！"]


def test_paragraph_breaks():
    segs = split_text("First one. Still first.\n\nSecond para.\n \n\t\n\nThird.\nSame para.", 60)
    assert segs == [Segment("First one. Still first.", "paragraph"), Segment("Second para.", "paragraph"), Segment("Third. Same para.", "end")]
    # sentences of different paragraphs are never merged, however short
    assert len(split_text("A.\n\nB.\r\n\r\nC.", 240)) == 3
    assert split_text("", 10) == [] and split_text(" \n\n \t", 10) == []


def test_over_long_sentences():
    # at the last clause mark inside the budget
    segs = split_text("one, two, three, four, five, six, seven, eight, nine, ten, eleven, twelve.", 40)
    assert segs == [Segment("one, two, three, four, five, six, seven,", "clause"), Segment("eight, nine, ten, eleven, twelve.", "end")]
    assert _texts(split_text("alpha beta; gamma delta: epsilon — zeta eta theta", 24)) == ["alpha beta; gamma delta:", "epsilon — zeta eta theta"]
    assert _texts(split_text("一二三，四五六、七八九十一二三四五六", 8)) == ["一二三，四五六、", "七八九十一二三四", "五六"]
    # else at whitespace
    segs = split_text("aaaa bbbb cccc dddd eeee ffff", 12)
    assert _texts(segs) == ["aaaa bbbb", "cccc dddd", "eeee ffff"] and [s.pause for s in segs] == ["clause", "clause", "end"]
    # else hard
    segs = split_text("x" * 25, 10)
    assert _texts(segs) == ["x" * 10, "x" * 10, "x" * 5] and [s.pause for s in segs] == ["clause", "clause", "end"]
    assert _texts(split_text("a" * 15 + " " + "b" * 4, 10)) == ["a" * 10, "aaaaa bbbb"]


def test_merge_budget():
    t = "Aa bb. Cc dd. Ee ff. Gg hh."
    assert _texts(split_text(t, 240)) == [t]
    assert _texts(split_text(t, 13)) == ["Aa bb. Cc dd.", "Ee ff. Gg hh."]         # exactly the budget
    assert _texts(split_text(t, 12)) == ["Aa bb.", "Cc dd.", "Ee ff.", "Gg hh."]
    assert _texts(split_text(t, 20)) == ["Aa bb. Cc dd. Ee ff.", "Gg hh."]          # greedy, left to right


ROUND_TRIP = [
    "Hello world.", "One. Two. Three.", "Dr. Who? Yes, Dr. Who!", "A very long sentence, with clauses; and more: and yet more — the end.",
    "Numbers like 3.14159 and 2.71828 are fine. So is 1,000,000.", "Para one.\n\nPara two.\n\n\nPara three.", "No terminator at all",
    "Trailing spaces.   ", "   Leading spaces.", "Tabs\tand\nnewlines inside. Next\tline.", "Quote: \"Is it?\" she asked. 'Yes.'",
    "Ellipsis… then more... and more.", "Mixed 你好。 English. 世界！", "你好。世界！这是一个测试？好；再见", "e.g. this, i.e. that, etc. and so on.",
    "J. R. R. Tolkien wrote it. C. S. Lewis read it.", "What?! Really?? Yes!!", "A (parenthetical.) Another [bracketed!] one.",
    "word " * 80, "x" * 700, "a, " * 200, "The U.S.A. is big. So is the U.K.", "Version 2.0 is out. Version 3 soon.", "Mr. and Mrs. Smith vs. the world.",
    "Semicolons; are clause marks: so are colons — and dashes.", "Windows\r\n\r\nline ends.\r\nSame para.", "One.\n\n\n\n\nTwo.",
    "「引号。」后面。", "Unicode ellipsis…Next without space.", "St. Petersburg is cold. Prof. X agrees.", "a.b.c.d", "End with number 42.",
    "?", "...", "Hello . World .", "He paid 3.50. She paid 4.", "Title\n\nBody sentence one. Body sentence two!\n\nFooter",
]


@pytest.mark.parametrize("max_chars", [1, 7, 40, 240])
def test_round_trip_budget_and_determinism(max_chars):
    assert len(ROUND_TRIP) >= 36
    for t in ROUND_TRIP:
        segs = split_text(t, max_chars)
        assert segs == split_text(t, max_chars)                                     # deterministic
        assert all(0 < len(s.text) <= max_chars and s.text == s.text.strip() for s in segs), (t, max_chars)
        assert [s.pause for s in segs][-1:] == (["end"] if segs else []) and all(s.pause != "end" for s in segs[:-1])
        joined = " ".join(_texts(segs))
        # every cut lies at whitespace unless a word is longer than the budget or CJK sentences touch: then the join's space is the
        # one difference, so the comparison that always holds ignores whitespace altogether ...
        assert re.sub(r"\s+", "", joined) == re.sub(r"\s+", "", t), (t, max_chars)
        # ... and where every word fits and no CJK mark is glued to its successor, it holds up to runs of whitespace
        if all(len(w) <= max_chars for w in t.split()) and not re.search(r"[。！？；，、…][^\s]", t) and max_chars >= 7:
            assert joined == " ".join(t.split()), (t, max_chars)


# ---- LongFormSpec -----------------------------------------------------------------------------------------------------------------
def test_long_form_spec_defaults_and_validation():
    s = LongFormSpec()
    assert s.max_chars == 240 and s.pause_ms == {"clause": 120, "sentence": 300, "paragraph": 650}
    assert (s.threshold, s.lead_hops, s.tail_hops, s.hold_hops) == (0.005, 2, 5, 100)
    assert [s.pause_samples(p, 24000) for p in ("clause", "sentence", "paragraph", "end")] == [2880, 7200, 15600, 0]
    c = s.join_config(24000)
    assert (c.in_rate, c.lead_hops, c.tail_hops, c.hold_hops) == (24000, 2, 5, 100) and abs(c.threshold - 0.005) < 1e-9
    assert _texts(LongFormSpec(max_chars=6).split("Aa bb. Cc dd.")) == ["Aa bb.", "Cc dd."]
    for bad in (dict(max_chars=0), dict(max_chars=2.5), dict(max_chars=True), dict(threshold=0.0), dict(threshold=1.0), dict(threshold="x"),
                dict(lead_hops=17), dict(lead_hops=-1), dict(hold_hops=401), dict(tail_hops=101), dict(tail_hops=-1), dict(hold_hops=3),
                dict(pause_ms={"clause": 1}), dict(pause_ms={"clause": 1, "sentence": 2, "paragraph": 5001}),
                dict(pause_ms={"clause": -1, "sentence": 2, "paragraph": 3}), dict(pause_ms=[1, 2, 3])):
        with pytest.raises(ValueError):
            LongFormSpec(**bad)
    with pytest.raises(ValueError):
        split_text("abc", 0)
    with pytest.raises(ValueError):
        split_text(None, 10)


# ---- ordered hand-over ------------------------------------------------------------------------------------------------------------
class _FakeJoin:
    """records the pushes; 'joins' by passing the chunk through"""

    def __init__(self):
        self.pushes = []

    def push(self, pcm, end, pause):
        self.pushes.append((pcm, end, pause))
        return pcm


def test_ordered_join_holds_later_segments_back():
    j = _FakeJoin()
    oj = OrderedJoin(j, [10, 20, 0])
    assert [k for k, _y, _e in oj.feed(1, "b0", False)] == []                       # segment 1 is early: it waits
    assert [k for k, _y, _e in oj.feed(2, "c0", True)] == []
    assert [(k, y) for k, y, _e in oj.feed(0, "a0", False)] == [(0, "a0")]          # segment 0 streams as it comes
    assert oj.max_waiting >= 2
    out = oj.feed(0, "a1", True)                                                    # its end releases what waited, in text order
    assert [(k, y, e) for k, y, e in out] == [(0, "a1", False), (1, "b0", False)]
    out = oj.feed(1, "b1", True)
    assert [(k, y, e) for k, y, e in out] == [(1, "b1", False), (2, "c0", True)] and oj.finished
    assert j.pushes == [("a0", 0, 0), ("a1", 1, 10), ("b0", 0, 0), ("b1", 1, 20), ("c0", 2, 0)]
    with pytest.raises(ValueError):
        oj.feed(0, "late", False)


# ---- public interface -------------------------------------------------------------------------------------------------------------
class _Graph:
    def capture(self, **kw):
        pass


def _wrapper(kind="base"):
    inner = SimpleNamespace(speech_tokenizer=SimpleNamespace(sample_rate=24000), tts_model_type=kind, tts_model_size="0b6")
    return FasterQwen3TTS(base_model=SimpleNamespace(model=inner), predictor_graph=_Graph(), talker_graph=_Graph())


def test_new_method_signatures():
    for long, short in (("generate_long_voice_clone", "generate_voice_clone"),
                        ("generate_long_voice_clone_streaming", "generate_voice_clone_streaming"),
                        ("generate_long_custom_voice", "generate_custom_voice"),
                        ("generate_long_custom_voice_streaming", "generate_custom_voice_streaming")):
        a, b = inspect.signature(getattr(FasterQwen3TTS, long)).parameters, inspect.signature(getattr(FasterQwen3TTS, short)).parameters
        names = [n for n in b if n != "parity_mode"]
        assert list(a) == names + ["lanes", "long_form"], long                      # the arguments of the short form, then the two new ones
        assert all(a[n].default == b[n].default for n in names)
        assert a["lanes"].default == 16 and a["long_form"].default is None
    assert inspect.signature(FasterQwen3TTS.generate_long_voice_clone_streaming).parameters["chunk_size"].default == 12
    assert not hasattr(FasterQwen3TTS, "generate_long_voice_design")


def test_voice_design_and_bad_arguments_are_refused_before_any_work():
    w = _wrapper("voice_design")
    with pytest.raises(ValueError, match="voice"):
        w.generate_long_voice_clone("One. Two.", "English")
    with pytest.raises(ValueError, match="voice"):
        next(w.generate_long_voice_clone_streaming("One. Two.", "English"))
    with pytest.raises(ValueError, match="voice"):
        w.generate_long_custom_voice("One. Two.", "vivian", "English")
    with pytest.raises(ValueError, match="voice"):
        next(w.generate_long_custom_voice_streaming("One. Two.", "vivian", "English"))
    b = _wrapper("base")
    for text in ("", "   \n\t"):
        with pytest.raises(ValueError, match="empty"):
            b.generate_long_voice_clone(text, "English")
        with pytest.raises(ValueError, match="empty"):
            next(b.generate_long_voice_clone_streaming(text, "English"))
    with pytest.raises(ValueError, match="LongFormSpec"):
        b.generate_long_voice_clone("Hi.", "English", long_form={"max_chars": 10})
    with pytest.raises(ValueError, match="custom voice"):
        b.generate_long_custom_voice("One. Two.", "vivian", "English")             # a base model has no custom voices
    with pytest.raises(NotImplementedError, match="backend='ggml'"):
        b.generate_long_voice_clone("Hi.", "English", ref_spk="a.spk")
    # the existing refusal of the batch entry points inside audio_output stands
    with b.audio_output(16000, "s16"):
        with pytest.raises(ValueError, match="batch entry points"):
            b.generate_voice_clone_batch(["a"], language="English")


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
class _ScriptedModel:
    sample_rate = 24000

    def __init__(self):
        self.calls = []

    def _wave(self, text):
        return np.full(240 * max(1, len(text)), 0.25, np.float32)

    @contextlib.contextmanager
    def seeded(self, seed):
        self.calls.append(("seeded", seed))
        yield seed

    def generate_voice_clone(self, text, **kw):
        self.calls.append(("clone", text, kw))
        return [self._wave(text)], 24000

    def generate_voice_clone_streaming(self, text, chunk_size=12, **kw):
        self.calls.append(("clone_stream", text, kw))
        w = self._wave(text)
        for i in range(0, len(w), 1000):
            yield w[i:i + 1000], 24000, {"chunk_index": i // 1000}

    def generate_long_voice_clone(self, text, lanes=16, long_form=None, **kw):
        self.calls.append(("long_clone", text, dict(kw, lanes=lanes, long_form=long_form)))
        return [self._wave(text)], 24000

    def generate_long_voice_clone_streaming(self, text, chunk_size=12, lanes=16, long_form=None, **kw):
        self.calls.append(("long_clone_stream", text, dict(kw, lanes=lanes, long_form=long_form)))
        segs = long_form.split(text)
        for k, s in enumerate(segs):
            yield self._wave(s.text), 24000, {"segment_index": k, "n_segments": len(segs), "chunk_index": k, "is_final": k == len(segs) - 1}

    def generate_long_custom_voice(self, text, speaker, lanes=16, long_form=None, **kw):
        self.calls.append(("long_custom", text, dict(kw, speaker=speaker, lanes=lanes, long_form=long_form)))
        return [self._wave(text)], 24000


def test_cli_long_flags(tmp_path):
    from fq3hip import audio_io, cli
    p = cli.build_parser()
    m = _ScriptedModel()
    out = str(tmp_path / "o.wav")
    a = p.parse_args(["clone", "--text", "One. Two.", "--output", out, "--ref-audio", "r.wav", "--ref-text", "t", "--long",
                      "--max-chars", "5", "--lanes", "4"])
    assert a.long and a.max_chars == 5 and a.lanes == 4
    cli.cmd_once(a, model=m)
    name, text, kw = m.calls[-1]
    assert name == "long_clone" and text == "One. Two." and kw["lanes"] == 4 and kw["long_form"].max_chars == 5 and kw["ref_audio"] == "r.wav"
    assert audio_io.read_wav(out)[1] == 24000
    cli.cmd_once(p.parse_args(["clone", "--text", "One. Two.", "--output", out, "--ref-audio", "r.wav", "--ref-text", "t", "--long", "--streaming"]),
                 model=m)
    assert m.calls[-1][0] == "long_clone_stream" and m.calls[-1][2]["lanes"] == 16 and m.calls[-1][2]["long_form"].max_chars == 240
    cli.cmd_once(p.parse_args(["custom", "--text", "One. Two.", "--output", out, "--speaker", "vivian", "--long"]), model=m)
    assert m.calls[-1][0] == "long_custom" and m.calls[-1][2]["speaker"] == "vivian"
    # without --long: today's path
    d = p.parse_args(["clone", "--text", "One. Two.", "--output", out, "--ref-audio", "r.wav", "--ref-text", "t"])
    assert d.long is False
    cli.cmd_once(d, model=m)
    assert m.calls[-1][0] == "clone"
    with pytest.raises(SystemExit):
        p.parse_args(["design", "--text", "x", "--output", out, "--instruct", "calm", "--long"])


# ---- server -----------------------------------------------------------------------------------------------------------------------
def test_server_long_form_field():
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app
    m = _ScriptedModel()
    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "t", "language": "English"}}
    client = TestClient(create_app(m, voices, default_voice="alloy", scheduler="lock", lanes=4, long_form=LongFormSpec(max_chars=20)))
    text = "First sentence here. Second sentence here. Third."
    r = client.post("/v1/audio/speech", json={"input": text, "voice": "alloy", "response_format": "pcm", "long_form": True})
    assert r.status_code == 200 and r.headers["X-Segments"] == "3"
    name, got_text, kw = m.calls[-1]
    assert name == "long_clone_stream" and got_text == text and kw["lanes"] == 4 and kw["long_form"].max_chars == 20
    assert len(r.content) == 2 * 240 * sum(len(s.text) for s in split_text(text, 20))
    # above the splitter's budget the path is taken without the field ...
    r = client.post("/v1/audio/speech", json={"input": text, "voice": "alloy", "response_format": "wav"})
    assert r.status_code == 200 and r.headers["X-Segments"] == "3" and r.content[:4] == b"RIFF" and m.calls[-1][0] == "long_clone_stream"
    # ... unless the request says no; below it, and without the field, every request behaves as it did
    r = client.post("/v1/audio/speech", json={"input": text, "voice": "alloy", "response_format": "pcm", "long_form": False})
    assert r.status_code == 200 and "X-Segments" not in r.headers and m.calls[-1][0] == "clone_stream"
    r = client.post("/v1/audio/speech", json={"input": "Short.", "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and "X-Segments" not in r.headers and m.calls[-1][0] == "clone_stream" and len(r.content) == 2 * 240 * 6
    # a short text with the field: one segment through the same path
    r = client.post("/v1/audio/speech", json={"input": "Short.", "voice": "alloy", "response_format": "pcm", "long_form": True, "seed": 5})
    assert r.status_code == 200 and r.headers["X-Segments"] == "1" and r.headers["X-Seed"] == "5" and m.calls[-1][0] == "long_clone_stream"


def test_server_long_form_under_the_batch_scheduler_is_a_400():
    from fastapi.testclient import TestClient
    from fq3hip.server import BatchWorker, create_app
    import queue

    class Worker:
        prefix_cache = None

        def __init__(self):
            self.seen = []

        def submit(self, cfg, text):
            self.seen.append(text)
            box = queue.Queue()
            box.put(np.full(100, 0.5, np.float32))
            box.put(BatchWorker.DONE)
            return box

    w = Worker()
    voices = {"alloy": {"voice_clone_prompt": {"x": 1}, "ref_text": "t", "language": "English"}}
    client = TestClient(create_app(_ScriptedModel(), voices, default_voice="alloy", scheduler="batch", worker=w,
                                   long_form=LongFormSpec(max_chars=20)))
    r = client.post("/v1/audio/speech", json={"input": "One. Two.", "voice": "alloy", "long_form": True})
    assert r.status_code == 400 and "lock scheduler" in r.text and w.seen == []
    # without the field the batch scheduler answers as it did, however long the text
    text = "First sentence here. Second sentence here. Third."
    r = client.post("/v1/audio/speech", json={"input": text, "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and "X-Segments" not in r.headers and w.seen == [text] and len(r.content) == 200


def test_server_long_form_needs_a_model_that_has_it():
    from fastapi.testclient import TestClient
    from fq3hip.server import create_app

    class Old:
        sample_rate = 24000

        def generate_voice_clone_streaming(self, text, chunk_size=12, **kw):
            yield np.full(240, 0.25, np.float32), 24000, {}

    voices = {"alloy": {"ref_audio": "a.wav", "ref_text": "t", "language": "English"}}
    client = TestClient(create_app(Old(), voices, default_voice="alloy", scheduler="lock", long_form=LongFormSpec(max_chars=5)))
    assert client.post("/v1/audio/speech", json={"input": "One. Two. Three.", "voice": "alloy", "long_form": True}).status_code == 400
    r = client.post("/v1/audio/speech", json={"input": "One. Two. Three.", "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and "X-Segments" not in r.headers and len(r.content) == 480
