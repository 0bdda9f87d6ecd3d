"""GPU: incremental text (fq3_decode_text_open / _append, the hold rule of frame_begin_body, fq3hip/text_stream.py, the stream_*
entry points).  The contract is identity: a session armed on the first text token and fed the rest in pieces of any size, at any
pace, gives the codes and the audio chunks of today's whole-text call with ``non_streaming_mode=False`` -- bit for bit, so every
comparison here is ``torch.equal`` / ``==``; the feature adds no arithmetic and no tolerance is involved.

The hold is exercised by NOT supplying rows, which is a normal state of the feature.  Tests that launch held (no-op) frames on
purpose use noise rings as long as the run: the generator's rings are refilled by the count of frames launched."""
import copy
import random
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import qwen3_tts_0p6b, tiny_test_config
from fq3hip.weights import synth_prompt, synth_weights

DTYPES = [torch.float32, torch.bfloat16]
TEXT_KEYS = ("talker.model.text_embedding.weight", "talker.text_projection.linear_fc1.weight", "talker.text_projection.linear_fc1.bias",
             "talker.text_projection.linear_fc2.weight", "talker.text_projection.linear_fc2.bias")


def _cfg(shape):
    if shape == "tiny":
        cfg = copy.deepcopy(tiny_test_config())
    else:       # the 0.6B layer shapes (text_hidden 2048 -> hidden 1024), depth and text vocabulary cut so that the weights are made in seconds
        cfg = qwen3_tts_0p6b()
        cfg.talker.num_hidden_layers, cfg.predictor.num_hidden_layers = 2, 1
        cfg.text_vocab_size = 4096
        cfg.tts_bos_token_id, cfg.tts_eos_token_id, cfg.tts_pad_token_id = 4090, 4091, 4092
    cfg.tts_model_type, cfg.tts_model_size = "custom_voice", "1b7"
    cfg.spk_id, cfg.spk_is_dialect = {"bob": 7}, {"bob": False}
    return cfg


def _engines(cfg, W, dtype, n, max_seq=128, max_frames=64):
    from fq3hip.engine import Fq3Engine
    first = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=max_seq, max_frames=max_frames)
    engs = [first] + [Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=max_seq, max_frames=max_frames, share=first)
                      for _ in range(n - 1)]
    for e in engs:
        e.bind_prompt_weights(*[W[k] for k in TEXT_KEYS])
    return engs


def _ids(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.text_vocab_size, (n,), generator=g, dtype=torch.long)


def _utt(cfg, dtype, seed, plen, n_text, max_new, sample, frames_of_noise):
    """A synthetic prompt, the token ids of its trailing text, and noise rings as long as the run."""
    tie, _tam, _tth, tpe, _ = synth_prompt(cfg, plen, 4, 0, dtype=dtype, seed=seed)
    g = torch.Generator().manual_seed(seed)
    V, Vp, G = cfg.talker.vocab_size, cfg.predictor.vocab_size, cfg.num_code_groups
    nf = frames_of_noise
    return dict(tie=(tie * 30).to(dtype), tpe=tpe, ids=_ids(cfg, n_text, seed + 7), max_new=max_new, sample=sample, nf=nf,
                first_noise=torch.empty(V).exponential_(1, generator=g).to(dtype).cuda(),
                tn=torch.empty(nf, V).exponential_(1, generator=g).to(dtype).cuda(),
                pn=torch.empty(nf, G - 1, Vp).exponential_(1, generator=g).to(dtype).cuda())


def _arm(eng, cfg, u, table):
    """prefill + first token + decode_begin with ``table`` [rows, H] as the (fixed, or first rows of the open) trailing table;
    min_new = max_new: EOS is suppressed, so every run has the length the test plans for."""
    kw = (dict(temperature=0.9, top_k=20, top_p=1.0, do_sample=True) if u["sample"] else dict(temperature=1.0, top_k=0, top_p=1.0, do_sample=False))
    eng.set_predictor_sampling(do_sample=u["sample"], top_k=20 if u["sample"] else 0, top_p=1.0, temperature=0.9 if u["sample"] else 1.0)
    x = u["tie"][0].cuda().contiguous()
    eng.set_generation_state(0, 0)
    logits, hidden = eng.prefill(x, n_pad=0)
    V = cfg.talker.vocab_size
    tok = eng.sample(logits, sup_lo=max(0, V - 1024), sup_hi=V, keep_id=cfg.codec_eos_token_id, suppress_eos=True,
                     noise=u["first_noise"] if u["sample"] else None, **kw)
    eng.decode_begin(first_token=int(tok), prefill_len=x.shape[0], gen_step=0, past_hidden=hidden, trailing_text=table,
                     tts_pad_embed=u["tpe"].view(-1).cuda().contiguous(), repetition_penalty=1.05 if u["sample"] else 1.0,
                     min_new_tokens=u["max_new"], max_new_tokens=u["max_new"], talker_noise=u["tn"] if u["sample"] else None,
                     pred_noise=u["pn"] if u["sample"] else None, noise_frames=u["nf"] if u["sample"] else 0, **kw)


# ---- 1. rows do not depend on the cut -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [("tiny", torch.float32), ("tiny", torch.bfloat16), ("0.6b", torch.float32), ("0.6b", torch.bfloat16)])
def test_rows_do_not_depend_on_the_cut(shape, dtype):
    """40 ids appended as pieces of 1, 1, 7, 16, 15 == fq3_text_project of all 40 at once == 40 single-id appends."""
    cfg = _cfg(shape)
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    eng = _engines(cfg, W, dtype, 1)[0]
    ids = _ids(cfg, 40, 5).cuda()
    whole = eng.text_project(ids)
    u = _utt(cfg, dtype, 3, 12, 40, 8, False, 8)
    for cuts in ([1, 1, 7, 16, 15], [1] * 40):
        _arm(eng, cfg, u, None)
        eng.decode_text_open(40)
        at = 0
        for i, n in enumerate(cuts):
            eng.decode_text_append(ids[at:at + n], final=i == len(cuts) - 1)
            at += n
        assert eng.decode_text_rows() == (40, True)
        got = eng.decode_text_read()
        torch.cuda.synchronize()
        assert torch.equal(got, whole), f"{shape} {dtype}: rows appended as {cuts[:5]}... differ from one projection of all 40"


def test_state_and_range_errors():
    """FQ3_ESTATE before begin / without an open table / without prompt weights, FQ3_EINVAL past the capacity (nothing is written)."""
    from fq3hip._lib import Fq3Error
    from fq3hip.engine import Fq3Engine
    cfg, dtype = _cfg("tiny"), torch.float32
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    bare = Fq3Engine(cfg, W, device="cuda", dtype=dtype, max_seq_len=128, max_frames=64)
    eng = _engines(cfg, W, dtype, 1)[0]
    u = _utt(cfg, dtype, 3, 12, 10, 8, False, 8)
    ids = u["ids"].cuda()

    def code(fn, *a, **k):
        with pytest.raises(Fq3Error) as e:
            fn(*a, **k)
        return e.value.code
    assert code(bare.decode_text_open, 8) == -3                  # no prompt weights
    assert code(eng.decode_text_open, 8) == -3                   # before begin
    assert code(eng.decode_text_append, ids[:2]) == -3           # not open
    assert code(eng.decode_text_rows) == -3
    _arm(eng, cfg, u, eng.text_project(ids[:4]))
    assert code(eng.decode_text_open, 3) == -1                   # smaller than the rows begin was given
    eng.decode_text_open(8)
    assert eng.decode_text_rows() == (4, False)
    assert code(eng.decode_text_append, ids[:5]) == -1           # past the capacity
    assert eng.decode_text_rows() == (4, False)                  # nothing was written
    assert code(eng.decode_text_append, ids[:0]) == -1           # no ids and not final
    eng.decode_text_append(ids[4:8])
    eng.decode_text_append(ids[:0], final=True)                  # n == 0 is allowed with final
    assert eng.decode_text_rows() == (8, True)
    assert code(eng.decode_text_append, ids[:1]) == -3           # closed
    assert code(eng.decode_text_open, 8) == -3                   # opened already
    torch.cuda.synchronize()


# ---- 2. codes do not depend on the cut or the timing -------------------------------------------------------------------------------
def _model(cfg, dtype, codec=False, **kw):
    from fq3hip.model import FasterQwen3TTS
    parts = ("talker", "predictor", "text") + (("codec",) if codec else ())
    W = synth_weights(cfg, 0, dtype, parts=parts)
    kw.setdefault("max_seq_len", 160)
    kw.setdefault("max_frames", 96)
    return FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=dtype, **kw)


class _StarvedFeeder:
    """Feeds ONE id each time the generator blocks on it: every frame waits for its row, with nothing queued on the device."""

    def __new__(cls, ids):
        from fq3hip.text_stream import TextFeeder

        class F(TextFeeder):
            def __init__(self, ids):
                super().__init__()
                self._todo, self.blocked = list(ids), 0

            def take(self, block=False, limit=None, timeout=None):
                if block and not self._ids and not self._closed:
                    self.blocked += 1
                    if self._todo:
                        self.feed_ids([self._todo.pop(0)])
                    else:
                        self.close()
                return super().take(block=False, limit=limit)
        return F(ids)


def _collect(gen):
    codes, meta = [], []
    for chunk, tm in gen:
        codes.append(chunk.cpu())
        meta.append((tm["chunk_index"], tm["chunk_steps"], tm["total_steps_so_far"], tm["is_final"]))
    return codes, meta


@pytest.mark.parametrize("shape,dtype,sample", [("tiny", torch.float32, False), ("tiny", torch.float32, True), ("tiny", torch.bfloat16, False),
                                                ("tiny", torch.bfloat16, True), ("0.6b", torch.bfloat16, True)])
def test_codes_do_not_depend_on_cut_or_timing(shape, dtype, sample):
    """Reference: fast_generate_streaming on the prompt and trailing table build_talker_inputs_hip(non_streaming_mode=False) gives
    for a 60-token text.  Session: the same first token, the other ids fed (a) all before the first frame, (b) one at a time with the
    generator starved between pieces, (c) in random pieces from a seeded generator on another thread.  72 frames: the 64-row noise
    ring wraps once; the text (59 rows + tts_eos) ends before the audio does, so the closing row and the pad rows are covered."""
    from fq3hip.prompt import build_talker_inputs_hip
    from fq3hip.streaming import fast_generate_streaming
    from fq3hip.text_stream import TextFeeder, fast_generate_text_streaming
    cfg = _cfg(shape)
    m = _model(cfg, dtype)
    inner = m.model.model
    m.predictor_graph.do_sample, m.predictor_graph.top_k = sample, (50 if sample else 0)
    text = "".join(chr(97 + (i * 7) % 26) if i % 6 != 5 else " " for i in range(60))
    iid = m.model._tokenize_texts([m.model._build_assistant_text(text)])[0]
    ids = [int(x) for x in iid.reshape(-1).tolist()]
    assert len(ids) == 3 + 60 + 5
    tie, tam, tth, tpe = build_talker_inputs_hip(inner, iid, None, None, 0, "English", "bob", False, None)
    assert tth.shape[1] == 60
    first = torch.tensor([ids[:4] + ids[-5:]], dtype=torch.long, device="cuda")
    tie1, tam1, tth1, tpe1 = build_talker_inputs_hip(inner, first, None, None, 0, "English", "bob", False, None)
    assert torch.equal(tie1, tie) and torch.equal(tpe1, tpe) and torch.equal(tth1[0, 0], tth[0, -1])      # the prompt needs the first token only
    talker, config = m._after_prepare(inner, tie)
    rest = ids[4:-5]
    kw = dict(max_new_tokens=72, min_new_tokens=72, chunk_size=12, repetition_penalty=1.05 if sample else 1.0,
              **(dict(temperature=0.9, top_k=50, top_p=1.0, do_sample=True) if sample else dict(temperature=1.0, top_k=0, top_p=1.0, do_sample=False)))

    def reference(use_graph):
        torch.manual_seed(1234)
        return _collect(fast_generate_streaming(talker, tie, tam, tth, tpe, config, m.predictor_graph, m.talker_graph, use_graph=use_graph, **kw))

    def session(feeder, use_graph):
        torch.manual_seed(1234)
        return _collect(fast_generate_text_streaming(talker, tie1, tam1, tpe1, config, m.predictor_graph, m.talker_graph, feeder,
                                                     tts_eos_id=cfg.tts_eos_token_id, use_graph=use_graph, **kw))

    ref_codes, ref_meta = reference(True)
    assert sum(c.shape[0] for c in ref_codes) == 72 and len(ref_codes) == 6
    d_codes, d_meta = reference(False)
    assert d_meta == ref_meta and all(torch.equal(a, b) for a, b in zip(d_codes, ref_codes)), "direct launches and the graph disagree (whole text)"
    for use_graph in (True, False):
        # (a) everything before the first frame
        fa = TextFeeder()
        fa.feed_ids(rest)
        fa.close()
        # (b) starved: one id per blocking wait
        fb = _StarvedFeeder(rest)
        # (c) random pieces from another thread
        fc = TextFeeder()
        rng = random.Random(99)

        def produce():
            at = 0
            while at < len(rest):
                n = rng.randint(1, 9)
                fc.feed_ids(rest[at:at + n])
                at += n
                time.sleep(rng.random() * 0.004)
            fc.close()
        for name, f in (("all up front", fa), ("starved", fb), ("random pieces", fc)):
            th = None
            if f is fc:
                th = threading.Thread(target=produce, daemon=True)
                th.start()
            codes, meta = session(f, use_graph)
            if th is not None:
                th.join(30)
            assert meta == ref_meta, f"{name} (graph={use_graph}): chunk boundaries / is_final / total_steps differ: {meta} vs {ref_meta}"
            for i, (a, b) in enumerate(zip(codes, ref_codes)):
                assert torch.equal(a, b), f"{name} (graph={use_graph}): codes of chunk {i} differ from the whole-text run"
        assert fb.blocked >= 59, "the starved feeder must have been waited on once per row"
    if sample:
        torch.manual_seed(4321)
        other, _ = _collect(fast_generate_streaming(talker, tie, tam, tth, tpe, config, m.predictor_graph, m.talker_graph, **kw))
        assert not all(torch.equal(a, b) for a, b in zip(other, ref_codes)), "the seed must matter, else the sampled case compares nothing"


# ---- 3. the hold is real and harmless ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_hold_is_real_and_harmless(dtype, graph):
    """A table opened with 3 rows, 8 frames queued: 3 frames are emitted and the loop reports done == 2; the rest appended with
    `final`, frames queued to the end: the codes of the whole-table run.  The five held frames ran the talker stack on stale input and
    overwrote past_hidden: this is the test that fails if frame_begin does not preserve it across the hold."""
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    eng = _engines(cfg, W, dtype, 1)[0]
    frames = 24
    u = _utt(cfg, dtype, 31, 20, 16, frames, True, frames + 8)
    ids = u["ids"].cuda()
    table = eng.text_project(ids)

    def prep():
        eng.graph_capture() if graph else eng.graph_reset()

    _arm(eng, cfg, u, table)
    prep()
    eng.decode_frames(frames + 1)
    n, st = eng.decode_poll_state()
    assert (n, st) == (frames, 1)
    ref = eng.decode_codes(0, n).cpu()

    _arm(eng, cfg, u, table[:3].contiguous())
    eng.decode_text_open(16)
    prep()
    eng.decode_frames(8)
    assert eng.decode_poll_state() == (3, 2)
    assert eng.decode_poll() == (3, True)                      # the bool view folds "held" into True
    eng.decode_frames(2)                                       # still no row: still held, nothing moves
    assert eng.decode_poll_state() == (3, 2)
    eng.decode_text_append(ids[3:9])
    eng.decode_frames(9)                                       # rows 3..8 -> frames 3..8, then held again at 9
    assert eng.decode_poll_state() == (9, 2)
    eng.decode_text_append(ids[9:], final=True)
    eng.decode_frames(frames - 9 + 1)
    n, st = eng.decode_poll_state()
    assert (n, st) == (frames, 1)
    got = eng.decode_codes(0, n).cpu()
    first_bad = int((got != ref).any(dim=1).nonzero()[0]) if not torch.equal(got, ref) else -1
    assert first_bad < 0, f"codes differ from the whole-table run from frame {first_bad} on"

    # cancel and re-begin on a held context behave as on a running one
    _arm(eng, cfg, u, None)
    eng.decode_text_open(16)
    eng.decode_frames(2)
    assert eng.decode_poll_state() == (0, 2)
    eng.decode_cancel()
    eng.decode_text_append(ids, final=True)
    eng.decode_frames(2)
    assert eng.decode_poll_state() == (0, 1)
    _arm(eng, cfg, u, None)
    eng.decode_text_open(16)
    eng.decode_frames(1)
    assert eng.decode_poll_state() == (0, 2)
    _arm(eng, cfg, u, table)                                   # begin on a held context: an ordinary fixed-table run
    eng.decode_frames(frames + 1)
    n, st = eng.decode_poll_state()
    assert (n, st) == (frames, 1) and torch.equal(eng.decode_codes(0, n).cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hold_under_teacher_forcing(dtype):
    """The same with fq3_decode_set_forced: the decisions recorded across two holds are those of the whole-table run."""
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    eng = _engines(cfg, W, dtype, 1)[0]
    frames = 20
    u = _utt(cfg, dtype, 41, 20, 14, frames, True, frames + 8)
    other = _utt(cfg, dtype, 42, 20, 14, frames, True, frames + 8)
    ids = u["ids"].cuda()
    table = eng.text_project(ids)
    # the ids to force: a free run of ANOTHER utterance (valid ids that the run under test would not choose itself)
    _arm(eng, cfg, other, table)
    eng.graph_reset()
    eng.decode_frames(frames)
    n, _ = eng.decode_poll_state()
    free = eng.decode_codes(0, n).to(torch.int32)
    forced = torch.cat([free, free[-1:]], dim=0).contiguous()

    def run(held):
        dec = torch.full((frames + 1, 16), -1, dtype=torch.int32, device="cuda")
        _arm(eng, cfg, u, table[:2].contiguous() if held else table)
        eng.decode_set_forced(forced, dec)
        if held:
            eng.decode_text_open(14)
            eng.decode_frames(5)
            assert eng.decode_poll_state() == (2, 2)
            eng.decode_text_append(ids[2:7])
            eng.decode_frames(7)
            assert eng.decode_poll_state() == (7, 2)
            eng.decode_text_append(ids[7:], final=True)
            eng.decode_frames(frames - 7)
        else:
            eng.decode_frames(frames)
        n, _ = eng.decode_poll_state()
        assert n == frames
        out = dec.cpu()
        eng.decode_set_forced(None, None)
        return out

    a, b = run(False), run(True)
    assert (a[1:frames] >= 0).all() and (a[0, 1:] >= 0).all()      # ([0][0] is the prefill's token: no sampler of the loop decides it)
    assert not torch.equal(a[:frames], forced[:frames].cpu()), "the run's own decisions must differ from the forced ids somewhere"
    assert torch.equal(a, b), "decisions under teacher forcing differ across the holds"


# ---- 4. lock-step lanes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lanes", [16, 64])
def test_lanes_hold_on_the_device(n_lanes):
    """bf16 default paths (16 lanes: one token tile; 64 lanes: weight-stationary GEMMs, lane attention).  Odd lanes hold open tables
    fed at different rates, even lanes fixed tables; all lanes advance together through fq3_batch_frames, so only the device can keep
    a lane whose row is missing in place.  Every lane's codes equal those of the same batch shape with every table whole and fixed
    (which is also the "no open lane at all" run the fixed lanes are compared with); the poll reports 2 exactly for the lanes a host
    model of the rule says are waiting, and 1 only at a lane's real end."""
    from fq3hip.engine import Fq3Batch
    dtype = torch.bfloat16
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    max_new = 18
    lanes = _engines(cfg, W, dtype, n_lanes, max_seq=96, max_frames=32)
    utts = [_utt(cfg, dtype, 200 + l, 14 + (5 * l) % 23, 6 + (3 * l) % 9, max_new, l % 4 != 2, max_new + 4) for l in range(n_lanes)]
    tables = [lanes[l].text_project(utts[l]["ids"].cuda()) for l in range(n_lanes)]
    batch = Fq3Batch(lanes)

    def states():
        batch.poll_async(0)
        return batch.poll_wait_states(0)

    for l in range(n_lanes):
        _arm(lanes[l], cfg, utts[l], tables[l])
    batch.graph_capture()
    batch.frames(max_new + 1)
    fr, st = states()
    assert fr == [max_new] * n_lanes and st == [1] * n_lanes
    ref = [lanes[l].decode_codes(0, max_new).cpu() for l in range(n_lanes)]

    open_lanes = [l for l in range(n_lanes) if l % 2 == 1]
    rows, closed = {}, {}
    for l in range(n_lanes):
        if l in open_lanes:
            k = (l // 2) % 3                                  # 0, 1 or 2 rows at begin
            _arm(lanes[l], cfg, utts[l], tables[l][:k].contiguous() if k else None)
            lanes[l].decode_text_open(len(utts[l]["ids"]))
            rows[l], closed[l] = k, False
        else:
            _arm(lanes[l], cfg, utts[l], tables[l])
    f = [0] * n_lanes
    done = [0] * n_lanes
    saw_hold = saw_mixed = False
    for rnd in range(60):
        for l in open_lanes:                                  # lane l gets 1 + l % 4 ids every (1 + l % 3)-th round
            if not closed[l] and rnd % (1 + l % 3) == 0:
                T = len(utts[l]["ids"])
                n = min(1 + l % 4, T - rows[l])
                fin = rows[l] + n == T
                lanes[l].decode_text_append(utts[l]["ids"][rows[l]:rows[l] + n].cuda(), final=fin)
                rows[l] += n
                closed[l] = fin
        batch.frames(3)
        for _ in range(3):                                    # the rule, on the host
            for l in range(n_lanes):
                if done[l] == 1:
                    continue
                if f[l] >= max_new:
                    done[l] = 1
                elif l in open_lanes and not closed[l] and f[l] >= rows[l]:
                    done[l] = 2
                else:
                    done[l] = 0
                    f[l] += 1
        fr, st = states()
        assert fr == f, f"round {rnd}: frames {fr} vs the rule's {f}"
        # (a lane that has emitted its last frame but has not been launched again reports 1 already if the token it sampled for the
        # frame after the budget happens to be EOS -- the one thing the host model cannot know; a waiting lane is never in that state)
        want = [d if not (d == 0 and f[l] == max_new) else st[l] for l, d in enumerate(done)]
        assert st == want and all(x in (0, 1, 2) for x in st), f"round {rnd}: poll states {st} vs the rule's {done}"
        saw_hold = saw_hold or 2 in st
        saw_mixed = saw_mixed or (2 in st and 0 in st)
        if all(d == 1 for d in done):
            break
    assert saw_hold and saw_mixed and all(d == 1 for d in done)
    for l in range(n_lanes):
        got = lanes[l].decode_codes(0, max_new).cpu()
        assert torch.equal(got, ref[l]), f"lane {l} ({'open' if l in open_lanes else 'fixed'} table) differs from the whole-table batch"
    batch.close()


# ---- 5. nothing moved for existing callers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_table_context_is_untouched(dtype):
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    a, b = _engines(cfg, W, dtype, 2)
    frames = 24
    u = _utt(cfg, dtype, 51, 20, 12, frames, True, frames)
    table = a.text_project(u["ids"].cuda())

    def run_a():
        _arm(a, cfg, u, table)
        a.graph_capture()
        seen = []
        for _ in range(6):
            a.decode_frames(4)
            seen.append(a.decode_poll_state())
        a.decode_frames(1)
        seen.append(a.decode_poll_state())
        return a.decode_codes(0, frames).cpu(), seen

    before, seen = run_a()
    # (after the last frame the poll may already say 1: the token sampled for the frame after the budget may be EOS)
    assert [s for _, s in seen[:5]] == [0] * 5 and seen[5][1] in (0, 1) and seen[6][1] == 1 and [n for n, _ in seen] == [4, 8, 12, 16, 20, 24, 24]
    ub = _utt(cfg, dtype, 52, 16, 12, 12, True, 16)
    _arm(b, cfg, ub, None)
    b.decode_text_open(12)
    b.decode_frames(3)
    assert b.decode_poll_state() == (0, 2)
    b.decode_text_append(ub["ids"].cuda(), final=True)
    b.decode_frames(13)
    assert b.decode_poll_state() == (12, 1)
    after, seen2 = run_a()
    assert torch.equal(before, after) and seen2 == seen


# ---- 6. public API ------------------------------------------------------------------------------------------------------------------
def _cuts(text, how):
    if how == "chars":
        return list(text)
    if how == "whitespace":
        out, cur = [], ""
        for ch in text:
            if ch.isspace() and cur:
                out.append(cur)
                cur = ""
            cur += ch
        return out + [cur]
    rng, out, at = random.Random(5), [], 0                     # inside words
    while at < len(text):
        n = rng.randint(1, 7)
        out.append(text[at:at + n])
        at += n
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_public_api_stream_custom_voice(dtype):
    """stream_custom_voice(iter(pieces)) yields the PCM chunks of generate_custom_voice_streaming(text, non_streaming_mode=False),
    for pieces cut inside words, at whitespace and one character at a time (multi-byte characters included); ICL is refused."""
    cfg = _cfg("tiny")
    m = _model(cfg, dtype, codec=True, codec_max_frames=64, max_frames=48)
    text = "Grüße an alle: the quick brown fox, 你好 world!"
    kw = dict(max_new_tokens=30, min_new_tokens=30, chunk_size=4)
    for sample in (False, True):
        m.predictor_graph.do_sample, m.predictor_graph.top_k = sample, (50 if sample else 0)
        skw = dict(kw, do_sample=sample, **({} if sample else dict(temperature=1.0, top_k=0, repetition_penalty=1.0)))
        torch.manual_seed(7)
        ref = [(np.asarray(a).copy(), sr, tm["chunk_steps"], tm["is_final"])
               for a, sr, tm in m.generate_custom_voice_streaming(text, "bob", "English", non_streaming_mode=False, **skw)]
        assert sum(r[2] for r in ref) == 30
        for how in ("inside", "whitespace", "chars"):
            pieces = _cuts(text, how)
            assert "".join(pieces) == text
            torch.manual_seed(7)
            got = [(np.asarray(a).copy(), sr, tm["chunk_steps"], tm["is_final"], tm.get("first_text_ms"))
                   for a, sr, tm in m.stream_custom_voice(iter(pieces), "bob", "English", **skw)]
            assert len(got) == len(ref), (how, len(got), len(ref))
            assert got[0][4] is not None and got[0][4] > 0 and all(g[4] is None for g in got[1:])
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g[1:4] == r[1:4], (how, i)
                assert g[0].shape == r[0].shape and np.array_equal(g[0], r[0]), f"{how}: PCM of chunk {i} differs (sampled={sample})"
    H = cfg.talker.hidden_size
    icl = dict(ref_spk_embedding=[torch.zeros(H)], x_vector_only_mode=[False], icl_mode=[True], ref_code=[torch.zeros(4, 16, dtype=torch.long)])
    with pytest.raises(ValueError, match="ICL"):
        next(m.stream_voice_clone(iter(["hello there"]), "English", voice_clone_prompt=icl))
    with pytest.raises(ValueError, match="ICL"):
        next(m.stream_voice_clone(iter(["hello there"]), "English", ref_audio="voice.wav", xvec_only=False))
