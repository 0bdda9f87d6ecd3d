"""GPU: incremental text in the lock-step batch -- ``fq3_batch_text_append`` (one projection for the ids of all lanes), the
scheduler's emitted-frame accounting (``fq3hip/batching.py``) and ``stream_*_batch``.  The contract is identity with the same
requests submitted as whole text in the step-by-step layout, so every comparison is ``torch.equal`` / ``==``.

Feeders are driven by scripts keyed to the scheduler's iteration counter, relative to the iteration in which the request's lane was
armed (the scheduler hands the feeder its wake-up event then), never to the wall clock."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fq3hip.config import qwen3_tts_0p6b, tiny_test_config
from fq3hip.weights import synth_prompt, synth_weights

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


def _engines(cfg, W, dtype, n, max_seq=128, max_frames=64, pool=None):
    from fq3hip.engine import Fq3Engine
    kw = dict(device="cuda", dtype=dtype, max_seq_len=max_seq, max_frames=max_frames)
    if pool is not None:
        kw["pool"] = pool
    first = Fq3Engine(cfg, W, **kw)
    engs = [first] + [Fq3Engine(cfg, W, share=first, **kw) for _ in range(n - 1)]
    for e in engs:
        e.bind_prompt_weights(*[W[k] for k in TEXT_KEYS])
    return engs


def _ids(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, cfg.text_vocab_size, (n,), generator=g, dtype=torch.long)


def _arm_greedy(eng, cfg, dtype, seed, max_new=8):
    """prefill + first token + decode_begin with an empty trailing table (greedy, EOS suppressed)."""
    tie, _tam, _tth, tpe, _ = synth_prompt(cfg, 12, 4, 0, dtype=dtype, seed=seed)
    x = (tie * 30).to(dtype)[0].cuda().contiguous()
    eng.set_predictor_sampling(do_sample=False, top_k=0, top_p=1.0, temperature=1.0)
    eng.set_generation_state(0, 0)
    logits, hidden = eng.prefill(x, n_pad=0)
    V = cfg.talker.vocab_size
    kw = dict(temperature=1.0, top_k=0, top_p=1.0, do_sample=False)
    tok = eng.sample(logits, sup_lo=max(0, V - 1024), sup_hi=V, keep_id=cfg.codec_eos_token_id, suppress_eos=True, noise=None, **kw)
    eng.decode_begin(first_token=int(tok), prefill_len=x.shape[0], gen_step=0, past_hidden=hidden, trailing_text=None,
                     tts_pad_embed=tpe.view(-1).cuda().contiguous(), repetition_penalty=1.0, min_new_tokens=max_new, max_new_tokens=max_new,
                     talker_noise=None, pred_noise=None, noise_frames=0, **kw)


def _read(eng):
    """Every row appended so far (an empty table has nothing to copy)."""
    n, _closed = eng.decode_text_rows()
    return eng.decode_text_read() if n else torch.empty(0, eng.cfg.talker.hidden_size, dtype=eng.dtype, device="cuda")


# ---- 1. batched append = projection ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lanes", [16, 64])
@pytest.mark.parametrize("shape,dtype", [("tiny", torch.float32), ("tiny", torch.bfloat16), ("0.6b", torch.float32), ("0.6b", torch.bfloat16)])
def test_batched_append_equals_projection(shape, dtype, n_lanes):
    """Ragged items over several calls: per call a lane gets 0 ids with final, 1, 7 or 100 ids, or is not named at all.  One call
    projects between a few hundred and ~1400 rows in ONE GEMM pair, so this is also the check that a row of text_projection does not
    depend on how many rows share its GEMM (the tile choice of gemm_launch follows M): every lane's table equals fq3_text_project of
    that lane's ids alone."""
    from fq3hip.engine import Fq3Batch
    cfg = _cfg(shape)
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    lanes = _engines(cfg, W, dtype, n_lanes, max_seq=64, max_frames=16)
    batch = Fq3Batch(lanes)
    cap = 160
    for l, e in enumerate(lanes):
        _arm_greedy(e, cfg, dtype, 300 + l)
        e.decode_text_open(cap)
    have = {l: [] for l in range(n_lanes)}
    closed = {l: False for l in range(n_lanes)}
    counts = (1, 7, 100, 0)
    for call in range(4):
        before = {l: _read(lanes[l]) for l in range(n_lanes)}
        items = []
        for l in range(n_lanes):
            if closed[l] or (l + call) % 3 == 0:                # not named in this call
                continue
            n = counts[(l + call) % 4]
            fin = n == 0 or (call == 3 and l % 2 == 0)
            ids = _ids(cfg, n, 1000 * call + l).tolist()
            items.append((l, ids, fin))
        assert len(items) > n_lanes // 3
        batch.text_append(items)
        named = {l for l, _i, _f in items}
        for l, ids, fin in items:
            have[l] += ids
            closed[l] = closed[l] or fin
        torch.cuda.synchronize()
        for l in range(n_lanes):
            assert lanes[l].decode_text_rows() == (len(have[l]), closed[l]), (call, l)
            got = _read(lanes[l])
            if l not in named:
                assert torch.equal(got, before[l]), f"call {call}: lane {l} was not named and changed"
            elif have[l]:
                want = lanes[0].text_project(torch.tensor(have[l], dtype=torch.long, device="cuda"))
                assert torch.equal(got, want), f"{shape} {dtype} call {call}: lane {l}'s rows differ from fq3_text_project of its ids"
    # a batched append continues a table the single-lane append began, and the other way round
    l = next(l for l in range(n_lanes) if not closed[l])
    more = _ids(cfg, 5, 77).tolist()
    lanes[l].decode_text_append(more[:2])
    batch.text_append([(l, more[2:], True)])
    have[l] += more
    want = lanes[0].text_project(torch.tensor(have[l], dtype=torch.long, device="cuda"))
    got = lanes[l].decode_text_read()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and lanes[l].decode_text_rows() == (len(have[l]), True)
    batch.close()


# ---- 2. errors are all-or-nothing --------------------------------------------------------------------------------------------------
def test_errors_change_nothing():
    from fq3hip._lib import Fq3Error
    from fq3hip.engine import Fq3Batch
    cfg, dtype = _cfg("tiny"), torch.float32
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    lanes = _engines(cfg, W, dtype, 4, max_seq=64, max_frames=16)
    batch = Fq3Batch(lanes)
    for l, e in enumerate(lanes):
        _arm_greedy(e, cfg, dtype, 300 + l)
    for l in (0, 1, 2):
        lanes[l].decode_text_open(8)
    ids = _ids(cfg, 12, 9).tolist()
    batch.text_append([(0, ids[:3], False), (1, ids[3:5], False), (2, ids[5:6], True)])       # lane 2 closed, lane 3 never opened

    def snapshot():
        torch.cuda.synchronize()
        return [(lanes[l].decode_text_rows(), lanes[l].decode_text_read().cpu()) for l in (0, 1, 2)]

    def same(a, b):
        return all(x[0] == y[0] and torch.equal(x[1], y[1]) for x, y in zip(a, b))

    base = snapshot()
    assert [b[0] for b in base] == [(3, False), (2, False), (1, True)]
    bad = {
        "capacity": ([(0, ids[:2], False), (1, ids[:7], False)], -1),
        "closed table": ([(0, ids[:2], False), (2, ids[:1], False)], -3),
        "never opened": ([(0, ids[:2], False), (3, ids[:1], False)], -3),
        "duplicate lane": ([(0, ids[:2], False), (1, ids[:1], False), (0, ids[:1], True)], -1),
        "bad index": ([(0, ids[:2], False), (4, ids[:1], False)], -1),
        "negative index": ([(-1, ids[:2], False)], -1),
        "nothing to do": ([(0, ids[:2], False), (1, [], False)], -1),
    }
    for what, (items, code) in bad.items():
        with pytest.raises(Fq3Error) as e:
            batch.text_append(items)
        assert e.value.code == code, what
        assert same(snapshot(), base), f"{what}: a refused call changed a lane"
    batch.text_append([(1, ids[6:12], True), (0, [], True)])                                      # to the last row of lane 1's capacity
    torch.cuda.synchronize()
    assert lanes[1].decode_text_rows() == (8, True) and lanes[0].decode_text_rows() == (3, True)
    assert torch.equal(lanes[1].decode_text_read(), lanes[0].text_project(torch.tensor(ids[3:5] + ids[6:12], device="cuda")))
    batch.close()


# ---- scheduler ---------------------------------------------------------------------------------------------------------------------
class _Script:
    """``source`` for ``BatchDecoder.run``: yields no request; feeds every feeder by its plan ``[(iterations after its lane was
    armed, ids to have fed by then or None = all + close)]``."""

    def __init__(self, dec, plans):
        self.dec, self.plans, self.armed_at, self.fed = dec, plans, {}, {}

    def __call__(self):
        it = self.dec.text_stats["iterations"]
        for rid, (feeder, ids, plan) in self.plans.items():
            if feeder.waker is None or feeder.closed:
                continue
            t0 = self.armed_at.setdefault(rid, it)
            for delta, upto in plan:
                if it - t0 >= delta:
                    n = len(ids) if upto is None else min(upto, len(ids))
                    if n > self.fed.get(rid, 0):
                        feeder.feed_ids(ids[self.fed.get(rid, 0):n])
                        self.fed[rid] = n
                    if upto is None:
                        feeder.close()
        return None


def _scheduler(cfg, W, dtype, n_lanes, sample=False, max_frames=160, max_seq=256):
    from fq3hip.batching import BatchDecoder
    from fq3hip.engine import Fq3KvPool
    pool = Fq3KvPool(cfg, 2 * n_lanes * Fq3KvPool.blocks_for(max_seq), dtype=dtype)
    engs = _engines(cfg, W, dtype, 2 * n_lanes, max_seq=max_seq, max_frames=max_frames, pool=pool)
    policy = dict(do_sample=True, top_k=20, top_p=1.0, temperature=0.9) if sample else dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0)
    dec = BatchDecoder(engs[:n_lanes], predictor_policy=policy, staging=engs[n_lanes:])
    dec.text_wait_s = 0.002
    return dec, engs


def _requests(cfg, dtype, engs, specs, as_text, sample=False):
    """specs: [(rid, prompt rows, text ids (without tts_eos), max_new, text-fed?)] -> (requests, plans for _Script)."""
    from fq3hip.batching import BatchRequest
    from fq3hip.text_stream import TextFeeder
    talker = SimpleNamespace(rope_deltas=None)
    tcfg = SimpleNamespace(codec_eos_token_id=cfg.codec_eos_token_id, vocab_size=cfg.talker.vocab_size)
    eos = int(cfg.tts_eos_token_id)
    reqs, plans = [], {}
    for rid, plen, ids, max_new, fed, plan in specs:
        tie, tam, _tth, tpe, _ = synth_prompt(cfg, plen, 4, 0, dtype=dtype, seed=500 + rid)
        tie = (tie * 30).to(dtype).cuda()
        kw = (dict(temperature=0.9, top_k=20, top_p=1.0, do_sample=True, repetition_penalty=1.05) if sample
              else dict(temperature=1.0, top_k=0, top_p=1.0, do_sample=False, repetition_penalty=1.0))
        kw.update(max_new_tokens=max_new, min_new_tokens=max_new)                      # EOS suppressed: every run has its planned length
        if fed and as_text:
            f = TextFeeder()
            H = tie.shape[-1]
            reqs.append(BatchRequest(rid, talker, tie, tam.cuda(), tie.new_zeros(1, 0, H), tpe.cuda(), tcfg, kw, text_feeder=f, tts_eos_id=eos))
            plans[rid] = (f, list(ids), plan)
        else:
            table = engs[0].text_project(torch.tensor(list(ids) + [eos], dtype=torch.long, device="cuda"))
            reqs.append(BatchRequest(rid, talker, tie, tam.cuda(), table[None], tpe.cuda(), tcfg, kw))
    return reqs, plans


def _run(dec, reqs, plans, chunk=12):
    out = {}
    for rid, codes, info in dec.run(reqs, source=_Script(dec, plans) if plans else None, chunk_frames=chunk):
        assert "error" not in info, info
        ev = info.get("codes_ready_event")
        if ev is not None:
            ev.synchronize()
        out.setdefault(rid, []).append((None if codes is None else codes.cpu(), bool(info.get("is_final")), int(info.get("total_steps_so_far", -1))))
    return out


def _same_events(a, b):
    assert sorted(a) == sorted(b)
    for rid in a:
        assert [(e[1], e[2], None if e[0] is None else tuple(e[0].shape)) for e in a[rid]] == \
               [(e[1], e[2], None if e[0] is None else tuple(e[0].shape)) for e in b[rid]], f"request {rid}: chunk boundaries differ"
        for x, y in zip(a[rid], b[rid]):
            assert (x[0] is None and y[0] is None) or torch.equal(x[0], y[0]), f"request {rid}: codes differ"


# plans: holds BEFORE (rows stop at 50), ON (64) and AFTER (70) the first ring boundary, then at 120 / 128 / 133 around the second
_LATE = [(0, 50), (12, 64), (22, 70), (30, 120), (42, 128), (52, 133), (60, None)]
_EARLY = [(0, None)]                                   # everything at once: never late
_SLOW = [(3 * k, 9 * k + 4) for k in range(16)] + [(50, None)]


@pytest.mark.parametrize("n_lanes", [16, 64])
def test_scheduler_identity_greedy(n_lanes):
    """More requests than lanes (lane reuse, staged admission), text-fed and whole-text requests mixed, long lanes past emitted frames
    64 and 128, feeders that are late before, on and after a ring boundary: every utterance's codes and chunk boundaries equal those
    of the same requests submitted as whole text through the same scheduler."""
    dtype = torch.bfloat16
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    dec, engs = _scheduler(cfg, W, dtype, n_lanes)
    n_req = n_lanes + n_lanes // 2
    specs = []
    for r in range(n_req):
        long = r % 4 != 3
        max_new = 150 + (r % 5) if long else 30 + r % 7
        n_text = [170, 90, 140, 25][r % 4] + r % 3              # longer and shorter than the run
        plan = [_LATE, _EARLY, _SLOW][r % 3]
        specs.append((r, 14 + (5 * r) % 23, _ids(cfg, n_text, 900 + r).tolist(), max_new, r % 5 != 4, plan))
    ref_reqs, _ = _requests(cfg, dtype, engs, specs, as_text=False)
    ref = _run(dec, ref_reqs, None)
    assert dec.text_stats["appends"] == 0 and dec.text_stats["polls_held"] == 0
    reqs, plans = _requests(cfg, dtype, engs, specs, as_text=True)
    got = _run(dec, reqs, plans)
    st = dec.text_stats
    assert st["appends"] > 0 and st["polls_held"] > 0 and st["polls_mixed"] > 0, st       # held and running lanes were seen together
    _same_events(got, ref)
    for r, _p, _i, max_new, _f, _pl in specs:
        assert sum(e[0].shape[0] for e in got[r] if e[0] is not None) == max_new


def test_sampled_request_across_ring_wraps():
    """ONE sampled text-fed request (the other lanes idle), late before, on and after emitted frames 64 and 128: its codes equal the
    whole-text run with the same seed.  The noise rings are refilled from the global generator, so this holds only if the refills
    follow EMITTED frames (a refill that follows launched frames redraws a ring the held lane has not finished reading).  With several
    sampled requests the draws from the one generator interleave by timing, so only the single-request form is an identity."""
    dtype = torch.bfloat16
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    dec, engs = _scheduler(cfg, W, dtype, 16, sample=True)
    specs = [(0, 20, _ids(cfg, 140, 31).tolist(), 150, True, _LATE)]
    torch.manual_seed(1234)
    ref_reqs, _ = _requests(cfg, dtype, engs, specs, as_text=False, sample=True)
    ref = _run(dec, ref_reqs, None)
    torch.manual_seed(1234)
    reqs, plans = _requests(cfg, dtype, engs, specs, as_text=True, sample=True)
    got = _run(dec, reqs, plans)
    assert dec.text_stats["polls_held"] > 0
    _same_events(got, ref)
    torch.manual_seed(99)                                  # (the seed matters: the comparison above is not vacuous)
    other = _run(dec, _requests(cfg, dtype, engs, specs, as_text=False, sample=True)[0], None)
    assert not all(torch.equal(x[0], y[0]) for x, y in zip(other[0], ref[0]))


def test_no_frames_while_every_lane_is_starved():
    """Four text-fed lanes with 16 rows each and nothing more until 60 scheduler iterations later.  frames() is called only when a lane
    can advance: ceil(16 / 8) calls before the gap and ceil((40 - 16) / 8) after it at poll_every = 8 -- not one call per iteration of
    the gap -- and decoding resumes to the codes of the whole text."""
    dtype = torch.bfloat16
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text"))
    dec, engs = _scheduler(cfg, W, dtype, 4, max_frames=64, max_seq=128)
    gap = [(0, 16), (60, None)]
    specs = [(r, 14 + 3 * r, _ids(cfg, 60, 40 + r).tolist(), 40, True, gap) for r in range(4)]
    ref = _run(dec, _requests(cfg, dtype, engs, specs, as_text=False)[0], None)
    whole_calls = dec.text_stats["frames_calls"]
    reqs, plans = _requests(cfg, dtype, engs, specs, as_text=True)
    got = _run(dec, reqs, plans)
    st = dec.text_stats
    assert st["frames_calls"] <= -(-16 // dec.poll_every) + -(-(40 - 16) // dec.poll_every), (st, whole_calls)
    assert st["idle_waits"] >= 40, st
    _same_events(got, ref)


# ---- public API ----------------------------------------------------------------------------------------------------------------------
def _pieces(text, how, seed):
    import random
    if how == "chars":
        return list(text)
    if how == "whole":
        return [text]
    rng, out, at = random.Random(seed), [], 0
    while at < len(text):
        n = rng.randint(1, 7)
        out.append(text[at:at + n])
        at += n
    return out


def test_public_api_stream_custom_voice_batch():
    """Ten utterances over four lanes (lane reuse), cut inside words, one character at a time, whole, one of them arriving slowly and one
    through a caller's TextFeeder: per utterance the PCM chunks of generate_custom_voice_batch_streaming(non_streaming_mode=False)."""
    import time
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.text_stream import TextFeeder, pump_text
    dtype = torch.bfloat16
    cfg = _cfg("tiny")
    W = synth_weights(cfg, 0, dtype, parts=("talker", "predictor", "text", "codec"))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=dtype, max_seq_len=160, max_frames=48, codec_max_frames=64)
    m.predictor_graph.do_sample, m.predictor_graph.top_k = False, 0
    texts = [f"Nummer {i}: Grüße an alle, the quick brown fox {'jumps over the lazy dog ' * (1 + i % 3)}你好 world!" for i in range(10)]
    kw = dict(max_new_tokens=30, min_new_tokens=30, chunk_size=4, do_sample=False, temperature=1.0, top_k=0, repetition_penalty=1.0, lanes=4)

    def collect(gen):
        out = {}
        for i, audio, sr, tm in gen:
            out.setdefault(i, []).append((np.asarray(audio).copy(), sr, tm["chunk_index"], tm["chunk_steps"], tm["is_final"], tm.get("first_text_ms")))
        return out
    ref = collect(m.generate_custom_voice_batch_streaming(texts, "bob", "English", non_streaming_mode=False, **kw))
    assert sorted(ref) == list(range(10)) and all(sum(c[3] for c in ref[i]) == 30 for i in ref)

    def slowly(pieces):
        for p in pieces:
            time.sleep(0.004)
            yield p
    iters = []
    for i, t in enumerate(texts):
        pieces = _pieces(t, ("inside", "chars", "whole")[i % 3], i)
        assert "".join(pieces) == t
        if i == 3:
            iters.append(slowly(pieces))
        elif i == 6:
            f = TextFeeder(m._text_tokenize())
            pump_text(f, slowly(pieces))
            iters.append(f)
        else:
            iters.append(iter(pieces))
    got = collect(m.stream_custom_voice_batch(iters, "bob", "English", **{k: v for k, v in kw.items()}))
    assert sorted(got) == sorted(ref)
    for i in ref:
        assert [c[1:5] for c in got[i]] == [c[1:5] for c in ref[i]], f"utterance {i}: chunk boundaries differ"
        assert got[i][0][5] is not None and got[i][0][5] > 0 and all(c[5] is None for c in got[i][1:])
        for k, (g, r) in enumerate(zip(got[i], ref[i])):
            assert g[0].shape == r[0].shape and np.array_equal(g[0], r[0]), f"utterance {i}: PCM of chunk {k} differs"
    H = cfg.talker.hidden_size
    icl = dict(ref_spk_embedding=[torch.zeros(H)], x_vector_only_mode=[False], icl_mode=[True], ref_code=[torch.zeros(4, 16, dtype=torch.long)])
    with pytest.raises(ValueError, match="ICL"):
        next(m.stream_voice_clone_batch([iter(["hello there"])], "English", voice_clone_prompt=icl))


def test_server_sessions_decode_in_lanes():
    """The real batch worker: five sessions over three lanes, text sent in pieces from client threads (one session starts late, so it
    is parked beside the scheduler until its first word is complete), audio streamed back; finished sessions are gone."""
    import struct
    import threading
    import time
    from fastapi.testclient import TestClient
    from fq3hip.model import FasterQwen3TTS
    from fq3hip.server import create_app
    cfg = tiny_test_config()
    W = synth_weights(cfg, 0, torch.float32, parts=("talker", "predictor", "codec", "text"))
    m = FasterQwen3TTS.from_weights(cfg, W, device="cuda", dtype=torch.float32, max_seq_len=160, codec_max_frames=128, max_frames=64)
    spk = torch.randn(cfg.talker.hidden_size, generator=torch.Generator().manual_seed(12))
    vcp = dict(ref_code=[None], ref_spk_embedding=[spk], x_vector_only_mode=[True], icl_mode=[False])
    voices = {"alloy": {"voice_clone_prompt": vcp, "language": "English", "max_new_tokens": 20}}
    client = TestClient(create_app(m, voices, default_voice="alloy", scheduler="batch", lanes=3, chunk_size=4))
    base = "/v1/audio/speech/sessions"
    texts = ["One short line.", "A second and rather longer request with more words in it.", "Third.", "Number four goes last.", "Five five."]
    ids = [client.post(base, json={"voice": "alloy", "response_format": "wav" if i % 2 == 0 else "pcm"}).json()["id"] for i in range(len(texts))]
    assert len(set(ids)) == len(ids)
    results, errors = [None] * len(texts), []

    def talk(i):
        if i == 4:
            time.sleep(0.3)
        words = texts[i].split(" ")
        for k, w in enumerate(words):
            r = client.post(f"{base}/{ids[i]}/text", json={"text": w + (" " if k + 1 < len(words) else ""), "final": k + 1 == len(words)})
            if r.status_code == 404 and k > 0:
                return                                       # the utterance reached its frame limit (20) before its text ended: finished, dropped
            if r.status_code != 200:
                errors.append((i, k, r.status_code, r.text))
                return
            time.sleep(0.005)

    def listen(i):
        results[i] = client.get(f"{base}/{ids[i]}/audio")

    th = [threading.Thread(target=f, args=(i,)) for i in range(len(texts)) for f in (talk, listen)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=180)
    assert not errors, errors
    for i, r in enumerate(results):
        assert r is not None and r.status_code == 200, None if r is None else r.text
        body = r.content
        if i % 2 == 0:
            assert body[:4] == b"RIFF" and struct.unpack("<I", body[40:44])[0] == 0xFFFFFFFF
            body = body[44:]
        assert len(body) > 2000 and len(body) % 2 == 0
        assert client.get(f"{base}/{ids[i]}/audio").status_code == 404
    # whole-text requests still go through the same worker
    r = client.post("/v1/audio/speech", json={"input": "pcm please", "voice": "alloy", "response_format": "pcm"})
    assert r.status_code == 200 and len(r.content) > 2000
