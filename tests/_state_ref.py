"""A model of the kernels that decide which row, which frame, which lane and whether the decode loop goes on, the cases the GPU test
runs through tools/microbench/libstate_probe.so, and the judge both tests share.

Written from the comments above the kernels (csrc/decode_kernels.cuh "On-device decode-loop state", csrc/batch_kernels.cuh,
csrc/prompt_kernels.cuh, csrc/state_kernels.cuh), from include/fq3hip.h and from the decode loop and the prompt builder of the
reference project (generate.py: EOS / limit test, [past_hidden ; embed(token)], the 16-way sum + text or pad row, the position limit;
_build_talker_inputs_local: text + codec rows), not from the kernel bodies:

* frame_begin (single and batch), six outcomes.  done == 1: nothing.  EOS token or frame >= max_new: done = 1 only.  Open table and
  gen_step >= trailing_len: entering (done == 0) copies past_hidden to ph_hold and sets done = 2; staying (done == 2) changes nothing.
  Otherwise the frame runs: a held lane takes the first half of the predictor input from ph_hold and returns to done = 0;
  codes[frame * G] = token, seen[token] = 1, pred_in = [past_hidden ; codec_emb[token]].  Batch: lane l's pred_in is 2 H elements wide.
* embed_sum (single and batch, G = 16): done != 0: nothing.  pos >= max_seq - 1: frame + 1, done = 1, nothing else.  Otherwise
  x = rnd(rnd(sum_g tab_g[id_g]) + text), the sum sequential in fp32 in table order, text = row gen_step of the trailing table or the
  pad row from gen_step == trailing_len on; rope_now = cos | sin of row clamp(pos + rope_delta, 0, rope_len - 1).  The single form
  takes rope_delta as an argument, the batch form from each lane's state.  Emulated in float32: bit-exact.
* text_gather: row copies with ids clamped into the table.  prompt_rows: text (0 <= trow < n_text), or codec, or rnd(text + codec);
  codec by kind (1: table 0 row clamp(arg); 2: spk, if there is one; 3: rnd(sequential fp32 sum over the 16 tables of frame
  clamp(arg)), ids clamped per table, if n_ref > 0; else none); neither: zeros.
* text_open / text_publish / text_scatter / text_publish_lanes, poll_gather, decode_arm / _set_forced / _cancel, codes_to_i64,
  kv_table_write, kv_paged_copy (both directions), kv_adopt: what their comments say, by bits.
* talker_step: the greedy branch of sample_talker_kernel (argmax, lowest index first; suppression window and min_new as in
  tests/_sampler_ref.py) -- it only advances the trajectories with the product's own code.
* rmsnorm_kernel: the rmsnorm reference and judge of tests/_rows_ref.py (bound + exact fraction, constants unchanged).

Memory is described whole (Mem): every buffer is a flat tensor of its storage type with guard rows in front and behind.  The sentinel
(a NaN no kernel produces; for integers 0xA5...) in an expected buffer means "keeps its bits", in an input "must not be read": a value
computed from it is a NaN and differs from the model.  Every table row that no id names holds the sentinel.  A case is an initial Mem and
a list of steps (probe launches, and host writes that play the parts of the frame this probe does not launch); after every launch the
WHOLE Mem -- all buffers by bits, all states field by field (on the device: byte for byte) -- must equal the model's."""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import _gemm_ref as G
import _rows_ref as RR

DTS = ("bf16", "f32")
TE = {"bf16": 0, "f32": 2}
TDT = {"bf16": torch.bfloat16, "f32": torch.float32}
KINDS = ["frame_begin", "frame_begin_batch", "embed_sum", "embed_sum_batch", "rmsnorm", "copy", "text_gather", "prompt_rows",
         "kv_import", "kv_export", "kv_adopt", "talker_step",
         "text_open", "text_publish", "poll_gather", "text_scatter", "text_publish_lanes", "kv_table_write", "decode_arm",
         "decode_set_forced", "decode_cancel", "codes_to_i64"]
KIND = {k: i for i, k in enumerate(KINDS)}
N_TYPED = KIND["text_open"]
KERNEL = {"frame_begin": "frame_begin_kernel", "frame_begin_batch": "frame_begin_batch_kernel", "embed_sum": "embed_sum_kernel",
          "embed_sum_batch": "embed_sum_batch_kernel", "rmsnorm": "rmsnorm_kernel", "copy": "copy_kernel", "text_gather": "text_gather_kernel",
          "prompt_rows": "prompt_rows_kernel", "kv_import": "kv_paged_copy_kernel (to the cache)", "kv_export": "kv_paged_copy_kernel (from the cache)",
          "kv_adopt": "kv_adopt_kernel", "talker_step": "sample_talker_kernel (greedy)", "text_open": "text_open_kernel",
          "text_publish": "text_publish_kernel", "poll_gather": "poll_gather_kernel", "text_scatter": "text_scatter_kernel",
          "text_publish_lanes": "text_publish_lanes_kernel", "kv_table_write": "kv_table_write_kernel", "decode_arm": "decode_arm_kernel",
          "decode_set_forced": "decode_set_forced_kernel", "decode_cancel": "decode_cancel_kernel", "codes_to_i64": "codes_to_i64_kernel"}
MAX_LANES, MAX_VOCAB, KEYS_PER_TILE, HEAD_DIM = 128, 4096, 64, 128
GUARD = 2
SENT32, SENT64, SENT8 = -1515870811, -6510615555426900571, 0xA5            # 0xA5A5... patterns

# the fields of DecodeState in declaration order: i = int32, f = float, p = pointer
STATE_FIELDS = [("token", "i"), ("frame", "i"), ("pos", "i"), ("gen_step", "i"), ("done", "i"), ("text_open", "i"), ("min_new", "i"),
                ("max_new", "i"), ("trailing_len", "i"), ("noise_frames", "i"), ("eos_id", "i"), ("max_seq", "i"), ("sup_lo", "i"),
                ("sup_hi", "i"), ("t_temperature", "f"), ("t_top_k", "i"), ("t_top_p", "f"), ("t_do_sample", "i"), ("t_rep_penalty", "f"),
                ("p_temperature", "f"), ("p_top_k", "i"), ("p_top_p", "f"), ("p_do_sample", "i"), ("trailing_text", "p"), ("tts_pad", "p"),
                ("talker_noise", "p"), ("pred_noise", "p"), ("past_hidden_init", "p"), ("n_pad", "i"), ("rope_delta", "i")]


def state(**kw):
    """A DecodeState as a dict; pointers are None or (buffer name, element offset)."""
    st = {n: (None if k == "p" else (0 if k == "i" else 0.0)) for n, k in STATE_FIELDS}
    st.update(noise_frames=1, eos_id=-1, max_new=1 << 20, max_seq=1 << 20, t_temperature=1.0, t_top_p=1.0, t_rep_penalty=1.0,
              p_temperature=0.9, p_top_k=50, p_top_p=1.0, p_do_sample=1, n_pad=3)
    assert set(kw) <= set(st), set(kw) - set(st)
    st.update(kw)
    return st


# ---- storage helpers ---------------------------------------------------------------------------------------------------------------
def esz(dt):
    return 2 if dt == "bf16" else 4


def sent(n, dt):
    """n elements of the NaN sentinel in storage type dt"""
    if dt == "bf16":
        return torch.full((n,), G.SENTINEL["bf16"] - (1 << 16), dtype=torch.int16).view(torch.bfloat16)
    return torch.full((n,), G.SENTINEL["f32"] - (1 << 32), dtype=torch.int32).view(torch.float32)


def isent(n, dtype=torch.int32):
    v = {torch.int32: SENT32, torch.int64: SENT64, torch.uint8: SENT8}[dtype]
    return torch.full((n,), v, dtype=dtype)


def bits(t):
    """the raw bits of a buffer as integers (floats by their bit pattern: NaNs compare by payload)"""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def rnd(x32, dt):
    """one rounding of fp32 values to the storage type, back in fp32"""
    return x32.to(TDT[dt]).to(torch.float32)


def values(g, n, dt):
    """n random T-representable values over a few binades (so that the order and the place of a rounding show)"""
    return RR.wide(g, dt, n, lo=-3, hi=3).to(TDT[dt])


def guarded_rows(rows, ld, dt, fill=None):
    """[GUARD + rows + GUARD][ld] of the sentinel, flat; returns (buffer, element offset of row 0).  fill(r) gives row r or None."""
    buf = sent((rows + 2 * GUARD) * ld, dt)
    off = GUARD * ld
    if fill is not None:
        for r in range(rows):
            v = fill(r)
            if v is not None:
                buf[off + r * ld:off + (r + 1) * ld] = v
    return buf, off


def table(g, rows, H, dt, used):
    used = set(used)
    return guarded_rows(rows, H, dt, lambda r: values(g, H, dt) if r in used else None)


# ---- the description of memory, launches and cases ---------------------------------------------------------------------------------
@dataclass
class Mem:
    bufs: dict = field(default_factory=dict)          # name -> flat tensor in its storage type
    states: dict = field(default_factory=dict)        # name -> DecodeState dict
    tfs: dict = field(default_factory=dict)           # name -> {"forced": ref, "decisions": ref} (TeacherForcing)

    def clone(self):
        return Mem({k: v.clone() for k, v in self.bufs.items()}, copy.deepcopy(self.states), copy.deepcopy(self.tfs))


@dataclass
class Launch:
    """One probe call in the probe's own terms.  A reference is (buffer name, element offset); ("$name", 0) names a state, ("&name", 0)
    a TeacherForcing object."""
    kind: str
    dt: str = "f32"
    p: list = field(default_factory=list)
    tab: dict = field(default_factory=dict)           # table index -> list of references
    iv: list = field(default_factory=list)
    iv2: list = field(default_factory=list)
    n: list = field(default_factory=list)
    f: list = field(default_factory=list)
    host: Optional[dict] = None                       # decode_arm: the initial state
    note: str = ""


@dataclass
class Write:
    """The host's part between two launches: buffer[off : off + len(data)] = data."""
    buf: str
    off: int
    data: torch.Tensor


@dataclass
class Case:
    name: str
    mem: Mem
    steps: list
    pb: Optional[RR.Problem] = None                   # rmsnorm: the problem of _rows_ref, judged by its judge
    lanes: Optional[list] = None                      # trajectories: what the comparison of single-stream and batch runs needs


def sl(mem, ref, n):
    name, off = ref
    b = mem.bufs[name]
    assert 0 <= off and off + n <= b.numel(), f"the model leaves buffer {name}: [{off}, {off + n}) of {b.numel()}"
    return b[off:off + n]


def st_of(mem, ref):
    assert ref[0].startswith("$"), ref
    return mem.states[ref[0][1:]]


# ---- the models ------------------------------------------------------------------------------------------------------------------------
def m_frame_begin(mem, st, past_hidden, codec_emb, pred_in, codes, seen, ph_hold, H, G_, mutant):
    if st["done"] == 1:
        return "finished"
    over = st["frame"] > st["max_new"] if mutant == "frame_gt_max_new" else st["frame"] >= st["max_new"]
    if st["token"] == st["eos_id"] or over:
        st["done"] = 1
        return "ends"
    if st["text_open"] and st["gen_step"] >= st["trailing_len"]:
        if st["done"] == 0:
            if mutant != "no_hold_copy":
                sl(mem, ph_hold, H)[:] = sl(mem, past_hidden, H)
            st["done"] = 2
            return "enters a hold"
        return "stays held"
    src, out = past_hidden, "runs"
    if st["done"] == 2:
        if mutant != "ph_hold_ignored":
            src = ph_hold
        st["done"] = 0
        out = "leaves a hold"
    tok = st["token"]
    slot = st["frame"] * G_ + (1 if mutant == "codes_slot_plus_1" else 0)
    sl(mem, codes, slot + 1)[slot] = tok
    sl(mem, seen, tok + 1)[tok] = 1
    pi = sl(mem, pred_in, 2 * H)
    pi[:H] = sl(mem, src, H)
    pi[H:] = sl(mem, (codec_emb[0], codec_emb[1] + tok * H), H)
    return out


def m_embed_sum(mem, st, codes, cos, sin, rope_now, x, tabs, H, rope_len, rope_delta, dt, mutant):
    if st["done"] != 0:
        return
    limit = st["max_seq"] if mutant == "pos_ge_max_seq" else st["max_seq"] - 1
    if st["pos"] >= limit:
        st["frame"] += 1
        st["done"] = 1
        return
    ids = sl(mem, codes, (st["frame"] + 1) * 16)[st["frame"] * 16:].tolist()
    rp = st["pos"] + rope_delta
    lo, hi = (-1 if mutant == "rope_clamp_low" else 0), (rope_len if mutant == "rope_clamp_high" else rope_len - 1)
    rp = lo if rp < lo else (hi if rp > hi else rp)
    rn = sl(mem, rope_now, HEAD_DIM)
    rn[:64] = sl(mem, (cos[0], cos[1] + rp * 64), 64)
    rn[64:] = sl(mem, (sin[0], sin[1] + rp * 64), 64)
    row = st["frame"] if mutant == "text_row_by_frame" else st["gen_step"]
    tt = st["trailing_text"]
    text = sl(mem, (tt[0], tt[1] + row * H), H) if row < st["trailing_len"] else sl(mem, st["tts_pad"], H)
    acc = None
    for g, (t, i) in enumerate(zip(tabs, ids)):
        r = sl(mem, (t[0], t[1] + i * H), H).to(torch.float32)
        acc = r if acc is None else acc + r
    sl(mem, x, H)[:] = (rnd(acc, dt) + text.to(torch.float32)).to(TDT[dt])


def m_prompt_rows(mem, L, mutant):
    dt = L.dt
    n_text, n_rows, n_ref, V0, V1, H = L.n[:6]
    text_rows, prog, ref_codes, spk, out = L.p[:5]
    tabs = L.tab[0]
    if text_rows is None:
        n_text = 0
    if ref_codes is None:
        n_ref = 0
    pg = sl(mem, prog, n_rows * 3).tolist()
    for r in range(n_rows):
        trow, kind, arg = pg[3 * r:3 * r + 3]
        has_text = 0 <= trow <= n_text if mutant == "trow_le_n_text" else 0 <= trow < n_text
        c = None
        if kind == 1:
            i = min(max(arg, 0), V0 - 1)
            c = sl(mem, (tabs[0][0], tabs[0][1] + i * H), H).to(torch.float32)
        elif kind == 2 and spk is not None:
            c = sl(mem, spk, H).to(torch.float32)
        elif kind == 3 and (n_ref > 0 or mutant == "no_n_ref_guard"):
            fr = min(max(arg, 0), n_ref - 1) if arg >= 0 else 0
            ids = sl(mem, (ref_codes[0], ref_codes[1] + fr * 16), 16).tolist()
            for g in range(16):
                i = min(max(ids[g], 0), (V0 if g == 0 else V1) - 1)
                row = sl(mem, (tabs[g][0], tabs[g][1] + i * H), H).to(torch.float32)
                c = row if c is None else c + row
            if mutant != "kind3_not_rounded":
                c = rnd(c, dt)
        t = sl(mem, (text_rows[0], text_rows[1] + trow * H), H).to(torch.float32) if has_text else None
        o = t + c if (t is not None and c is not None) else (t if t is not None else (c if c is not None else torch.zeros(H)))
        sl(mem, (out[0], out[1] + r * H), H)[:] = o.to(TDT[dt])


def m_talker_step(mem, L):
    st = st_of(mem, L.p[0])
    if st["done"]:
        return
    assert st["t_do_sample"] == 0 and st["t_rep_penalty"] == 1.0
    V = L.n[0]
    lg = sl(mem, L.p[1], V).to(torch.float32).clone()
    extra = st["eos_id"] if st["frame"] + 1 < st["min_new"] else -1
    for i in range(V):
        if (st["sup_lo"] <= i < st["sup_hi"] and i != st["eos_id"]) or i == extra:
            lg[i] = -math.inf
    st["token"] = int(torch.argmax(lg))            # (the cases plant one strict maximum)
    st["frame"] += 1
    st["pos"] += 1
    st["gen_step"] += 1


def apply(mem: Mem, L: Launch, mutant: str = ""):
    """The effect of one launch on mem (in place).  mutant names a deliberate defect (the checker's self-test)."""
    k, p, n, dt = L.kind, L.p, L.n, L.dt
    if k == "frame_begin":
        return m_frame_begin(mem, st_of(mem, p[0]), p[1], p[2], p[3], p[4], p[5], p[6], n[0], n[1], mutant)
    if k == "frame_begin_batch":
        H, G_, B = n[0], n[1], n[4]
        stride = H if mutant == "pred_in_stride_h" else 2 * H
        return [m_frame_begin(mem, st_of(mem, L.tab[0][l]), L.tab[3][l], p[0], (p[1][0], p[1][1] + l * stride), L.tab[1][l], L.tab[2][l],
                              L.tab[4][l], H, G_, mutant) for l in range(B)]
    if k == "embed_sum":
        return m_embed_sum(mem, st_of(mem, p[0]), p[1], p[2], p[3], p[4], p[5], L.tab[0], n[0], n[1], n[2], dt, mutant)
    if k == "embed_sum_batch":
        H, B = n[0], n[6]
        for l in range(B):
            st = st_of(mem, L.tab[0][l])
            delta = st_of(mem, L.tab[0][0])["rope_delta"] if mutant == "lane_rope_delta_ignored" else st["rope_delta"]
            m_embed_sum(mem, st, L.tab[1][l], p[1], p[2], (p[3][0], p[3][1] + l * HEAD_DIM), (p[0][0], p[0][1] + l * H), L.tab[2], H, n[1],
                        delta, dt, mutant)
        return
    if k == "copy":
        sl(mem, p[0], n[0])[:] = sl(mem, p[1], n[0])
    elif k == "text_gather":
        cnt, Ht, vocab = n[:3]
        ids = sl(mem, p[0], cnt).tolist()
        for r, i in enumerate(ids):
            i = min(max(i, 0), vocab - 1)
            sl(mem, (p[2][0], p[2][1] + r * Ht), Ht)[:] = sl(mem, (p[1][0], p[1][1] + i * Ht), Ht)
    elif k == "prompt_rows":
        m_prompt_rows(mem, L, mutant)
    elif k in ("kv_import", "kv_export"):
        blk_stride, n_kv, Ln = n[:3]
        nb = (Ln + KEYS_PER_TILE - 1) // KEYS_PER_TILE
        tb = sl(mem, p[1], nb).tolist()
        for h in range(n_kv):
            for key in range(Ln):
                b, r = key // KEYS_PER_TILE, key % KEYS_PER_TILE
                if mutant == "block_and_row_swapped":
                    b, r = r % nb, b
                c = (p[0][0], p[0][1] + tb[b] * blk_stride + (h * KEYS_PER_TILE + r) * HEAD_DIM)
                d = (p[2][0], p[2][1] + (h * Ln + key) * HEAD_DIM)
                if k == "kv_import":
                    sl(mem, c, HEAD_DIM)[:] = sl(mem, d, HEAD_DIM)
                else:
                    sl(mem, d, HEAD_DIM)[:] = sl(mem, c, HEAD_DIM)
    elif k == "kv_adopt":
        n_which, nb, be = n[:3]
        dt_, stb = sl(mem, p[0], nb).tolist(), sl(mem, p[1], nb).tolist()
        if mutant == "source_by_destination_table":
            stb = dt_
        for w in range(n_which):
            d, s = L.tab[0][w], L.tab[1][w]
            for b in range(nb):
                sl(mem, (d[0], d[1] + dt_[b] * be), be)[:] = sl(mem, (s[0], s[1] + stb[b] * be), be)
    elif k == "talker_step":
        m_talker_step(mem, L)
    elif k == "text_open":
        st = st_of(mem, p[0])
        cnt = n[0] * 4 // mem.bufs[p[1][0]].element_size()          # n[0] counts 32-bit words, whatever the buffers hold
        sl(mem, p[1], cnt)[:] = sl(mem, p[2], cnt)
        st["trailing_text"], st["text_open"] = (p[1][0], p[1][1]), 1
    elif k == "text_publish":
        st = st_of(mem, p[0])
        st["trailing_len"] = n[0]
        if n[1]:
            st["text_open"] = 0
    elif k == "poll_gather":
        out = sl(mem, p[0], 2 * n[0])
        for l in range(n[0]):
            st = st_of(mem, L.tab[0][l])
            out[2 * l] = st["frame"]
            held = 1 if mutant == "poll_held_as_finished" else 2
            out[2 * l + 1] = held if st["done"] == 2 else (1 if (st["done"] or st["token"] == st["eos_id"]) else 0)
    elif k == "text_scatter":
        items, row_vec, N = n[:3]
        first = L.iv
        w = row_vec * 4                                  # the packed buffer and the tables are described in 32-bit words
        for r in range(N):
            if mutant == "scatter_first_item":
                i = min(j for j in range(items) if first[j] <= r)
            else:
                i = max(j for j in range(items) if first[j] <= r)
            d = L.tab[0][i]
            sl(mem, (d[0], d[1] + (r - first[i]) * w), w)[:] = sl(mem, (p[0][0], p[0][1] + r * w), w)
    elif k == "text_publish_lanes":
        for i in range(n[0]):
            st = st_of(mem, L.tab[0][i])
            st["trailing_len"] = L.iv[i]
            if L.iv2[i]:
                st["text_open"] = 0
    elif k == "kv_table_write":
        sl(mem, (p[0][0], p[0][1] + n[0]), n[1])[:] = torch.tensor(L.iv[:n[1]], dtype=torch.int32)
    elif k == "decode_arm":
        sl(mem, p[1], n[0])[:] = 0
        sl(mem, p[2], n[1])[:] = sl(mem, p[3], n[1])
        mem.states[p[0][0][1:]] = copy.deepcopy(L.host)
    elif k == "decode_set_forced":
        mem.tfs[p[0][0][1:]] = {"forced": p[1], "decisions": p[2]}
    elif k == "decode_cancel":
        st_of(mem, p[0])["done"] = 1
    elif k == "codes_to_i64":
        sl(mem, p[1], n[0])[:] = sl(mem, p[0], n[0]).to(torch.int64)
    else:
        raise KeyError(k)


def run_model(case: Case, mutant: str = ""):
    """The Mem after every launch of the case (host writes applied in between)."""
    mem = case.mem.clone()
    out = []
    for s in case.steps:
        if isinstance(s, Write):
            mem.bufs[s.buf][s.off:s.off + s.data.numel()] = s.data
        else:
            apply(mem, s, mutant)
            out.append(mem.clone())
    return out


def judge(want: Mem, got: Mem, what: str = "") -> list:
    """Every buffer by bits, every state field by field, every forcing object.  Returns the differences (empty: equal)."""
    bad = []
    for name, w in want.bufs.items():
        g = got.bufs[name]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(f"{what}: buffer {name} has another type or size")
            continue
        ne = bits(g) != bits(w)
        if bool(ne.any()):
            i = int(torch.nonzero(ne)[0])
            bad.append(f"{what}: buffer {name}: {int(ne.sum())} of {w.numel()} elements differ, first at {i}: got {g[i].item()!r}, "
                       f"the model has {w[i].item()!r}")
    for name, w in want.states.items():
        g = got.states[name]
        for f_, _k in STATE_FIELDS:
            if g[f_] != w[f_]:
                bad.append(f"{what}: state {name}.{f_} = {g[f_]!r}, the model has {w[f_]!r}")
    if want.tfs != got.tfs:
        bad.append(f"{what}: a TeacherForcing object differs")
    return bad


# ---- cases: the frame prologue ---------------------------------------------------------------------------------------------------------
V0, V1 = 96, 40                  # talker and predictor vocabularies (they differ, as in the product)
OUTCOMES = ("finished", "ends by EOS", "ends by max_new", "enters a hold", "stays held", "leaves a hold", "runs")


def gen(*seed):
    return RR.gen("state", *seed)


def outcome_state(kind, tok, frame, max_new):
    """A state that frame_begin takes to outcome `kind`."""
    st = state(token=tok, frame=frame, pos=40 + frame, gen_step=3, max_new=max_new, eos_id=V0 - 7, trailing_len=6, min_new=2)
    if kind == "finished":
        st.update(done=1)
    elif kind == "ends by EOS":
        st.update(token=st["eos_id"])
    elif kind == "ends by max_new":
        st.update(frame=max_new)
    elif kind == "enters a hold":
        st.update(text_open=1, trailing_len=3)
    elif kind == "stays held":
        st.update(text_open=1, trailing_len=2, done=2)
    elif kind == "leaves a hold":
        st.update(text_open=1, trailing_len=4, done=2)
    else:
        assert kind == "runs"
    return st


def lane_buffers(mem, g, tag, dt, H, G_, frames, slot, n_slots):
    """One lane's codes, seen, past_hidden and ph_hold inside shared buffers, at slot `slot` of n_slots (the slots are handed out in
    shuffled order, so lane index and address order disagree); between the slots lie guard regions."""
    need = {"codes": ((frames + 2 * GUARD) * G_, torch.int32), "seen": (V0 + 2 * 16, torch.uint8), "ph": (H + 2 * 8, None), "hold": (H + 2 * 8, None)}
    refs = {}
    for name, (cnt, ity) in need.items():
        key = f"{tag}{name}"
        if key not in mem.bufs:
            mem.bufs[key] = isent(cnt * n_slots, ity) if ity is not None else sent(cnt * n_slots, dt)
        lead = {"codes": GUARD * G_, "seen": 16, "ph": 8, "hold": 8}[name]
        refs[name] = (key, slot * cnt + lead)
    sl(mem, refs["ph"], H)[:] = values(g, H, dt)
    sl(mem, refs["hold"], H)[:] = values(g, H, dt)          # differs from past_hidden in every element (random, the same binades)
    sl(mem, refs["seen"], V0)[:] = 0
    return refs


def frame_begin_case(dt, H, G_, lanes, batch, seed):
    """lanes: [(outcome, tok, frame, max_new)].  Single: one launch per lane; batch: one launch over all lanes."""
    g = gen("fb", dt, H, G_, len(lanes), seed)
    mem = Mem()
    frames = max(l[3] for l in lanes)
    mem.bufs["emb"], emb_off = table(g, V0, H, dt, {l[1] for l in lanes})
    B = len(lanes)
    mem.bufs["pred_in"] = sent((B + 2 * GUARD) * 2 * H, dt)
    perm = torch.randperm(B, generator=g).tolist()
    steps, tabs = [], {i: [] for i in range(5)}
    for l, (kind, tok, frame, max_new) in enumerate(lanes):
        mem.states[f"l{l}"] = outcome_state(kind, tok, frame, max_new)
        r = lane_buffers(mem, g, "", dt, H, G_, frames, perm[l], B)
        for i, ref in enumerate([(f"$l{l}", 0), r["codes"], r["seen"], r["ph"], r["hold"]]):
            tabs[i].append(ref)
        if not batch:
            steps.append(Launch("frame_begin", dt, p=[(f"$l{l}", 0), r["ph"], ("emb", emb_off), ("pred_in", (GUARD + l) * 2 * H), r["codes"], r["seen"],
                                                      r["hold"]], n=[H, G_, V0, frames], note=f"{kind} tok {tok} frame {frame}"))
    if batch:
        steps = [Launch("frame_begin_batch", dt, p=[("emb", emb_off), ("pred_in", GUARD * 2 * H)], tab=tabs, n=[H, G_, V0, frames, B],
                        note=f"B {B}")]
    return Case(f"frame_begin{'_batch' if batch else ''} {dt} H {H} G {G_} B {B} #{seed}", mem, steps)


def outcome_lanes(B, max_new=5):
    """B lanes cycling through the outcomes, frame 0 and max_new - 1, tok 0 and V - 1 among them"""
    out = []
    for l in range(B):
        kind = OUTCOMES[(l + 6) % 7] if B > 1 else "runs"
        tok = (0, V0 - 1, 5, 17)[l % 4]
        frame = (0, max_new - 1, 2)[(l // 2) % 3]
        out.append((kind, tok, frame, max_new))
    return out


def frame_begin_cases(dt):
    cs = []
    for H in (1, 8, 257, 264, 1024, 2048, 2056):
        cs.append(frame_begin_case(dt, H, 16, [("runs", 0, 0, 4), ("leaves a hold", V0 - 1, 3, 4)], False, 0))
    for G_ in (16, 3):
        cs.append(frame_begin_case(dt, 264, G_, outcome_lanes(14), False, 1))
    for B in (1, 3, 128):
        cs.append(frame_begin_case(dt, 264, 16, outcome_lanes(B), True, 2))
    cs.append(frame_begin_case(dt, 8, 3, outcome_lanes(9), True, 3))
    return cs


# ---- cases: the embedding sum ------------------------------------------------------------------------------------------------------------
ROPE_LEN = 11


def embed_sum_case(dt, H, lanes, batch, seed):
    """lanes: [dict(pos_delta = pos + rope_delta wanted, stop, gen_rel = gen_step - trailing_len, trailing_len, done, rope_delta)]"""
    g = gen("es", dt, H, len(lanes), seed)
    mem = Mem()
    B = len(lanes)
    frames = 3
    ids = [[int(torch.randint(0, V0 if j == 0 else V1, (1,), generator=g)) for j in range(16)] for _ in range(B)]
    for l in range(B):                                     # row 0 and the last row of every table are named
        for j in range(16):
            if (l + j) % 5 == 0:
                ids[l][j] = 0
            if (l + j) % 5 == 1:
                ids[l][j] = (V0 if j == 0 else V1) - 1
    tabs = []
    for j in range(16):
        mem.bufs[f"tab{j}"], off = table(g, V0 if j == 0 else V1, H, dt, {ids[l][j] for l in range(B)})
        tabs.append((f"tab{j}", off))
    used_rope = set()
    sts = []
    T_ROWS = 4
    for l, c in enumerate(lanes):
        rd = c.get("rope_delta", -5 - l % 3)
        max_seq = 50 + l
        pos = max_seq - 1 if c.get("stop") else (max_seq - 2 if c.get("last") else c["pos_delta"] - rd)
        if c.get("stop") or c.get("last"):
            rd = c["pos_delta"] - pos
        tl = c.get("trailing_len", 3)
        st = state(token=3, frame=1, pos=pos, gen_step=tl + c.get("gen_rel", -1), trailing_len=tl, max_seq=max_seq, rope_delta=rd,
                   done=c.get("done", 0), text_open=c.get("text_open", 0), eos_id=V0 - 7)
        st["trailing_text"], st["tts_pad"] = ("trail", (GUARD + l * (T_ROWS + 1)) * H), ("pad", (GUARD + 2 * l) * H)
        sts.append(st)
        mem.states[f"l{l}"] = st
        used_rope.add(min(max(c["pos_delta"], 0), ROPE_LEN - 1))
    mem.bufs["cos"], cos_off = guarded_rows(ROPE_LEN, 64, "f32", lambda r: values(g, 64, "f32") if r in used_rope else None)
    mem.bufs["sin"], sin_off = guarded_rows(ROPE_LEN, 64, "f32", lambda r: values(g, 64, "f32") if r in used_rope else None)
    mem.bufs["trail"] = sent((2 * GUARD + B * (T_ROWS + 1)) * H, dt)
    mem.bufs["pad"] = sent((2 * GUARD + 2 * B) * H, dt)
    mem.bufs["x"] = sent((B + 2 * GUARD) * H, dt)
    mem.bufs["rope_now"] = sent((B + 2 * GUARD) * HEAD_DIM, "f32")
    perm = torch.randperm(B, generator=g).tolist()
    mem.bufs["codes"] = isent(B * (frames + 2 * GUARD) * 16)
    steps, t_st, t_codes = [], [], []
    for l, (c, st) in enumerate(zip(lanes, sts)):
        codes = ("codes", (perm[l] * (frames + 2 * GUARD) + GUARD) * 16)
        sl(mem, codes, frames * 16)[16:32] = torch.tensor(ids[l], dtype=torch.int32)
        runs = st["done"] == 0 and st["pos"] < st["max_seq"] - 1
        if runs and 0 <= st["gen_step"] < st["trailing_len"]:
            tt = st["trailing_text"]
            sl(mem, (tt[0], tt[1] + st["gen_step"] * H), H)[:] = values(g, H, dt)
        elif runs:
            sl(mem, st["tts_pad"], H)[:] = values(g, H, dt)
        t_st.append((f"$l{l}", 0))
        t_codes.append(codes)
        if not batch:
            steps.append(Launch("embed_sum", dt, p=[(f"$l{l}", 0), codes, ("cos", cos_off), ("sin", sin_off), ("rope_now", (GUARD + l) * HEAD_DIM),
                                                    ("x", (GUARD + l) * H)], tab={0: tabs}, n=[H, ROPE_LEN, st["rope_delta"], V0, V1, frames, T_ROWS],
                                note=str(c)))
    if batch:
        steps = [Launch("embed_sum_batch", dt, p=[("x", GUARD * H), ("cos", cos_off), ("sin", sin_off), ("rope_now", GUARD * HEAD_DIM)],
                        tab={0: t_st, 1: t_codes, 2: tabs}, n=[H, ROPE_LEN, V0, V1, frames, T_ROWS, B], note=f"B {B}")]
    return Case(f"embed_sum{'_batch' if batch else ''} {dt} H {H} B {B} #{seed}", mem, steps)


def embed_lanes(B):
    base = [dict(pos_delta=-3), dict(pos_delta=0, gen_rel=0), dict(pos_delta=ROPE_LEN - 1), dict(pos_delta=ROPE_LEN, gen_rel=0, trailing_len=0),
            dict(pos_delta=ROPE_LEN + 5, gen_rel=2), dict(pos_delta=4, last=True), dict(pos_delta=4, stop=True), dict(pos_delta=3, done=1),
            dict(pos_delta=3, done=2, text_open=1), dict(pos_delta=5, gen_rel=-3)]
    return [dict(base[l % len(base)]) for l in range(B)]


def embed_sum_cases(dt):
    cs = []
    for H in (8, 264, 1024, 2048, 2056):
        cs.append(embed_sum_case(dt, H, [dict(pos_delta=2), dict(pos_delta=ROPE_LEN - 1, gen_rel=0)], False, 0))
    cs.append(embed_sum_case(dt, 264, embed_lanes(10), False, 1))
    for B in (1, 3, 128):
        cs.append(embed_sum_case(dt, 264, embed_lanes(B) if B > 1 else [dict(pos_delta=-3)], True, 2))
    cs.append(embed_sum_case(dt, 2056, embed_lanes(3), True, 3))
    return cs


# ---- cases: rmsnorm_kernel and copy_kernel -----------------------------------------------------------------------------------------------
def rmsnorm_cases(dt):
    """one row of K elements; the seed rotates through the operand sets of _rows_ref.norm_rows_input (wide-range, all equal, mean =
    100 std -- the cancelling one --, zero)"""
    cs = []
    for K in (1, 255, 256, 257, 1024, 2048):
        for seed in range(4):
            pb = RR.rmsnorm(dict(C=K, rows=1, row_lo=0, NS=1, seed=seed), dt, kind="rmsnorm_kernel")
            cs.append(Case(f"rmsnorm {dt} K {K} {RR.ROW_SETS[seed % 4]}", Mem(), [], pb=pb))
    return cs


def copy_cases(dt):
    cs = []
    for n in (1, 8, 257, 264, 1024, 2056):
        g = gen("copy", dt, n)
        mem = Mem()
        mem.bufs["src"] = sent(n + 16, dt)
        mem.bufs["src"][8:8 + n] = rand_words(g, n, dt)
        mem.bufs["dst"] = sent(n + 16, dt)
        cs.append(Case(f"copy {dt} n {n}", mem, [Launch("copy", dt, p=[("dst", 8), ("src", 8)], n=[n])]))
    return cs


# ---- cases: the prompt builder -----------------------------------------------------------------------------------------------------------
def text_gather_cases(dt):
    cs = []
    vocab = 23
    for Ht in (8, 264, 1024, 2048, 2056):
        g = gen("tg", dt, Ht)
        ids = [0, vocab - 1, -1, -(1 << 40), vocab, (1 << 33) + 2, 7, 7, 11]
        mem = Mem()
        mem.bufs["table"], off = table(g, vocab, Ht, dt, {min(max(i, 0), vocab - 1) for i in ids})
        mem.bufs["ids"] = torch.cat([isent(2, torch.int64), torch.tensor(ids, dtype=torch.int64), isent(2, torch.int64)])
        mem.bufs["out"] = sent((len(ids) + 2 * GUARD) * Ht, dt)
        cs.append(Case(f"text_gather {dt} Ht {Ht}", mem, [Launch("text_gather", dt, p=[("ids", 2), ("table", off), ("out", GUARD * Ht)],
                                                                 n=[len(ids), Ht, vocab])]))
    return cs


N_TEXT, N_REF = 5, 4


def prompt_rows_case(dt, H, n_text, n_ref, seed=0):
    """One launch whose prog holds every (kind 0..4) x (trow -1, 0, n_text - 1, n_text) x (arg -1, 0, last, last + 1), `last` being the
    last valid argument of the kind.  The text rows and reference frames are laid out for N_TEXT / N_REF whatever n_text / n_ref the launch
    states; the rows in front of ref_codes (its guard) hold out-of-range ids, which clamp to rows 0 and last of the tables: those hold the
    sentinel here when n_ref = 0, so a kernel that reads frame -1 gives NaN and stays inside the allocation."""
    g = gen("pr", dt, H, n_text, n_ref, seed)
    mem = Mem()
    prog = []
    for kind in range(5):
        last = {1: V0 - 1, 3: N_REF - 1}.get(kind, 3)
        for trow in (-1, 0, N_TEXT - 1, N_TEXT):
            for arg in (-1, 0, last, last + 1):
                prog += [trow, kind, arg]
    n_rows = len(prog) // 3
    ref = torch.stack([torch.randint(0, V0 if j == 0 else V1, (N_REF,), generator=g) for j in range(16)], dim=1)       # [N_REF][16]
    ref[0, 3], ref[1, 0], ref[N_REF - 1, 5], ref[N_REF - 1, 0] = -4, V0 + 9, V1, 0                                       # ids that clamp
    ref[0, 7], ref[N_REF - 1, 9] = 0, V1 - 1
    guard_ids = torch.tensor([-(1 << 35) if j % 2 else (1 << 35) for j in range(16)], dtype=torch.int64)
    mem.bufs["ref_codes"] = torch.cat([guard_ids, guard_ids, ref.reshape(-1), guard_ids, guard_ids])
    tabs = []
    for j in range(16):
        Vj = V0 if j == 0 else V1
        used = set()
        if n_ref > 0:
            used |= {min(max(int(ref[f, j]), 0), Vj - 1) for f in (0, n_ref - 1)}
        if j == 0:
            used |= {0, V0 - 1}
        mem.bufs[f"tab{j}"], off = table(g, Vj, H, dt, used)
        tabs.append((f"tab{j}", off))
    mem.bufs["text"], t_off = guarded_rows(N_TEXT, H, dt, lambda r: values(g, H, dt) if (n_text > 0 and r in (0, n_text - 1)) else None)
    mem.bufs["spk"] = sent(H + 16, dt)
    mem.bufs["spk"][8:8 + H] = values(g, H, dt)
    mem.bufs["prog"] = torch.cat([isent(6), torch.tensor(prog, dtype=torch.int32), isent(6)])
    mem.bufs["out"] = sent((n_rows + 2 * GUARD) * H, dt)
    L = Launch("prompt_rows", dt, p=[("text", t_off), ("prog", 6), ("ref_codes", 32), ("spk", 8), ("out", GUARD * H)], tab={0: tabs},
               n=[n_text, n_rows, n_ref, V0, V1, H], note=f"n_text {n_text} n_ref {n_ref}")
    return Case(f"prompt_rows {dt} H {H} n_text {n_text} n_ref {n_ref}", mem, [L])


def prompt_rows_cases(dt):
    cs = [prompt_rows_case(dt, H, N_TEXT, N_REF) for H in (8, 264, 1024, 2048, 2056)]
    cs += [prompt_rows_case(dt, 264, 0, N_REF), prompt_rows_case(dt, 264, N_TEXT, 0), prompt_rows_case(dt, 2056, N_TEXT, 0)]
    return cs


# ---- cases: the text table, the poll and the small host-side kernels ----------------------------------------------------------------------
def text_table_cases():
    cs = []
    for words in (0, 1, 255, 256, 257, 1056):
        g = gen("to", words)
        mem = Mem()
        mem.bufs["rows"] = torch.cat([isent(4), torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), generator=g, dtype=torch.int64).to(torch.int32), isent(4)])
        mem.bufs["table"] = isent(words + 64)
        mem.states["s"] = state(token=5, frame=2, trailing_len=3, gen_step=1, trailing_text=("rows", 4), tts_pad=("rows", 0))
        cs.append(Case(f"text_open words {words}", mem, [Launch("text_open", p=[("$s", 0), ("table", 8), ("rows", 4)], n=[words, words + 56])]))
    for rows, final, open_ in ((7, 0, 1), (7, 1, 1), (0, 1, 1), (9, 0, 0)):
        mem = Mem()
        mem.states["s"] = state(token=5, frame=2, trailing_len=3, gen_step=1, text_open=open_, done=2)
        cs.append(Case(f"text_publish rows {rows} final {final}", mem, [Launch("text_publish", p=[("$s", 0)], n=[rows, final])]))
    return cs


def scatter_cases():
    """first lists: an empty first item, an empty middle item, an empty last item, a single item, 128 items"""
    cs = []
    lists = {"empty first": [0, 0, 2, 5], "empty middle": [0, 2, 2, 5], "empty last": [0, 3, 5, 5], "single": [0, 4],
             "empty first, middle and last": [0, 0, 1, 1, 1, 4, 4], "128 items": None}
    for name, first in lists.items():
        for row_vec in ((1, 33, 257) if first is not None else (33,)):
            g = gen("sc", name, row_vec)
            if first is None:
                cnt = [int(torch.randint(0, 3, (1,), generator=g)) for _ in range(MAX_LANES)]
                cnt[0], cnt[5], cnt[MAX_LANES - 1] = 0, 2, 0
                first = [0]
                for c in cnt:
                    first.append(first[-1] + c)
            items, N, w = len(first) - 1, first[-1], row_vec * 4
            mem = Mem()
            mem.bufs["y"] = torch.cat([isent(w), torch.randint(-2 ** 31, 2 ** 31 - 1, (N * w,), generator=g, dtype=torch.int64).to(torch.int32), isent(w)])
            cap = 4
            mem.bufs["dst"] = isent((items * (cap + 1) + 1) * w)
            perm = torch.randperm(items, generator=g).tolist()
            dst = [("dst", (perm[i] * (cap + 1) + 1) * w) for i in range(items)]
            cs.append(Case(f"text_scatter {name} row_vec {row_vec}", mem,
                           [Launch("text_scatter", p=[("y", w)], tab={0: dst}, iv=list(first), iv2=[cap] * items, n=[items, row_vec, N])]))
    return cs


def lane_states(B, seed):
    g = gen("ls", B, seed)
    sts = {}
    for l in range(B):
        done = (0, 1, 2, 0)[l % 4]
        eos = 40 + l
        sts[f"l{l}"] = state(token=eos if l % 8 == 3 else 3 + l, frame=l * 3 + 1, done=done, eos_id=eos, trailing_len=2 + l, text_open=int(done != 1),
                             gen_step=int(torch.randint(0, 9, (1,), generator=g)))
    return sts


def poll_and_publish_cases():
    cs = []
    for B in (1, 3, 128):
        mem = Mem(states=lane_states(B, 0))
        mem.bufs["out"] = isent(2 * MAX_LANES + 8)
        cs.append(Case(f"poll_gather B {B}", mem, [Launch("poll_gather", p=[("out", 4)], tab={0: [(f"$l{l}", 0) for l in range(B)]}, n=[B])]))
    for B, named in ((1, [0]), (5, [3, 1]), (5, []), (128, list(range(127, -1, -1)))):
        mem = Mem(states=lane_states(B, 1))
        rows = [100 + 2 * i for i in named]
        closes = [(i + len(named)) % 3 == 0 for i in range(len(named))]
        cs.append(Case(f"text_publish_lanes B {B} items {len(named)}", mem,
                       [Launch("text_publish_lanes", tab={0: [(f"$l{l}", 0) for l in named]}, iv=rows, iv2=[int(c) for c in closes], n=[len(named)])]))
    return cs


def host_side_cases():
    cs = []
    for first, count in ((0, 0), (0, 1), (3, 5), (1, 128)):
        mem = Mem()
        mem.bufs["table"] = isent(140)
        cs.append(Case(f"kv_table_write first {first} count {count}", mem,
                       [Launch("kv_table_write", p=[("table", 4)], iv=[1000 + 7 * i for i in range(count)], n=[first, count, 132])]))
    for dt in DTS:
        for H in (8, 264, 2056):
            g = gen("arm", dt, H)
            words = H * esz(dt) // 4
            mem = Mem()
            mem.bufs["seen"] = isent(MAX_VOCAB + 64, torch.uint8)
            mem.bufs["ph"] = isent(words + 8)
            mem.bufs["src"] = torch.cat([isent(4), torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), generator=g, dtype=torch.int64).to(torch.int32), isent(4)])
            mem.states["s"] = state(token=9, frame=4, done=1, text_open=1, trailing_len=8, trailing_text=("src", 0), rope_delta=-5)
            init = state(token=17, pos=33, gen_step=2, min_new=2, max_new=200, trailing_len=4, noise_frames=3, eos_id=V0 - 7, max_seq=512, sup_lo=64,
                         sup_hi=96, t_temperature=0.9, t_top_k=50, t_top_p=0.95, t_do_sample=1, t_rep_penalty=1.05, trailing_text=("src", 4),
                         tts_pad=("src", 5), talker_noise=("src", 6), pred_noise=("src", 7), n_pad=1, rope_delta=-3)
            cs.append(Case(f"decode_arm {dt} H {H}", mem, [Launch("decode_arm", p=[("$s", 0), ("seen", 32), ("ph", 4), ("src", 4)], host=init,
                                                                  n=[MAX_VOCAB, words, MAX_VOCAB + 32, words + 4])]))
    mem = Mem()
    mem.bufs["forced"], mem.bufs["dec"] = isent(40), isent(40)
    mem.tfs["t"] = {"forced": None, "decisions": None}
    cs.append(Case("decode_set_forced", mem, [Launch("decode_set_forced", p=[("&t", 0), ("forced", 3), ("dec", 5)]),
                                              Launch("decode_set_forced", p=[("&t", 0), None, ("dec", 7)]),
                                              Launch("decode_set_forced", p=[("&t", 0), None, None])]))
    for done in (0, 1, 2):
        mem = Mem()
        mem.states["s"] = state(token=9, frame=4, done=done, text_open=1, trailing_len=8, rope_delta=-5)
        cs.append(Case(f"decode_cancel done {done}", mem, [Launch("decode_cancel", p=[("$s", 0)])]))
    for n in (1, 16, 255, 256, 257, 48 * 16):
        g = gen("c64", n)
        mem = Mem()
        mem.bufs["src"] = torch.cat([isent(4), torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32), isent(4)])
        mem.bufs["dst"] = isent(n + 8, torch.int64)
        cs.append(Case(f"codes_to_i64 n {n}", mem, [Launch("codes_to_i64", p=[("src", 4), ("dst", 4)], n=[n])]))
    return cs


# ---- cases: KV ---------------------------------------------------------------------------------------------------------------------------
def rand_words(g, n, dt):
    """n elements of storage type dt with random bit patterns"""
    b = RR.rand_bits(g, dt, n)
    if dt == "bf16":
        return torch.where(b >= (1 << 15), b - (1 << 16), b).to(torch.int16).view(torch.bfloat16)
    return torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32).view(torch.float32)


def kv_copy_cases(dt):
    cs = []
    for L in (1, 63, 64, 65, 130):
        for n_kv in (1, 2):
            for export in (False, True):
                g = gen("kv", dt, L, n_kv, export)
                nb = (L + KEYS_PER_TILE - 1) // KEYS_PER_TILE
                blocks = nb + 3
                blk_stride = n_kv * KEYS_PER_TILE * HEAD_DIM + (64 if n_kv == 1 else 0)        # (a stride wider than the block)
                tb = torch.randperm(blocks, generator=g)[:nb].tolist()
                mem = Mem()
                mem.bufs["table"] = torch.cat([isent(2), torch.tensor(tb, dtype=torch.int32), isent(2)])
                dense_n = n_kv * L * HEAD_DIM
                if export:
                    mem.bufs["cache"] = rand_words(g, blocks * blk_stride, dt)
                    mem.bufs["dense"] = sent(dense_n + 2 * HEAD_DIM, dt)
                else:
                    mem.bufs["cache"] = sent(blocks * blk_stride, dt)
                    mem.bufs["dense"] = torch.cat([sent(HEAD_DIM, dt), rand_words(g, dense_n, dt), sent(HEAD_DIM, dt)])
                cs.append(Case(f"kv_{'export' if export else 'import'} {dt} L {L} n_kv {n_kv}", mem,
                               [Launch("kv_export" if export else "kv_import", dt, p=[("cache", 0), ("table", 2), ("dense", HEAD_DIM)],
                                       n=[blk_stride, n_kv, L, blocks, nb])]))
    return cs


def kv_adopt_cases(dt):
    cs = []
    for L, layers, n_kv in ((1, 2, 1), (63, 2, 2), (64, 2, 1), (65, 2, 1), (130, 2, 2), (65, 64, 1)):
        g = gen("adopt", dt, L, layers)
        nb = (L + KEYS_PER_TILE - 1) // KEYS_PER_TILE
        be = n_kv * KEYS_PER_TILE * HEAD_DIM
        if layers == 64:
            be = 8 * (16 // esz(dt))                       # the most layers the table admits: small blocks keep the case quick
        db, sb = nb + 2, nb + 3
        dtab, stab = torch.randperm(db, generator=g)[:nb].tolist(), torch.randperm(sb, generator=g)[:nb].tolist()
        if nb > 1 and dtab == stab[:nb]:
            stab = stab[::-1]
        mem = Mem()
        mem.bufs["dtab"] = torch.cat([isent(2), torch.tensor(dtab, dtype=torch.int32), isent(2)])
        mem.bufs["stab"] = torch.cat([isent(2), torch.tensor(stab, dtype=torch.int32), isent(2)])
        n_which = 2 * layers
        mem.bufs["dst"] = sent(n_which * db * be, dt)
        mem.bufs["src"] = rand_words(g, n_which * sb * be, dt)
        perm = torch.randperm(n_which, generator=g).tolist()
        cs.append(Case(f"kv_adopt {dt} L {L} layers {layers}", mem,
                       [Launch("kv_adopt", dt, p=[("dtab", 2), ("stab", 2)],
                               tab={0: [("dst", perm[w] * db * be) for w in range(n_which)], 1: [("src", w * sb * be) for w in range(n_which)]},
                               n=[n_which, nb, be, db, sb, nb])]))
    return cs


# ---- trajectories ----------------------------------------------------------------------------------------------------------------------
# A lane's script: per FRAME the token the talker sampler is made to give at its end (a planted maximum), the predictor codes the test
# plants and the hidden state the stack leaves (a step that does not run a frame leaves junk there, as a held frame's stack does); the
# text rows and when they are published, and the cancel.  Events are (step, what, ...) applied before frame_begin of that step.
TRAJ_H, TRAJ_V, TRAJ_STEPS = 264, 64, 10
TRAJ_EOS = 61
SCRIPTS = {
    # holds entered and left twice (rows arriving late), one row exactly on time, EOS sampled by the frame that leaves the second hold
    "A": dict(open=True, begin_rows=2, text_rows=5, max_new=12, max_seq_slack=40, rope_delta=-2, tokens=[7, 0, 63, 13, TRAJ_EOS, 4, 4, 4, 4, 4, 4, 4],
              events=[(4, "publish", 3, 0), (5, "publish", 4, 0), (7, "publish", 5, 0)]),
    # a final publish with no rows closes the table: the pad row from then on; max_new reached
    "B": dict(open=True, begin_rows=1, text_rows=1, max_new=4, max_seq_slack=40, rope_delta=3, tokens=[5, 6, 0, 63, 8, 8, 8, 8, 8, 8, 8, 8],
              events=[(1, "publish", 1, 1)]),
    # a fixed table (never opened), the position limit reached
    "C": dict(open=False, begin_rows=2, text_rows=2, max_new=12, max_seq_slack=3, rope_delta=-4, tokens=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12],
              events=[]),
    # cancel while held; a publish after it changes the length and nothing else
    "D": dict(open=True, begin_rows=1, text_rows=3, max_new=12, max_seq_slack=40, rope_delta=0, tokens=[9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 63, 62],
              events=[(3, "cancel"), (5, "publish", 3, 1)]),
}
PAIRS = (("A", "B"), ("C", "D"))


def traj_lane(mem, name, dt, slot, n_slots, g):
    """The buffers of one lane: the script's data and the references of its buffers."""
    sc = SCRIPTS[name]
    H = TRAJ_H
    d = dict(name=name, sc=sc)
    d["pcodes"] = [[int(torch.randint(0, V1, (1,), generator=g)) for _ in range(15)] for _ in range(TRAJ_STEPS)]
    d["junk"] = [values(g, H, dt) for _ in range(TRAJ_STEPS)]
    d["first"] = int(torch.randint(0, TRAJ_V - 8, (1,), generator=g))
    d["ph_vals"] = [values(g, H, dt) for _ in range(TRAJ_STEPS + 1)]        # [0]: initial; then one per step (the stack's output, held or not)
    d["text_vals"] = [values(g, H, dt) for _ in range(sc["text_rows"])]
    d["pad_val"] = values(g, H, dt)
    d.update(lane_buffers_t(mem, name, dt, slot, n_slots))
    return d


def lane_buffers_t(mem, name, dt, slot, n_slots):
    H, G_ = TRAJ_H, 16
    frames = TRAJ_STEPS + 1
    need = {"codes": ((frames + 2 * GUARD) * G_, torch.int32, GUARD * G_), "seen": (TRAJ_V + 32, torch.uint8, 16), "ph": (H + 16, None, 8),
            "hold": (H + 16, None, 8), "begin": (8 * H, None, H), "ttab": (8 * H, None, H), "pad": (H + 16, None, 8), "logits": (TRAJ_V + 16, None, 8)}
    refs = {}
    for k, (cnt, ity, lead) in need.items():
        if k not in mem.bufs:
            mem.bufs[k] = isent(cnt * n_slots, ity) if ity is not None else sent(cnt * n_slots, dt)
        refs[k] = (k, slot * cnt + lead)
    return refs


def trajectory_case(pair, dt, batch):
    """Up to TRAJ_STEPS steps of frame_begin -> (codes 1..15 planted) -> embed_sum -> (the stack's part: a new past_hidden) -> talker_step
    for the lanes of `pair`, one after the other (single-stream kernels) or in lock-step (batch kernels), over the same scripts."""
    g = gen("traj", pair, dt)                              # (the same data for the single and the batch form)
    mem = Mem()
    H, G_ = TRAJ_H, 16
    B = len(pair)
    perm = {2: [1, 0], 1: [0]}[B]
    lanes = [traj_lane(mem, nm, dt, perm[i], B, g) for i, nm in enumerate(pair)]
    # tables: the rows the scripts name hold values, all others the sentinel
    used0 = set()
    for d in lanes:
        used0 |= {d["first"]} | set(d["sc"]["tokens"])
    tabs = []
    mem.bufs["tab0"], off = table(g, TRAJ_V, H, dt, used0)
    tabs.append(("tab0", off))
    for j in range(1, 16):
        mem.bufs[f"tab{j}"], off = table(g, V1, H, dt, {d["pcodes"][s][j - 1] for d in lanes for s in range(TRAJ_STEPS)})
        tabs.append((f"tab{j}", off))
    rope_len = 64
    mem.bufs["cos"], cos_off = guarded_rows(rope_len, 64, "f32", lambda r: values(g, 64, "f32"))
    mem.bufs["sin"], sin_off = guarded_rows(rope_len, 64, "f32", lambda r: values(g, 64, "f32"))
    mem.bufs["pred_in"] = sent((B + 2 * GUARD) * 2 * H, dt)
    mem.bufs["x"] = sent((B + 2 * GUARD) * H, dt)
    mem.bufs["rope_now"] = sent((B + 2 * GUARD) * HEAD_DIM, "f32")
    steps = []
    frames = TRAJ_STEPS + 1
    for l, d in enumerate(lanes):
        sc = d["sc"]
        pos0 = 20 + 3 * l
        for r in range(sc["begin_rows"]):
            sl(mem, (d["begin"][0], d["begin"][1] + r * H), H)[:] = d["text_vals"][r]
        sl(mem, d["pad"], H)[:] = d["pad_val"]
        sl(mem, d["ph"], H)[:] = d["ph_vals"][0]
        sl(mem, d["seen"], TRAJ_V)[:] = 0
        d["st"] = f"${d['name']}"
        mem.states[d["name"]] = state(token=d["first"], pos=pos0, gen_step=0, max_new=sc["max_new"], trailing_len=sc["begin_rows"], eos_id=TRAJ_EOS,
                                      max_seq=pos0 + sc["max_seq_slack"], rope_delta=sc["rope_delta"], trailing_text=d["begin"], tts_pad=d["pad"])
        if sc["open"]:
            words = sc["begin_rows"] * H * esz(dt) // 4
            steps.append(Launch("text_open", dt, p=[(d["st"], 0), d["ttab"], d["begin"]], n=[words, 6 * H * esz(dt) // 4], note=f"lane {d['name']}"))
    t_st = [(d["st"], 0) for d in lanes]
    for step in range(TRAJ_STEPS):
        for l, d in enumerate(lanes):
            for ev in d["sc"]["events"]:
                if ev[0] != step:
                    continue
                if ev[1] == "cancel":
                    steps.append(Launch("decode_cancel", p=[(d["st"], 0)], note=f"lane {d['name']} step {step}"))
                else:
                    rows, final = ev[2], ev[3]
                    have = max([e[2] for e in d["sc"]["events"] if e[1] == "publish" and e[0] < step] + [d["sc"]["begin_rows"]])
                    for r in range(have, rows):             # the rows first (the projection's part), then the length
                        steps.append(Write(d["ttab"][0], d["ttab"][1] + r * H, d["text_vals"][r]))
                    if batch:
                        steps.append(Launch("text_publish_lanes", tab={0: [(d["st"], 0)]}, iv=[rows], iv2=[final], n=[1], note=f"lane {d['name']} step {step}"))
                    else:
                        steps.append(Launch("text_publish", p=[(d["st"], 0)], n=[rows, final], note=f"lane {d['name']} step {step}"))
        fb, es = [], []
        for l, d in enumerate(lanes):
            fb.append(Launch("frame_begin", dt, p=[(d["st"], 0), d["ph"], tabs[0], ("pred_in", (GUARD + l) * 2 * H), d["codes"], d["seen"], d["hold"]],
                             n=[H, G_, TRAJ_V, frames], note=f"lane {d['name']} step {step}"))
            es.append(Launch("embed_sum", dt, p=[(d["st"], 0), d["codes"], ("cos", cos_off), ("sin", sin_off), ("rope_now", (GUARD + l) * HEAD_DIM),
                                                 ("x", (GUARD + l) * H)], tab={0: tabs}, n=[H, rope_len, d["sc"]["rope_delta"], TRAJ_V, V1, frames, 6],
                             note=f"lane {d['name']} step {step}"))
        if batch:
            fb = [Launch("frame_begin_batch", dt, p=[tabs[0], ("pred_in", GUARD * 2 * H)],
                         tab={0: t_st, 1: [d["codes"] for d in lanes], 2: [d["seen"] for d in lanes], 3: [d["ph"] for d in lanes],
                              4: [d["hold"] for d in lanes]}, n=[H, G_, TRAJ_V, frames, B], note=f"step {step}")]
            es = [Launch("embed_sum_batch", dt, p=[("x", GUARD * H), ("cos", cos_off), ("sin", sin_off), ("rope_now", GUARD * HEAD_DIM)],
                         tab={0: t_st, 1: [d["codes"] for d in lanes], 2: tabs}, n=[H, rope_len, TRAJ_V, V1, frames, 6, B], note=f"step {step}")]
        steps += fb
        steps.append(("plant", step))                      # resolved below: the predictor's codes go to the frame the state names NOW
        steps += es
        for l, d in enumerate(lanes):
            steps.append(("stack", step, l))               # resolved below: past_hidden is overwritten, held or not; the logits
            steps.append(Launch("talker_step", dt, p=[(d["st"], 0), d["logits"], d["seen"]], n=[TRAJ_V, G_], note=f"lane {d['name']} step {step}"))
    return Case(f"trajectory {'+'.join(pair)} {dt} {'batch' if batch else 'single'}", mem, resolve_plants(mem, steps, lanes), lanes=lanes)


def resolve_plants(mem, steps, lanes):
    """The predictor's part: codes 1..15 of the frame each lane's state names after frame_begin, written by the host.  Which frame that is
    depends on the run so far, so the model is run along to place the writes (a lane that does not run the frame gets none)."""
    m = mem.clone()
    out = []

    def put(w):
        m.bufs[w.buf][w.off:w.off + w.data.numel()] = w.data
        out.append(w)

    for s in steps:
        if isinstance(s, tuple) and s[0] == "plant":
            for d in lanes:
                st = m.states[d["name"]]
                if st["done"] == 0:
                    put(Write(d["codes"][0], d["codes"][1] + st["frame"] * 16 + 1, torch.tensor(d["pcodes"][st["frame"]], dtype=torch.int32)))
            continue
        if isinstance(s, tuple):
            d = lanes[s[2]]
            st = m.states[d["name"]]
            ran = st["done"] == 0                           # (after embed_sum: neither held, nor finished, nor at the position limit)
            put(Write(d["ph"][0], d["ph"][1], d["ph_vals"][st["frame"] + 1] if ran else d["junk"][s[1]]))
            lg = torch.linspace(-1.0, 1.0, TRAJ_V).to(m.bufs[d["logits"][0]].dtype).clone()
            lg[d["sc"]["tokens"][min(st["frame"], TRAJ_STEPS - 1)]] = 4.0
            put(Write(d["logits"][0], d["logits"][1], lg))
            continue
        if isinstance(s, Write):
            m.bufs[s.buf][s.off:s.off + s.data.numel()] = s.data
        else:
            apply(m, s)
        out.append(s)
    return out


def trajectory_cases(dt):
    return [trajectory_case(pair, dt, batch) for pair in PAIRS for batch in (False, True)]


def lane_view(mem, d):
    """What one lane of a trajectory owns, by bits, wherever it lies: for the comparison of the single-stream and the batch run"""
    H = TRAJ_H
    out = {k: bits(sl(mem, d[k], n)).clone() for k, n in (("codes", (TRAJ_STEPS + 1) * 16), ("seen", TRAJ_V), ("hold", H), ("ttab", 6 * H))}
    out["state"] = {f: v for f, v in mem.states[d["name"]].items()}
    return out


# ---- the suite -----------------------------------------------------------------------------------------------------------------------
def all_cases():
    cs = []
    for dt in DTS:
        cs += frame_begin_cases(dt) + embed_sum_cases(dt) + rmsnorm_cases(dt) + copy_cases(dt) + text_gather_cases(dt) + prompt_rows_cases(dt)
        cs += kv_copy_cases(dt) + kv_adopt_cases(dt) + trajectory_cases(dt)
    cs += text_table_cases() + scatter_cases() + poll_and_publish_cases() + host_side_cases()
    return cs


MUTANTS = ("no_hold_copy", "ph_hold_ignored", "frame_gt_max_new", "pos_ge_max_seq", "text_row_by_frame", "rope_clamp_low", "rope_clamp_high",
           "lane_rope_delta_ignored", "pred_in_stride_h", "codes_slot_plus_1", "trow_le_n_text", "kind3_not_rounded", "no_n_ref_guard",
           "scatter_first_item", "poll_held_as_finished", "block_and_row_swapped", "source_by_destination_table")
