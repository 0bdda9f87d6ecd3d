"""Conformance of every sampler kernel with the float64 reference of tests/_sampler_ref.py.

Each launch goes alone through tools/microbench/libsampler_probe.so, on sentinel-filled outputs.  Every logits and noise row has slack
behind V that holds the largest finite logit and the smallest positive noise, so an id >= V that a kernel fails to mask wins and is
seen; the noise rings hold more (distinct) rows than noise_frames, so a row index without the modulo stays inside the buffer and gives
another token.  Asserted per launch: the token by the checker's rule (equal to the reference on a decided case, one of the three
scalings' tokens otherwise), read from out / codes / out64 / st->token / decisions[slot]; the exact codes slot with every other
element still the sentinel; next_in bit-equal to row `tok` of the table with the sentinel behind H; the whole DecodeState byte for
byte (token, frame + 1, pos + 1, gen_step + 1 for the talker; nothing for the predictor); with done != 0 no byte of any output; and on
decided cases the register kind, the LDS kind and the batch kind of one case give the same token.

The last test prints the per-family record and asserts that every instantiation the probe builds was launched.
Observed on the MI355X (a record: nothing is tuned to it; "cases" counts every scored token, a batch launch scores one per lane):
  kernel                           cases  launches   decided share
  sample_api_kernel                 1248      1248          0.9744
  sample_api_wave_kernel            1580      1580          0.9861
  sample_pred_kernel                2014      2078          0.9682
  sample_pred_wave_kernel           1662      1726          0.9795
  sample_talker_kernel              1472      1504          0.9783
  sample_talker_wave_kernel         1280      1312          0.9867
  sample_pred_batch_kernel          1528       140          0.9679
  sample_talker_batch_kernel        1826       146          0.9775
  fq3_sample + history               208         -          1.0000
  Instantiations launched: 26 of 26 (three LDS kernels and five register kernels with NC = 1 and 2, each in bf16 and fp32).
  The undecided cases are the planted exact ties in fp32 (equal logits and equal noise across a lane, wave or chunk boundary; a
  cumulative sum equal to top_p): the rule's bounds at p (1 -+ E) overlap there by construction, and all three scalings give one
  token, which every kernel returned.
One defect found: with the k-th value a zero, both cores dropped the -0.0 candidates the reference keeps (okey() ordered -0.0 below
+0.0).  The signed-zero cases failed on all eight kernels in both storage types -- e.g. V = 8: token 6 (bf16) / 5 (fp32) where the
reference gives 0 -- and pass since okey() gives -0.0 the key of +0.0 (csrc/sampler.cuh).  Nothing else failed: no stray write, no id
>= V, no state byte out of place.
"""
import ctypes as C
import os
from collections import defaultdict
from dataclasses import replace

import numpy as np
import pytest
import torch

import _sampler_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libsampler_probe.so")
K_API, K_API_WAVE, K_PRED, K_PRED_WAVE, K_TALKER, K_TALKER_WAVE, K_PRED_BATCH, K_TALKER_BATCH = range(8)
KIND_NAME = ("sample_api_kernel", "sample_api_wave_kernel", "sample_pred_kernel", "sample_pred_wave_kernel", "sample_talker_kernel",
             "sample_talker_wave_kernel", "sample_pred_batch_kernel", "sample_talker_batch_kernel")
REG = (K_API_WAVE, K_PRED_WAVE, K_TALKER_WAVE, K_PRED_BATCH, K_TALKER_BATCH)
TE = {"bf16": 0, "f32": 2}
TDT = {"bf16": torch.bfloat16, "f32": torch.float32}
REFUSED = 100000
SENT32, SENT64 = -1515870811, -6510615555426900571          # 0xA5A5A5A5 patterns
vp, i32, f32c = C.c_void_p, C.c_int32, C.c_float


class SampleCfg(C.Structure):
    _fields_ = [("temperature", f32c), ("top_k", i32), ("top_p", f32c), ("do_sample", i32), ("rep_penalty", f32c), ("sup_lo", i32),
                ("sup_hi", i32), ("keep_id", i32), ("sup_extra", i32)]


class DecodeState(C.Structure):
    _fields_ = [("token", i32), ("frame", i32), ("pos", i32), ("gen_step", i32), ("done", i32), ("text_open", i32), ("min_new", i32),
                ("max_new", i32), ("trailing_len", i32), ("noise_frames", i32), ("eos_id", i32), ("max_seq", i32), ("sup_lo", i32),
                ("sup_hi", i32), ("t_temperature", f32c), ("t_top_k", i32), ("t_top_p", f32c), ("t_do_sample", i32), ("t_rep_penalty", f32c),
                ("p_temperature", f32c), ("p_top_k", i32), ("p_top_p", f32c), ("p_do_sample", i32), ("trailing_text", vp), ("tts_pad", vp),
                ("talker_noise", vp), ("pred_noise", vp), ("past_hidden_init", vp), ("n_pad", i32), ("rope_delta", i32)]


class TeacherForcing(C.Structure):
    _fields_ = [("forced", vp), ("decisions", vp)]


class SamplerProbeArgs(C.Structure):
    _fields_ = [("V", i32), ("H", i32), ("G", i32), ("B", i32), ("cb", i32), ("nc", i32), ("n_hist", i32), ("noise_rows", i32),
                ("codes_len", i32), ("tf_len", i32), ("logit_stride", C.c_long), ("cfg", SampleCfg), ("logits", vp), ("noise", vp),
                ("seen", vp), ("history", vp), ("out", vp), ("st", vp), ("codes", vp), ("out64", vp), ("next_emb", vp), ("next_in", vp),
                ("tf", vp), ("lane_st", C.POINTER(vp)), ("lane_codes", C.POINTER(vp)), ("lane_seen", C.POINTER(vp)),
                ("lane_tf", C.POINTER(vp))]


def layout_of(s):
    return [C.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_]


STATS = defaultdict(lambda: {"cases": 0, "decided": 0, "launches": 0})
REACHED = set()
TOKENS = {}                        # case name -> the token its first launch gave (decided cases: every kind must agree)


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libsampler_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.sampler_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(SamplerProbeArgs), vp]
    lib.sampler_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(SamplerProbeArgs)]
    lib.sampler_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    assert lib.sampler_probe_version() == 1 and lib.sampler_probe_kinds() == 8 and lib.sampler_probe_refused_code() == REFUSED
    buf = (C.c_long * 128)()
    n = lib.sampler_probe_layout(buf, 128)
    want = layout_of(DecodeState) + layout_of(SampleCfg) + layout_of(TeacherForcing) + layout_of(SamplerProbeArgs)
    assert list(buf[:n - 2]) == want, "a ctypes mirror of DecodeState / SampleCfg / TeacherForcing / SamplerProbeArgs is out of date"
    assert list(buf[n - 2:n]) == [R.MAX_VOCAB, R.MAX_LANES]
    assert [lib.sampler_probe_rule_nc(V) for V in (8, 2048, 2056, 4096)] == [1, 1, 2, 2]
    return lib


# ---- device images ---------------------------------------------------------------------------------------------------------------------
_DEV = {}


def cached(key, make, alive=None):
    """make() once per key; `alive` (the host object whose id() is part of the key) is held so that the id is not reused."""
    if key not in _DEV:
        _DEV[key] = (make(), alive)
    return _DEV[key][0]


def store(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(TDT[dt]).cuda()


def dev_row(x, dt, slack):
    """A [V] row of T values with SLACK elements of `slack` behind it."""
    return cached(("row", id(x), dt), lambda: store(np.concatenate([x, np.full(R.SLACK, slack)]), dt), x)


def dev_ring(ring, dt):
    return cached(("ring", id(ring), dt), lambda: store(np.concatenate([ring.reshape(-1), np.full(R.SLACK, R.SLACK_NOISE)]), dt), ring)


def dev_seen(seen):
    return cached(("seen", id(seen)), lambda: torch.from_numpy(np.concatenate([seen, np.zeros(R.SLACK, np.uint8)])).cuda(), seen)


def dev_emb(dt, V, H):
    def make():
        g = torch.Generator(device="cuda").manual_seed(V * 7919 + H)
        return torch.randn((V + R.SLACK) * H, generator=g, device="cuda").to(TDT[dt])
    return cached(("emb", dt, V, H), make)


def sent32(n):
    return torch.full((n,), SENT32, dtype=torch.int32, device="cuda")


def sent64(n):
    return torch.full((n,), SENT64, dtype=torch.int64, device="cuda")


def sent_t(n, dt):
    t = sent32(n)
    return t.view(torch.float32) if dt == "f32" else torch.full((n,), -23131, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def upload(struct):
    return torch.frombuffer(bytearray(bytes(struct)), dtype=torch.uint8).cuda()


def ptr(t):
    return t.data_ptr() if t is not None else None


def c_cfg(cfg: R.Cfg):
    return SampleCfg(cfg.temperature, cfg.top_k, cfg.top_p, int(cfg.do_sample), cfg.rep_penalty, cfg.sup_lo, cfg.sup_hi, cfg.keep_id, cfg.sup_extra)


def run(probe, kind, dt, p, what):
    assert probe.sampler_probe_admits(kind, TE[dt], C.byref(p)) == 1, f"{what}: the probe refuses the launch"
    rc = probe.sampler_probe_run(kind, TE[dt], C.byref(p), None)
    if rc not in (0, REFUSED):                   # a HIP error: nothing more is launched in this process
        pytest.exit(f"{what}: the probe returned HIP error {rc}", returncode=3)
    assert rc == 0, f"{what}: the probe returned {rc}"
    REACHED.add(probe.sampler_probe_last_inst())
    STATS[KIND_NAME[kind]]["launches"] += 1


def score(kind, name, v: R.Verdict, tok, what):
    """The checker's rule, the family record, and the agreement of the kinds on decided cases."""
    msg = R.check(v, tok, what)
    assert msg == "", msg
    st = STATS[KIND_NAME[kind]]
    st["cases"] += 1
    st["decided"] += int(v.decided)
    if v.decided:
        assert TOKENS.setdefault(name, tok) == tok, f"{what}: another kind gave {TOKENS[name]} on this decided case"


# ---- stateless cases as in-graph launches ------------------------------------------------------------------------------------------------
def to_graph(c: R.Case, role):
    """The in-graph launch that poses the stateless problem c to a predictor / talker kernel with a state, or None."""
    cfg = c.cfg
    ring = c.noise[None] if c.noise is not None else None
    if role == "pred":
        if c.seen is not None or cfg.sup_lo != cfg.sup_hi or cfg.sup_extra != -1:
            return None
        g = R.GraphCase(c.name, c.dt, c.V, "pred", c.logits, 2, 0, 8, 0, 1, policy=replace(cfg, rep_penalty=1.0, keep_id=-1), ring=ring)
    else:
        if not (cfg.sup_extra == -1 or cfg.sup_extra == cfg.keep_id or cfg.keep_id == -1):
            return None
        eos = cfg.keep_id if cfg.keep_id >= 0 else cfg.sup_extra
        g = R.GraphCase(c.name, c.dt, c.V, "talker", c.logits, 2, 0, 8, 0, 1, min_new=5 if cfg.sup_extra >= 0 else 0, eos_id=eos,
                        sup_lo=cfg.sup_lo, sup_hi=cfg.sup_hi, policy=cfg, ring=ring, seen=c.seen)
        rc = R.resolve(g).cfg
        assert (rc.sup_lo, rc.sup_hi, rc.sup_extra, rc.rep_penalty) == (cfg.sup_lo, cfg.sup_hi, cfg.sup_extra, cfg.rep_penalty)
        assert np.array_equal(R.masked(R.resolve(g)), R.masked(c), equal_nan=True), c.name
    return g


class Lane:
    """The device image of one in-graph launch: state, logits, noise ring, bitmap, codes, forcing object; outputs sentinel-filled."""

    def __init__(self, g: R.GraphCase, outs=("codes", "out64", "emb")):
        self.g, dt = g, g.dt
        self.logits = dev_row(g.logits, dt, R.SLACK_LOGIT[dt])
        self.ring = dev_ring(g.ring, dt) if g.ring is not None else None
        self.noise_rows = g.ring.shape[0] if g.ring is not None else 0
        self.seen = dev_seen(g.seen) if g.seen is not None else None
        p, st = g.policy, DecodeState()
        st.token, st.frame, st.pos, st.gen_step, st.done, st.text_open = -7, g.frame, 11 + g.frame, 5 + g.frame, g.done, 0
        st.min_new, st.max_new, st.trailing_len, st.noise_frames, st.eos_id, st.max_seq = g.min_new, 1000, 7, g.noise_frames, g.eos_id, 999
        st.sup_lo, st.sup_hi, st.n_pad, st.rope_delta = g.sup_lo, g.sup_hi, 3, -3
        if g.role == "talker":
            st.t_temperature, st.t_top_k, st.t_top_p, st.t_do_sample, st.t_rep_penalty = p.temperature, p.top_k, p.top_p, int(p.do_sample), p.rep_penalty
            st.p_temperature, st.p_top_k, st.p_top_p, st.p_do_sample = 0.5, 1, 0.25, 1          # the other role's policy must not be used
            st.talker_noise = ptr(self.ring)
        else:
            st.p_temperature, st.p_top_k, st.p_top_p, st.p_do_sample = p.temperature, p.top_k, p.top_p, int(p.do_sample)
            st.t_temperature, st.t_top_k, st.t_top_p, st.t_do_sample, st.t_rep_penalty = 0.5, 1, 0.25, 1, 1.7
            st.pred_noise = ptr(self.ring)
        self.st0, self.st = st, upload(st)
        self.codes_len = self.tf_len = (max(R.FRAMES) + 2) * g.G + 1          # (one length for every lane of a batch)
        self.codes = sent32(self.codes_len) if "codes" in outs and g.role == "pred" else None
        self.out64 = sent64(g.G) if "out64" in outs and g.role == "pred" else None
        self.emb = dev_emb(dt, g.V, g.H) if "emb" in outs and g.role == "pred" else None
        self.next_in = None
        self.forced = self.decisions = self.tf = None
        if g.tf != "none":
            self.decisions = sent32(self.tf_len)
            self.forced = torch.full((self.tf_len,), g.forced_id, dtype=torch.int32, device="cuda") if g.tf == "forced" else None
            self.tf = upload(TeacherForcing(ptr(self.forced), ptr(self.decisions)))

    def verify(self, kind, v, what, next_in=None):
        g, G = self.g, self.g.G
        now = bytes(self.st.cpu().numpy())
        codes = self.codes.cpu().numpy() if self.codes is not None else None
        out64 = self.out64.cpu().numpy() if self.out64 is not None else None
        dec = self.decisions.cpu().numpy() if self.decisions is not None else None
        if g.done:
            assert now == bytes(self.st0), f"{what}: done = {g.done}, the state changed"
            for a, s in ((codes, SENT32), (out64, SENT64), (dec, SENT32)):
                assert a is None or (a == s).all(), f"{what}: done = {g.done}, an output changed"
            if next_in is not None:
                assert (bits(next_in).cpu().numpy() == bits(sent_t(1, g.dt)).cpu().numpy()[0]).all(), f"{what}: done = {g.done}, next_in changed"
            return
        slot = g.slot
        if dec is not None:
            tok = int(dec[slot])
            assert (np.delete(dec, slot) == SENT32).all(), f"{what}: a decisions slot other than {slot} changed"
        elif g.role == "talker":
            tok = DecodeState.from_buffer_copy(now).token
        elif codes is not None:
            tok = int(codes[slot])
        elif out64 is not None:
            tok = int(out64[g.cb])
        else:
            tok = None
        final = tok
        if tok is not None:
            score(kind, g.name, v, tok, what)
            final = g.forced_id if g.tf == "forced" else tok
        if g.role == "talker":
            want = DecodeState.from_buffer_copy(bytes(self.st0))
            want.token, want.frame, want.pos, want.gen_step = final, g.frame + 1, want.pos + 1, want.gen_step + 1
            assert now == bytes(want), f"{what}: the state is not (token, frame + 1, pos + 1, gen_step + 1, nothing else changed)"
            return
        assert now == bytes(self.st0), f"{what}: the predictor sampler changed the state"
        if codes is not None:
            assert codes[slot] == final and (np.delete(codes, slot) == SENT32).all(), f"{what}: codes[{slot}] = {codes[slot]}, want {final} alone"
        if out64 is not None:
            assert out64[g.cb] == final and (np.delete(out64, g.cb) == SENT64).all(), f"{what}: out64[{g.cb}] = {out64[g.cb]}, want {final} alone"
        if next_in is not None and self.emb is not None and final is not None:
            H = g.H
            got, tab = bits(next_in).cpu().numpy(), bits(self.emb[final * H:(final + 1) * H]).cpu().numpy()
            assert np.array_equal(got[:H], tab), f"{what}: next_in is not row {final} of the table"
            assert (got[H:] == bits(sent_t(1, g.dt)).cpu().numpy()[0]).all(), f"{what}: next_in written behind H"


def launch_single(probe, kind, lane: Lane, v, what, nc=0):
    g = lane.g
    p = SamplerProbeArgs()
    p.V, p.H, p.G, p.B, p.cb, p.nc = g.V, g.H, g.G, 1, g.cb, nc
    p.noise_rows, p.codes_len, p.tf_len = lane.noise_rows, lane.codes_len, lane.tf_len
    p.logits, p.seen, p.st, p.tf = ptr(lane.logits), ptr(lane.seen), ptr(lane.st), ptr(lane.tf)
    p.cfg = c_cfg(R.Cfg(0.5, 1, 0.25, False))                    # the immediate policy must not be used when a state is given
    next_in = None
    if g.role == "pred":
        p.codes, p.out64, p.next_emb = ptr(lane.codes), ptr(lane.out64), ptr(lane.emb)
        if lane.emb is not None:
            next_in = sent_t(g.H + 8, g.dt)
            p.next_in = ptr(next_in)
    run(probe, kind, g.dt, p, what)
    lane.verify(kind, v, what, next_in)


def launch_batch(probe, kind, lanes, vs, what):
    g0, B = lanes[0].g, len(lanes)
    dt, V, H = g0.dt, g0.V, g0.H
    pred = kind == K_PRED_BATCH
    stride = V + R.SLACK if pred else V                          # the predictor launcher's logit_stride may exceed V; the talker's rows are V apart
    rows = [l.logits[:stride] for l in lanes] + [lanes[-1].logits[V:]]
    logits = torch.cat(rows)
    p = SamplerProbeArgs()
    p.V, p.H, p.G, p.B, p.cb, p.logit_stride = V, H, g0.G, B, g0.cb, stride
    p.noise_rows = min(l.noise_rows for l in lanes if l.noise_rows) if any(l.noise_rows for l in lanes) else 0
    p.codes_len = p.tf_len = min(l.codes_len for l in lanes)
    p.logits = ptr(logits)
    arr = lambda f: (vp * B)(*[f(l) for l in lanes])
    keep = [arr(lambda l: ptr(l.st)), arr(lambda l: ptr(l.codes)), arr(lambda l: ptr(l.seen)), arr(lambda l: ptr(l.tf))]
    p.lane_st, p.lane_codes, p.lane_seen, p.lane_tf = keep
    next_in = None
    if pred:
        next_in = sent_t(B * H + 8, dt)
        p.next_emb, p.next_in = ptr(lanes[0].emb), ptr(next_in)
    run(probe, kind, dt, p, what)
    tail = bits(sent_t(1, dt))[0]
    for i, (l, v) in enumerate(zip(lanes, vs)):
        ni = None
        if pred:                                                  # lane i's row, followed by the sentinel tail for the check behind H
            ni = torch.cat([next_in[i * H:(i + 1) * H], next_in[B * H:]])
        l.verify(kind, v, f"{what} lane {i}: {l.g.name}", ni)
    if pred:                                                      # rows of lanes are H apart: nothing is written behind the last one
        assert (bits(next_in[B * H:]) == tail).all(), f"{what}: next_in written behind the last lane"


def graph_lists(role, dt):
    """(GraphCase, Verdict) of both lists for a role and a storage type: the stateless cases posed through a state, then the in-graph cases."""
    out = []
    cases, vs = R.verdicts("stateless")
    for c, v in zip(cases, vs):
        if c.dt == dt:
            g = to_graph(c, role)
            if g is not None:
                out.append((g, v))
    cases, vs = R.verdicts("graph")
    out += [(g, v) for g, v in zip(cases, vs) if g.dt == dt and g.role == role]
    return out


def lds_only(g):
    return g.policy.do_sample and R.f32(g.policy.top_p) < 1.0


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("kind", [K_API, K_API_WAVE])
def test_api_kinds(probe, kind, dt):
    cases, vs = R.verdicts("stateless")
    for c, v in zip(cases, vs):
        if c.dt != dt or (kind == K_API_WAVE and c.cfg.do_sample and R.f32(c.cfg.top_p) < 1.0):
            continue
        p = SamplerProbeArgs()
        p.V, p.cfg = c.V, c_cfg(c.cfg)
        p.logits = ptr(dev_row(c.logits, dt, R.SLACK_LOGIT[dt]))
        p.noise = ptr(dev_row(c.noise, dt, R.SLACK_NOISE)) if c.noise is not None else None
        hist = None
        if c.seen is not None:
            if kind == K_API:
                hist = torch.from_numpy(np.flatnonzero(c.seen).astype(np.int64)).cuda()
                p.history, p.n_hist = ptr(hist), hist.numel()
            else:
                p.seen = ptr(dev_seen(c.seen))
        for nc in ((0, 2) if kind == K_API_WAVE and c.V <= 2048 else (0,)):
            out = sent64(3)
            p.out, p.nc = ptr(out), nc
            what = f"{KIND_NAME[kind]} nc={nc}: {c.name}"
            run(probe, kind, dt, p, what)
            o = out.cpu().numpy()
            assert (o[1:] == SENT64).all(), f"{what}: written behind out[0]"
            score(kind, c.name, v, int(o[0]), what)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("kind", [K_PRED, K_PRED_WAVE])
def test_pred_kinds_without_a_state(probe, kind, dt):
    """st = null: the immediate policy and noise, frame 0; suppression comes from the immediate SampleCfg."""
    cases, vs = R.verdicts("stateless")
    G, cb, H = 2, 0, 8
    for i, (c, v) in enumerate(zip(cases, vs)):
        if c.dt != dt or c.seen is not None or (kind == K_PRED_WAVE and c.cfg.do_sample and R.f32(c.cfg.top_p) < 1.0):
            continue
        p = SamplerProbeArgs()
        p.V, p.H, p.G, p.cb, p.cfg = c.V, H, G, cb, c_cfg(c.cfg)
        p.logits = ptr(dev_row(c.logits, dt, R.SLACK_LOGIT[dt]))
        p.noise = ptr(dev_row(c.noise, dt, R.SLACK_NOISE)) if c.noise is not None else None
        codes, out64 = (sent32(5), None) if i % 2 else (None, sent64(2))           # each null in turn
        p.codes, p.codes_len, p.out64 = ptr(codes), 5, ptr(out64)
        what = f"{KIND_NAME[kind]} st=null: {c.name}"
        run(probe, kind, dt, p, what)
        if codes is not None:
            o = codes.cpu().numpy()
            tok = int(o[1 + cb])
            assert (np.delete(o, 1 + cb) == SENT32).all(), f"{what}: a codes slot other than {1 + cb} changed"
        else:
            o = out64.cpu().numpy()
            tok = int(o[cb])
            assert o[1] == SENT64, f"{what}: written behind out64[{cb}]"
        score(kind, c.name, v, tok, what)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("kind", [K_PRED, K_PRED_WAVE, K_TALKER, K_TALKER_WAVE])
def test_in_graph_kinds(probe, kind, dt):
    role = "pred" if kind in (K_PRED, K_PRED_WAVE) else "talker"
    variants = (("codes", "out64", "emb"), ("codes",), ("out64", "emb"))
    n = 0
    for g, v in graph_lists(role, dt):
        if kind in REG and lds_only(g):
            continue
        outs = variants[n % 3] if role == "pred" and g.tf == "none" and not g.done else variants[0]
        n += 1
        launch_single(probe, kind, Lane(g, outs), v, f"{KIND_NAME[kind]}: {g.name}")
        if kind in REG and g.V == 2048 and "frames" in g.name:     # the two-chunk instantiation on a one-chunk vocabulary
            launch_single(probe, kind, Lane(g), v, f"{KIND_NAME[kind]} nc=2: {g.name}", nc=2)
    assert n > 100


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("kind", [K_PRED_BATCH, K_TALKER_BATCH])
def test_batch_kinds(probe, kind, dt):
    """Lanes of one (V, G, H, cb) packed into launches of 1, 3, 17 and 128 lanes: greedy, top-k and nucleus policies, finished and held
    lanes among running ones, per-lane bitmaps, noise rings and forcing objects in one launch."""
    role = "pred" if kind == K_PRED_BATCH else "talker"
    groups = defaultdict(list)
    for g, v in graph_lists(role, dt):
        groups[(g.V, g.G, g.H, g.cb, g.noise_frames)].append((g, v))
    sizes_seen = set()
    for key, lst in groups.items():
        sizes = [1, 3, 17] + ([128] if key[0] in (2048, 3072) and len(lst) > 40 else [])
        at = 0
        while at < len(lst):
            B = sizes.pop(0) if sizes else min(17, len(lst) - at)
            chunk = [lst[(at + i) % len(lst)] for i in range(B)]          # (the last launch of a group wraps round to fill its lanes)
            at += B
            sizes_seen.add(B)
            launch_batch(probe, kind, [Lane(g, ("codes", "emb")) for g, _ in chunk], [v for _, v in chunk], f"{KIND_NAME[kind]} B={B} V={key[0]} G={key[1]}")
    assert {1, 3, 17, 128} <= sizes_seen


def test_probe_refuses_what_would_leave_the_buffers(probe):
    dt, V = "f32", 2048
    x = torch.zeros(V + R.SLACK, device="cuda")
    nz = torch.ones(V + R.SLACK, device="cuda")
    out = sent64(3)

    def api(**kw):
        p = SamplerProbeArgs()
        p.V, p.logits, p.noise, p.out, p.cfg = V, ptr(x), ptr(nz), ptr(out), c_cfg(R.Cfg(0.9, 5, 1.0, True))
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    bad = [(K_API_WAVE, api(V=0)), (K_API, api(V=R.MAX_VOCAB + 8)), (K_API_WAVE, api(V=12)), (K_API, api(V=-8)), (K_API, api(logits=None)),
           (K_API_WAVE, api(out=None)), (K_API, api(noise=None)), (K_API_WAVE, api(noise=None)), (K_API_WAVE, api(V=3072, nc=1)),
           (K_API, api(n_hist=4)), (K_API, api(nc=1)), (K_API_WAVE, api(logits=ptr(x) + 4))]
    g = R.GraphCase("refusal", dt, V, "talker", np.zeros(V), 2, policy=R.Cfg(0.9, 5, 1.0, True), ring=np.ones((3, V)), noise_frames=3)
    lane = Lane(g)

    def graph(kind, ln, **kw):
        p = SamplerProbeArgs()
        p.V, p.H, p.G, p.B, p.noise_rows, p.codes_len, p.tf_len = V, 8, 2, 1, ln.noise_rows, ln.codes_len, ln.tf_len
        p.logits, p.st = ptr(ln.logits), ptr(ln.st)
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    bad += [(K_TALKER, graph(K_TALKER, lane, noise_rows=2)), (K_TALKER_WAVE, graph(K_TALKER_WAVE, lane, st=None)),
            (K_TALKER, graph(K_TALKER, lane, G=1))]
    no_noise = Lane(replace(g, ring=None))
    bad += [(K_TALKER, graph(K_TALKER, no_noise)), (K_TALKER_WAVE, graph(K_TALKER_WAVE, no_noise))]
    pl = Lane(replace(g, role="pred", ring=np.ones((3, V))))
    emb_ok = dict(codes=ptr(pl.codes), next_emb=ptr(pl.emb), next_in=ptr(sent_t(64, dt)))
    bad += [(K_PRED_WAVE, graph(K_PRED_WAVE, pl, H=12, **emb_ok)), (K_PRED, graph(K_PRED, pl, cb=1, **emb_ok)),
            (K_PRED, graph(K_PRED, pl, codes=ptr(pl.codes), codes_len=1)), (K_PRED_WAVE, graph(K_PRED_WAVE, pl, noise_rows=2, **emb_ok)),
            (K_PRED, graph(K_PRED, pl, next_emb=ptr(pl.emb)))]
    one = (vp * 1)(ptr(lane.st))
    many = (vp * (R.MAX_LANES + 1))(*[ptr(lane.st)] * (R.MAX_LANES + 1))
    bad += [(K_TALKER_BATCH, graph(K_TALKER_BATCH, lane, st=None, lane_st=one, B=0)),
            (K_TALKER_BATCH, graph(K_TALKER_BATCH, lane, st=None, lane_st=many, B=R.MAX_LANES + 1)),
            (K_TALKER_BATCH, graph(K_TALKER_BATCH, lane, st=None, B=1)),
            (K_PRED_BATCH, graph(K_PRED_BATCH, pl, st=None, lane_st=(vp * 1)(ptr(pl.st)), logit_stride=V - 8))]
    for i, (kind, p) in enumerate(bad):
        assert probe.sampler_probe_admits(kind, TE[dt], C.byref(p)) == 0, f"refusal {i} ({KIND_NAME[kind]}) was admitted"
        assert probe.sampler_probe_run(kind, TE[dt], C.byref(p), None) == REFUSED, f"refusal {i} ({KIND_NAME[kind]}) was launched"
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT64).all() and (pl.codes.cpu().numpy() == SENT32).all()
    assert bytes(lane.st.cpu().numpy()) == bytes(lane.st0) and bytes(pl.st.cpu().numpy()) == bytes(pl.st0)
    ok = graph(K_TALKER, lane)
    assert probe.sampler_probe_admits(K_TALKER, TE[dt], C.byref(ok)) == 1


@pytest.mark.parametrize("dt", R.DTS)
def test_fq3_sample_with_a_history(dt):
    """fq3_sample with a history (build_seen_kernel: repeated and out-of-range ids) and fq3_apply_repetition_penalty with the same
    history against the reference; the penalised vector element for element."""
    from fq3hip.engine import Fq3Engine
    from fq3hip.sampling import apply_repetition_penalty
    eng = Fq3Engine.sampler_only(torch.device("cuda", torch.cuda.current_device()), TDT[dt])
    cases, vs = R.verdicts("stateless")
    n = 0
    for c, v in zip(cases, vs):
        if c.dt != dt or c.seen is None:
            continue
        ids = np.flatnonzero(c.seen)
        hist = torch.from_numpy(np.concatenate([[-1, c.V, c.V + 100], ids, ids[::2], [-5, 1 << 20, c.V]]).astype(np.int64)).cuda()
        x = store(c.logits, dt)
        nz = store(c.noise, dt) if c.noise is not None else None
        tok = int(eng.sample(x, temperature=c.cfg.temperature, top_k=c.cfg.top_k, top_p=c.cfg.top_p, do_sample=c.cfg.do_sample,
                             repetition_penalty=c.cfg.rep_penalty, history=hist, noise=nz))
        msg = R.check(v, tok, f"fq3_sample: {c.name}")
        assert msg == "", msg
        pen = apply_repetition_penalty(x.clone(), hist, c.cfg.rep_penalty)
        want = store(R.penalised(c), dt)
        assert torch.equal(bits(pen), bits(want)), f"fq3_apply_repetition_penalty: {c.name}"
        n += 1
    STATS["fq3_sample + history"]["cases"] += n
    STATS["fq3_sample + history"]["decided"] += n
    assert n >= 13 * len(R.VS)


def test_zz_record(probe):
    """Prints the per-family record; every instantiation the probe builds was launched."""
    print()
    print(f"  {'kernel':<30}{'cases':>8}{'launches':>10}{'decided share':>16}")
    for name in list(KIND_NAME) + ["fq3_sample + history"]:
        st = STATS[name]
        if st["cases"]:
            print(f"  {name:<30}{st['cases']:>8}{st['launches']:>10}{st['decided'] / st['cases']:>16.4f}")
            assert 1.0 - st["decided"] / st["cases"] <= R.UNDECIDED_CAP, name
    want = {(k * 2 + t) * 3 + nc for k in range(8) for t in (0, 1) for nc in ((1, 2) if k in REG else (0,))}
    if all(STATS[name]["cases"] for name in KIND_NAME):              # (the whole module ran)
        assert REACHED == want, f"instantiations never launched: {sorted(want - REACHED)}"
        print(f"  instantiations launched: {len(REACHED)} of {len(want)}")
