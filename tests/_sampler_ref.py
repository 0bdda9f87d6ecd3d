"""Float64 reference of the sampler kernels, the checker, and the case lists shared by tests/test_sampler_reference_cpu.py (no GPU)
and tests/test_gpu_sampler_reference.py.

The operation (fq3hip/sampling.py, oracle.sample_logits): repetition penalty by bitmap -> suppress window [sup_lo, sup_hi) except
keep_id, plus sup_extra -> greedy argmax (first index) | division by the temperature -> k-th value with ties kept (FLOAT comparison:
signed zeros are equal) -> optional nucleus (stable descending order = lowest index first among equals, running fp32 sum of the
T-rounded probabilities, cut rnd(cum) > rnd(top_p), first always kept) -> softmax -> argmax(rnd(rnd(p) / q)), first index on ties.
Plain NumPy in float64 with explicit roundings to the storage type T where the Torch ops round.

Everything up to and including the top-k filter is exact (one correctly rounded fp32 operation, then the rounding to T), so those
decisions are never excused.  Only exp, the sum and the two divisions can differ from the device by rounding: the checker carries a
relative uncertainty E = 2^-20 on the unrounded probabilities (<= 1 ulp of expf, <= 12 * 2^-24 from a tree sum of up to 4096 positive
terms, 1 ulp per division; all fp32).  A case is DECIDED when the nucleus cut is the same at p (1 - E), p and p (1 + E) and the
winner's lower bound beats every other candidate's upper bound (strictly for lower indices, >= for higher ones).  On a decided case
the device token must equal the reference token; on an undecided one it must be a token the reference produces at one of the three
scalings; undecided cases may be at most UNDECIDED_CAP of a family's list.

On top of the stateless core, the state semantics of the in-graph kernels (resolve): policy from DecodeState, the noise row
(frame % noise_frames) * (G - 1) + cb (predictor) / frame % noise_frames (talker), sup_extra = eos while frame + 1 < min_new, the
teacher-forcing slots frame * G + 1 + cb / (frame + 1) * G.

`mut` names a deliberately wrong variant (MUTANTS); the CPU test shows that the checker rejects each on a decided case of the list.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np

E = 2.0 ** -20
UNDECIDED_CAP = 0.05
MAX_VOCAB, MAX_LANES = 4096, 128
SLACK = 8                                    # elements behind V in every logits / noise row of the device image
DTS = ("bf16", "f32")
VS = (8, 256, 2040, 2048, 2056, 3072, 4088, 4096)
MUTANTS = ("tie_high", "topk_drop_ties", "topk_key", "sup_lo_off", "sup_hi_off", "no_keep", "min_new_le", "pen_div_neg",
           "noise_nomod", "noise_G", "no_mask_geV", "nuc_drop_first", "nuc_ge")
F32_MAX = float(np.finfo(np.float32).max)
SLACK_LOGIT = {"f32": F32_MAX, "bf16": float(np.float32(3.3895313892515355e38))}       # the largest finite value of T
SLACK_NOISE = 2.0 ** -126                                                                # the smallest positive normal of T


def f32(x) -> float:
    return float(np.float32(x))


def rnd(x, dt):
    """float64 -> the nearest value of the storage type, through fp32 (round to nearest even both times), as float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        x32 = np.atleast_1d(np.asarray(x, dtype=np.float64)).astype(np.float32)
    if dt == "f32":
        return x32.astype(np.float64)
    u = x32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(x32), np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def okey(x):
    """The order-preserving uint32 key of csrc/sampler.cuh BEFORE signed zeros were made equal (the `topk_key` mutant)."""
    u = np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


@dataclass
class Cfg:
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    do_sample: bool = False
    rep_penalty: float = 1.0
    sup_lo: int = 0
    sup_hi: int = 0
    keep_id: int = -1
    sup_extra: int = -1


@dataclass
class Case:
    """One stateless sampling problem.  logits / noise: float64 arrays of T values, [V]; seen: uint8 [V] or None."""
    name: str
    dt: str
    V: int
    logits: np.ndarray
    cfg: Cfg
    noise: Optional[np.ndarray] = None
    seen: Optional[np.ndarray] = None
    tags: tuple = ()


@dataclass
class Verdict:
    token: int
    decided: bool
    allowed: frozenset


def first_argmax(v, mut=None):
    v = np.where(np.isnan(v), -np.inf, v)
    m = v.max()
    idx = np.flatnonzero(v == m)
    return int(idx[-1] if mut == "tie_high" else idx[0])


def masked(c: Case, mut=None):
    """Stage 1: the penalised, suppressed row (exact)."""
    cfg, dt, V = c.cfg, c.dt, c.V
    x = c.logits.astype(np.float64).copy()
    pen = f32(cfg.rep_penalty)
    if c.seen is not None and pen != 1.0:
        s = c.seen != 0
        pos = np.ones(V, bool) if mut == "pen_div_neg" else x > 0
        x = np.where(s, np.where(pos, rnd(x / pen, dt), rnd(x * pen, dt)), x)
    ids = np.arange(V)
    lo = cfg.sup_lo + (1 if mut == "sup_lo_off" else 0)
    hi = cfg.sup_hi - (1 if mut == "sup_hi_off" else 0)
    keep = -1 if mut == "no_keep" else cfg.keep_id
    sup = ((ids >= lo) & (ids < hi) & (ids != keep)) | (ids == cfg.sup_extra)
    x[sup] = -np.inf
    return x


def penalised(c: Case):
    """apply_repetition_penalty alone: the row after the penalty, as T values."""
    return masked(replace(c, cfg=replace(c.cfg, sup_lo=0, sup_hi=0, keep_id=-1, sup_extra=-1)))


def filtered(c: Case, mut=None):
    """Stages 1-3 of a sampling case: masks, temperature, top-k with ties kept (exact)."""
    cfg, dt = c.cfg, c.dt
    x = masked(c, mut)
    q = c.noise.astype(np.float64)
    if mut == "no_mask_geV":
        x = np.concatenate([x, np.full(SLACK, SLACK_LOGIT[dt])])
        q = np.concatenate([q, np.full(SLACK, SLACK_NOISE)])
    with np.errstate(over="ignore"):
        x = rnd(x / f32(cfg.temperature), dt)
    n = x.shape[0]
    if cfg.top_k > 0:
        kk = min(cfg.top_k, n)
        if mut == "topk_key":
            key = okey(x)
            kth = np.sort(key)[::-1][kk - 1]
            x = np.where(key < kth, -np.inf, x)
        else:
            kth = np.sort(x)[::-1][kk - 1]
            if mut == "topk_drop_ties":                      # exactly k survive: the ties at the k-th value in index order
                above = x > kth
                ties = np.flatnonzero(x == kth)[:kk - int(above.sum())]
                keepm = above.copy()
                keepm[ties] = True
                x = np.where(keepm, x, -np.inf)
            else:
                x = np.where(x < kth, -np.inf, x)
    return x, q


def softmax64(x):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max())
        return e / e.sum()


def nucleus(x, cfg: Cfg, dt, scale, mut=None):
    """Stage 4 at probabilities scaled by `scale`: the row with the cut ids at -inf."""
    order = np.argsort(-x, kind="stable")                       # float comparison: equal values (signed zeros too) in index order
    p = rnd(softmax64(x)[order] * scale, dt)
    cum = rnd(np.cumsum(p.astype(np.float32), dtype=np.float32).astype(np.float64), dt)
    thr = float(rnd(f32(cfg.top_p), dt)[0])
    rm = cum >= thr if mut == "nuc_ge" else cum > thr
    if mut != "nuc_drop_first":
        rm[0] = False
    out = x.copy()
    out[order[rm]] = -np.inf
    return out


def race(x, q, dt, scale):
    """Stage 5 at probabilities scaled by `scale`: rnd(rnd(p) / q)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return rnd(rnd(softmax64(x) * scale, dt) / q, dt)


def sample(c: Case, mut=None) -> Verdict:
    """The reference token, whether the case is decided, and the tokens an undecided case may give."""
    cfg, dt = c.cfg, c.dt
    if not cfg.do_sample:
        x = masked(c, mut)
        if mut == "no_mask_geV":
            x = np.concatenate([x, np.full(SLACK, SLACK_LOGIT[dt])])
        t = first_argmax(x, mut)
        return Verdict(t, True, frozenset([t]))
    x, q = filtered(c, mut)
    toks, cuts, vals = [], [], []
    for s in (1.0, 1.0 - E, 1.0 + E):
        xs = nucleus(x, cfg, dt, s, mut) if f32(cfg.top_p) < 1.0 else x
        v = race(xs, q, dt, s)
        cuts.append(np.isneginf(xs))
        vals.append(v)
        toks.append(first_argmax(v, mut))
    w = toks[0]
    decided = bool((cuts[0] == cuts[1]).all() and (cuts[0] == cuts[2]).all())
    if decided:
        lo = np.where(np.isnan(vals[1]), -np.inf, vals[1])[w]
        hi = np.where(np.isnan(vals[2]), -np.inf, vals[2])
        decided = bool((hi[:w] < lo).all() and (hi[w + 1:] <= lo).all()) if mut != "tie_high" else \
            bool((hi[:w] <= lo).all() and (hi[w + 1:] < lo).all())
    return Verdict(w, decided, frozenset(toks))


def check(v: Verdict, tok: int, what: str) -> str:
    """'' when the device token `tok` satisfies the checker's rule for verdict v, else the message."""
    if v.decided:
        return "" if tok == v.token else f"{what}: token {tok}, the reference gives {v.token} (decided case)"
    return "" if tok in v.allowed else f"{what}: token {tok}, the reference gives one of {sorted(v.allowed)} (undecided case)"


# ---- the in-graph kernels ------------------------------------------------------------------------------------------------------------
@dataclass
class GraphCase:
    """One launch of a predictor / talker sampler inside the loop.  ring: float64 [rows][V] of T noise values shared by a group of
    cases (it holds MORE rows than noise_frames needs, all distinct, so that an index without the modulo stays inside the buffer and
    gives another token); state: the DecodeState fields that matter; tf: 'none' | 'dec' | 'forced'."""
    name: str
    dt: str
    V: int
    role: str                          # 'pred' | 'talker'
    logits: np.ndarray
    G: int
    cb: int = 0
    H: int = 8
    frame: int = 0
    noise_frames: int = 3
    min_new: int = 0
    done: int = 0
    eos_id: int = -1
    sup_lo: int = 0
    sup_hi: int = 0
    policy: Cfg = field(default_factory=Cfg)           # temperature, top_k, top_p, do_sample (talker: rep_penalty too)
    ring: Optional[np.ndarray] = None
    seen: Optional[np.ndarray] = None
    tf: str = "none"
    forced_id: int = 0
    tags: tuple = ()

    @property
    def slot(self):
        return self.frame * self.G + 1 + self.cb if self.role == "pred" else (self.frame + 1) * self.G


def noise_row(g: GraphCase, mut=None) -> int:
    f = g.frame if mut == "noise_nomod" else g.frame % g.noise_frames
    if g.role == "talker":
        return f
    return f * (g.G if mut == "noise_G" else g.G - 1) + g.cb


def resolve(g: GraphCase, mut=None) -> Case:
    """The stateless problem the kernel solves for this launch (done == 0)."""
    p = g.policy
    if g.role == "pred":
        cfg = Cfg(p.temperature, p.top_k, p.top_p, p.do_sample)
        seen = None
    else:
        before = g.frame + 1 <= g.min_new if mut == "min_new_le" else g.frame + 1 < g.min_new
        cfg = Cfg(p.temperature, p.top_k, p.top_p, p.do_sample, p.rep_penalty, g.sup_lo, g.sup_hi, g.eos_id, g.eos_id if before else -1)
        seen = g.seen
    noise = g.ring[noise_row(g, mut)] if p.do_sample else None
    return Case(g.name, g.dt, g.V, g.logits, cfg, noise, seen, g.tags)


def graph_sample(g: GraphCase, mut=None) -> Verdict:
    return sample(resolve(g, mut), mut)


# ---- case lists ------------------------------------------------------------------------------------------------------------------------
def _seed(name, dt, V, extra=0):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), DTS.index(dt), V, extra])


def row(rng, V, dt, scale=3.0):
    return rnd(rng.standard_normal(V) * scale, dt)


def exp_noise(rng, n, dt):
    return np.maximum(rnd(rng.exponential(1.0, n), dt), 2.0 ** -20)


def window(V):
    """The product's suppress window [V - 1024, V); the upper half for vocabularies that small that it would cover them whole."""
    return (V - 1024, V) if V > 1024 else (V // 2, V)


PLANT = (0, 7, 8, 511, 512, 2047, 2048)
TOP_PS = (0.99, 0.9, 0.5, 1e-6)


def stateless_cases():
    """The stateless list: every (storage type, V) of the issue with every policy, value and mask case."""
    out = []
    for dt in DTS:
        for V in VS:
            def add(name, x, cfg, noise=None, seen=None, tags=()):
                out.append(Case(f"{name} {dt} V={V}", dt, V, x, cfg, noise, seen, tuple(tags)))

            lo, hi = window(V)
            # greedy: the maximum planted at every boundary id, alone and tied with its lower neighbour across the boundary
            for j, pid in enumerate(sorted({p for p in PLANT if p < V} | {V - 1})):
                rng = _seed("greedy", dt, V, pid)
                x = row(rng, V, dt)
                x[pid] = float(x.max()) + 2.0
                add(f"greedy max@{pid}", x, Cfg())
                y = x.copy()
                other = pid - 1 if pid > 0 else 1
                y[other] = y[pid]
                add(f"greedy tie@{other},{pid}", y, Cfg(), tags=("tie",))
                # the same tie under sampling (lane, wave and chunk boundary): equal logits AND equal noise, the smallest of the row
                if pid not in (8, 512, 2048):
                    continue
                nz = exp_noise(rng, V, dt)
                nz[[other, pid]] = 2.0 ** -12
                add(f"sampled tie@{other},{pid}", y, Cfg(0.9, 50, 1.0, True), nz, tags=("tie",))
            # temperature x top_k
            for T in (0.7, 0.9, 1.3):
                for k in (0, 1, 5, 50, V, V + 7):
                    rng = _seed("policy", dt, V, int(T * 10) * 10000 + k)
                    add(f"T={T} k={k}", row(rng, V, dt), Cfg(T, k, 1.0, True), exp_noise(rng, V, dt))
            # the k-th value inside a tie group of 10 (ranks 3..12, k = 5), and the whole top-k inside one tie (ranks 1..10, k = 5);
            # the noise favours the LAST member of the group, which a filter that drops ties at the k-th value loses
            if V >= 256:
                for first, nm in ((2, "kth inside a tie of 10"), (0, "top-k inside one tie")):
                    rng = _seed(nm, dt, V)
                    x = row(rng, V, dt)
                    order = np.argsort(-x, kind="stable")
                    grp = np.sort(order[first:first + 10])
                    x[grp] = x[order[first + 10]] + 0.5
                    x[order[:first]] = x[grp[0]] + 0.5
                    nz = exp_noise(rng, V, dt)
                    nz[grp[-1]] = 2.0 ** -14
                    for p in (1.0, 0.9):
                        add(f"{nm} top_p={p}", x, Cfg(1.0, 5, p, True), nz, tags=("tie",))
            # signed zeros: k - 1 positive values, then zeros of both signs, everything else negative; the k-th value is a zero and the
            # noise favours a -0.0 entry (at a lower and at a higher index than the +0.0 entries)
            for which in ("low", "high"):
                rng = _seed("zeros" + which, dt, V)
                x = -np.abs(row(rng, V, dt)) - 1.0
                ids = np.sort(rng.choice(V, 8, replace=False)) if V > 8 else np.arange(8)
                pos_ids, zero_ids = ids[[1, 5]], ids[[0, 2, 3, 4, 6, 7]]
                x[pos_ids] = (1.0, 0.5)
                x[zero_ids] = (-0.0, 0.0, -0.0, 0.0, 0.0, -0.0)
                pick = zero_ids[0] if which == "low" else zero_ids[5]
                nz = exp_noise(rng, V, dt)
                nz[pick] = 2.0 ** -14
                for p in (1.0, 0.95):
                    add(f"signed zeros pick {which} top_p={p}", x, Cfg(0.9, 3, p, True), nz, tags=("zero",))
                add(f"signed zeros greedy {which}", np.where(x > 0, -1.0, x), Cfg(), tags=("zero",))
            # nucleus: peaked rows at every top_p, one flat (top_k = 0) row
            for p in TOP_PS:
                for k in ((50, 0) if p == 0.9 else (50,)):
                    rng = _seed("nucleus", dt, V, int(p * 1e6) + k)
                    add(f"top_p={p} k={k}", row(rng, V, dt), Cfg(0.9, k, p, True), exp_noise(rng, V, dt), tags=("nucleus",))
            # nucleus cut inside a tie group: one value above six equal ones at scattered ids; the cut falls after the second member, the
            # noise favours the third (cut) and then the second (kept)
            if V >= 256:
                rng = _seed("nucleus tie", dt, V)
                x = np.full(V, -30.0)
                ids = rng.choice(V, 7, replace=False)
                x[ids[0]] = 2.0
                grp = np.sort(ids[1:])
                x[grp] = 1.0
                nz = exp_noise(rng, V, dt)
                nz[grp[2]], nz[grp[1]] = 2.0 ** -14, 2.0 ** -10
                add("nucleus cut inside a tie", x, Cfg(1.0, 0, 0.6, True), nz, tags=("nucleus", "tie"))
            # cumulative sum EQUAL to top_p: four equal survivors of top_k = 4 (p = 0.25 each, exact), top_p = 0.5 keeps two
            rng = _seed("nucleus equal", dt, V)
            x = -np.abs(row(rng, V, dt)) - 1.0
            grp = np.sort(rng.choice(V, 4, replace=False))
            x[grp] = 1.0
            nz = exp_noise(rng, V, dt)
            nz[grp[1]] = 2.0 ** -14
            add("nucleus cum == top_p", x, Cfg(1.0, 4, 0.5, True), nz, tags=("nucleus", "tie"))
            # repetition penalty: sparse and dense bitmaps over negative, zero and positive logits
            for pen in (1.0, 1.05, 1.3):
                for dens, nm in ((0.02, "sparse"), (0.6, "dense")):
                    rng = _seed("penalty" + nm, dt, V, int(pen * 100))
                    x = row(rng, V, dt)
                    seen = (rng.random(V) < dens).astype(np.uint8)
                    x[rng.choice(V, max(1, V // 16), replace=False)] = 0.0
                    top = np.argsort(-x, kind="stable")[:3]
                    seen[top[0]] = 1
                    seen[int(np.argmin(x))] = 1
                    seen[int(np.flatnonzero(x == 0.0)[0])] = 1
                    add(f"penalty {pen} {nm} greedy", x, Cfg(rep_penalty=pen), seen=seen, tags=("seen",))
                    add(f"penalty {pen} {nm} sampled", x, Cfg(0.9, 50, 1.0, True, pen), exp_noise(rng, V, dt), seen, tags=("seen",))
            # a seen NEGATIVE maximum: multiplied it falls behind the runner-up, divided it would stay ahead
            rng = _seed("penalty negative", dt, V)
            x = -np.abs(row(rng, V, dt)) - 4.0
            a, b = (int(i) for i in rng.choice(V, 2, replace=False))
            x[a], x[b] = -1.0, -1.25
            seen = np.zeros(V, np.uint8)
            seen[a] = 1
            add("penalty on a negative maximum", x, Cfg(rep_penalty=1.3), seen=seen, tags=("seen",))
            # suppress window with keep_id inside it, at its edges and absent; the maximum sits at keep_id
            for keep in (lo, (lo + hi) // 2, hi - 1, -1):
                rng = _seed("suppress", dt, V, keep + 1)
                x = row(rng, V, dt)
                if keep >= 0:
                    x[keep] = float(x.max()) + 2.0
                add(f"suppress keep={keep} greedy", x, Cfg(sup_lo=lo, sup_hi=hi, keep_id=keep), tags=("sup",))
                add(f"suppress keep={keep} sampled", x, Cfg(0.9, 50, 1.0, True, 1.0, lo, hi, keep), exp_noise(rng, V, dt), tags=("sup",))
            # the maximum on either edge of the window (suppressed), keep_id elsewhere
            for at in (lo, hi - 1):
                rng = _seed("suppress edge", dt, V, at)
                x = row(rng, V, dt)
                x[at] = float(x.max()) + 2.0
                add(f"suppress max@{at}", x, Cfg(sup_lo=lo, sup_hi=hi, keep_id=(lo + hi) // 2), tags=("sup",))
            # sup_extra: the maximum sits there (alone, and as keep_id of the window: the talker's eos before min_new)
            rng = _seed("sup_extra", dt, V)
            x = row(rng, V, dt)
            ex = 3 if V > 8 else 1
            x[ex] = float(x.max()) + 2.0
            add("sup_extra greedy", x, Cfg(sup_extra=ex), tags=("sup",))
            add("sup_extra sampled", x, Cfg(0.9, 50, 1.0, True, sup_extra=ex), exp_noise(rng, V, dt), tags=("sup",))
            y = row(rng, V, dt)
            y[hi - 2] = float(y.max()) + 2.0
            add("sup_extra == keep_id", y, Cfg(sup_lo=lo, sup_hi=hi, keep_id=hi - 2, sup_extra=hi - 2), tags=("sup",))
            # all ids but one suppressed
            one = V // 3
            add("all but one suppressed greedy", row(rng, V, dt), Cfg(sup_lo=0, sup_hi=V, keep_id=one), tags=("sup",))
            add("all but one suppressed sampled", row(rng, V, dt), Cfg(0.9, 50, 1.0, True, 1.0, 0, V, one), exp_noise(rng, V, dt), tags=("sup",))
            # the whole top-k suppressed: the five largest values sit inside the window
            x = row(rng, V, dt)
            n5 = min(5, hi - lo)
            x[lo:lo + n5] = float(x.max()) + 1.0 + np.arange(n5)
            add("top-k suppressed", x, Cfg(0.9, 5, 1.0, True, 1.0, lo, hi, -1), exp_noise(rng, V, dt), tags=("sup",))
    return out


NOISE_FRAMES = 3
FRAMES = (0, 1, NOISE_FRAMES - 1, NOISE_FRAMES, 2 * NOISE_FRAMES + 3)
RING_FRAMES = 2 * NOISE_FRAMES + 4            # frames the ring buffers hold (the kernels may use the first NOISE_FRAMES)
GRAPH_SHAPES = ((8, 2, 2056), (256, 16, 2056), (2040, 2, 8), (2048, 16, 1024), (2056, 2, 8), (3072, 16, 1024), (4088, 2, 8), (4096, 2, 8))  # (V, G, H)

_RINGS = {}


def ring(dt, V, rows):
    key = (dt, V, rows)
    if key not in _RINGS:
        _RINGS[key] = exp_noise(_seed("ring", dt, V, rows), rows * V, dt).reshape(rows, V)
    return _RINGS[key]


def graph_cases():
    """The in-graph list: every frame / cb / min_new / done / teacher-forcing case, for both roles."""
    out = []
    sampled = Cfg(0.9, 50, 1.0, True)
    for dt in DTS:
        for V, G, H in GRAPH_SHAPES:
            lo, hi = window(V)
            eos = hi - 3
            pr, tr = ring(dt, V, RING_FRAMES * (G - 1)), ring(dt, V, RING_FRAMES)

            def pred(name, frame, cb, policy=sampled, seed=0, **kw):
                rng = _seed("gpred", dt, V, frame * 64 + cb * 4 + seed)
                out.append(GraphCase(f"pred {name} f={frame} cb={cb} {dt} V={V} G={G}", dt, V, "pred", row(rng, V, dt), G, cb, H, frame,
                                     NOISE_FRAMES, policy=policy, ring=pr, **kw))

            def talker(name, frame, policy=replace(sampled, rep_penalty=1.05), x=None, seed=0, **kw):
                rng = _seed("gtalk", dt, V, frame * 64 + seed)
                seen = (rng.random(V) < 0.05).astype(np.uint8)
                kw.setdefault("min_new", 2)
                out.append(GraphCase(f"talker {name} f={frame} {dt} V={V} G={G}", dt, V, "talker", row(rng, V, dt) if x is None else x, G, 0, H,
                                     frame, NOISE_FRAMES, eos_id=eos, sup_lo=lo, sup_hi=hi, policy=policy, ring=tr, seen=seen, **kw))

            for frame in FRAMES:
                for cb in sorted({0, G - 2}):
                    pred("frames", frame, cb)
                talker("frames", frame)
            # the min_new boundary: the maximum sits at eos; frame + 1 == min_new - 1 suppresses it, frame + 1 == min_new does not
            for policy, nm in ((Cfg(rep_penalty=1.05), "greedy"), (replace(sampled, rep_penalty=1.05), "sampled")):
                for mn in (6, 5):
                    rng = _seed("gminnew", dt, V, mn)
                    x = row(rng, V, dt)
                    x[eos] = float(x.max()) + 6.0
                    talker(f"min_new={mn} {nm}", 4, policy, x, min_new=mn)
            for done in (1, 2):
                pred(f"done={done}", 1, 0, done=done)
                talker(f"done={done}", 1, done=done)
            for tf in ("dec", "forced"):
                pred(f"tf={tf}", 2, G - 2, tf=tf, forced_id=V - 1, seed=1)
                talker(f"tf={tf}", 2, tf=tf, forced_id=V // 2, seed=1)
                pred(f"tf={tf} done", 2, 0, tf=tf, forced_id=1, done=1, seed=2)
            pred("greedy", 1, 0, Cfg(), seed=3)
            talker("greedy", 1, Cfg(rep_penalty=1.3), seed=3)
            for p in (0.9, 0.5):                                    # nucleus policies: the LDS kinds and the NUCLEUS bodies of the batch kinds
                pred(f"top_p={p}", 1, 0, replace(sampled, top_p=p), seed=4, tags=("nucleus",))
                talker(f"top_p={p}", 1, replace(sampled, top_p=p, rep_penalty=1.05), seed=4, tags=("nucleus",))
    return out


def family_of(c) -> str:
    if isinstance(c, GraphCase):
        return c.role
    return "stateless"


def undecided_share(verdicts) -> float:
    verdicts = list(verdicts)
    return sum(not v.decided for v in verdicts) / max(1, len(verdicts))


_CACHE = {}


def verdicts(which):
    """The reference verdicts of a case list, computed once per process: (cases, verdicts)."""
    if which not in _CACHE:
        cases = stateless_cases() if which == "stateless" else graph_cases()
        vs = [sample(c) if which == "stateless" else (graph_sample(c) if c.done == 0 else None) for c in cases]
        _CACHE[which] = (cases, vs)
    return _CACHE[which]
