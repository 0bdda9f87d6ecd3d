"""Self-test of tests/_rows_ref.py (no GPU): every reference agrees with a second float64 formulation of the operation, the judge
rejects every listed mutant of a reference on at least one case of the GPU test's own case list (imported, not copied), and the
conditions the GPU test relies on hold for the reference alone."""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as G
import _rows_ref as R
from _rows_ref import F64, GUARD
from oracle import qwen3tts_oracle as O


def put(pb, name, values):
    """The reference's device image with the written elements of output `name` replaced by `values` (a second formulation)."""
    got = R.as_got(pb)
    o = pb.outs[name]
    mask = ~torch.isnan(o.ref)
    full = torch.full_like(o.ref, R.NAN)
    v = values.reshape(-1)
    if v.numel() != int(mask.sum()):         # given with NaN where nothing is written
        v = v[~torch.isnan(v)]
    full[mask] = v
    got[name] = torch.where(mask, R.encode(full, pb.storage_fmt(name)), got[name])
    return got


def agrees(pb, name, values):
    """within the bound of the checker (the second formulation rounds once, at the end; the exact fraction is not asked of it)"""
    for r in R.judge(pb, put(pb, name, values), fraction=False):
        assert r.ok, r.msg


def inner(buf, off_rows, rows):
    return buf[off_rows:off_rows + rows]


@pytest.mark.parametrize("name", list(R.SUITE))
def test_reference_passes_its_own_judge(name):
    build, cases, dts = R.SUITE[name]
    pool = R.Pool()
    for dt in dts:
        for c in cases(dt):
            pb = build(c, dt)
            res = R.judge(pb, R.as_got(pb))
            pool.add(res)
            for r in res:
                assert r.ok, r.msg
    assert not pool.failures()


@pytest.mark.parametrize("dt", R.DTS)
def test_norms_second_formulation(dt):
    for c in R.norm_cases()[::7] + R.norm_cases(2)[:2]:
        C, n = c["C"], c["NS"] * c["rows"]
        pb = R.rmsnorm(c, dt, kind="rmsnorm_rows" if C < 1024 else "rmsnorm_vec2")
        x, w = inner(pb.bufs["x"], GUARD, n), pb.bufs["w"][:C]
        agrees(pb, "y", G.rnd(x * torch.rsqrt((x * x).mean(dim=1, keepdim=True) + R.EPS) * w, dt))
        live = ~torch.isnan(x[:, 0])
        y = torch.full_like(x, R.NAN)
        y[live] = O.rms_norm(x[live], w, R.EPS)              # the oracle's (fp32 inside)
        agrees(pb, "y", G.rnd(y, dt))
        if C < 1024:
            pl = R.layernorm(c, dt)
            x, w, b = inner(pl.bufs["x"], GUARD, n), pl.bufs["w"][:C], pl.bufs["b"][:C]
            agrees(pl, "y", G.rnd(F.layer_norm(x, (C,), w, b, R.EPS), dt))


@pytest.mark.parametrize("dt", R.DTS)
def test_convolutions_second_formulation(dt):
    for c in R.dwconv_cases()[::9]:
        C, rows, NS = c["C"], c["rows"], c["NS"]
        pb = R.dwconv7(c, dt)
        x = inner(pb.bufs["x"], GUARD, NS * rows).view(NS, rows, C).transpose(1, 2)
        w, b = pb.bufs["w"].view(C, 1, 7), pb.bufs["b"]
        y = F.conv1d(F.pad(x, (6, 0)), w, b, groups=C).transpose(1, 2)
        y2 = torch.stack([O.causal_conv1d(x[u], w, b, groups=C) for u in range(NS)]).transpose(1, 2)
        for alt in (y, y2):
            alt = alt.clone()
            alt[:, :c["row_lo"]] = R.NAN
            agrees(pb, "y", G.rnd(alt.reshape(NS * rows, C), dt)[~torch.isnan(alt.reshape(NS * rows, C))])
    for c in R.final_conv_cases(dt)[::5]:
        C, rows, NS, t_lo = c["C"], c["rows"], c["NS"], c["t_lo"]
        pb = R.final_conv(c, dt)
        x = inner(pb.bufs["x"], GUARD, NS * rows).view(NS, rows, C).transpose(1, 2)
        w = pb.bufs["w"].view(7, C).t().reshape(1, C, 7)
        y = F.conv1d(F.pad(x, (6, 0)), w, pb.bufs["b"][:1])[:, 0, t_lo:]
        agrees(pb, "pcm", G.rnd(y, dt).clamp(-1.0, 1.0))
    for c in R.conv_in_cases():
        n, C, K = c["n"], c["C"], c["K"]
        pb = R.conv_in(c)
        x = inner(pb.bufs["x"], GUARD, n).view(1, 1, n)
        y = F.conv1d(F.pad(x, (K - 1, 0)), pb.bufs["w"].view(C, 1, K), pb.bufs["b"])[0].t()
        agrees(pb, "y", y)
        agrees(pb, "e", F.elu(y))


def test_final_conv_f32_chain_model():
    """the float32 model of the stated chain lies within the float64 bound, and the clamp set clamps 10 % to 40 % of its samples"""
    for dt in R.DTS:
        clamped = total = 0
        for c in R.final_conv_cases(dt):
            pb = R.final_conv(c, dt)
            if c["C"] <= 128 and c["NS"] == 1 and c["seed"] % 4 == 0:
                agrees(pb, "pcm", R.final_conv_f32_chain(c, dt))
            if c["set"] == "clamp":
                o = pb.outs["pcm"]
                m = ~torch.isnan(o.ref)
                clamped += int((o.pre_clamp[m].abs() > 1.0).sum())
                total += int(m.sum())
        assert 0.10 <= clamped / total <= 0.40, (dt, clamped, total)


@pytest.mark.parametrize("dt", R.DTS)
def test_elementwise_second_formulation(dt):
    for c in R.silu_cases():
        pb = R.silu_mul(c, dt)
        gu = inner(pb.bufs["gu"], GUARD, c["rows"])
        agrees(pb, "y", G.rnd(F.silu(gu[:, :c["I"]]) * gu[:, c["I"]:], dt))
    for c in R.rope_cases()[::5]:
        hd, NH, rows, NS, lo = c["hd"], c["NH"], c["rows"], c["NS"], c["row_lo"]
        pb = R.rope(c, dt)
        qkv = inner(pb.bufs["qkv"], GUARD, NS * rows).view(NS, rows, 3, NH, hd)
        alt = torch.full_like(qkv, R.NAN)
        for u in range(NS):
            pos = c["base"][u] + torch.arange(rows - lo)
            cs, sn = (torch.cat([t[pos], t[pos]], dim=1) for t in (pb.bufs["cos"], pb.bufs["sin"]))
            for th in (0, 1):
                alt[u, lo:, th] = O.apply_rope(qkv[u, lo:, th], cs, sn)          # the oracle's rotate_half form
        alt = G.rnd(alt, dt).reshape(NS * rows, -1)
        agrees(pb, "qkv", alt[~torch.isnan(alt)])
    for c in R.snake_cases():
        pb = R.snake_consts(c, dt)
        C = c["C"]
        agrees(pb, "a", G.rnd(torch.exp(pb.bufs["alpha"][:C]), dt))
        if dt != "bf16":        # (in bf16 the 1e-9 vanishes behind exp(beta) except where it decides: the chain's roundings matter)
            agrees(pb, "ib", G.rnd(1.0 / (torch.exp(pb.bufs["beta"][:C]) + R.F32_1E9), dt))
    for c in R.rvq_gather_cases():
        if c["nq"] > 2:
            continue
        pb = R.rvq_gather(c, dt)        # at most one addition per half: the rounded float64 sum
        codes = pb.bufs["codes"].view(c["NS"], c["Tn"], c["nq"])
        books = [inner(pb.bufs[f"book{j}"], GUARD, R.BOOK_ROWS) for j in range(c["nq"])]
        for name, js in (("first", range(0, c["n_first"])), ("rest", range(c["n_first"], c["nq"]))):
            alt = torch.zeros(c["NS"], c["Tn"], c["dim"], dtype=F64)
            for j in js:
                alt += books[j][codes[:, :, j]]
            alt = G.rnd(alt, dt)[:, c["row_lo"]:]
            got = put(pb, name, alt)
            assert all(r.ok for r in R.judge(pb, got)), (c, name)


def test_analysers_second_formulation():
    for c in R.pad_cases():
        T, pl, ro = c["T"], c["pad_l"], c["rows_out"]
        if c["mode"] == 0 and max(pl, ro - T - pl) >= T:
            continue                    # torch's reflect needs pad < T; the clamped case is the kernel comment's own rule
        pb = R.pad_rows(c)
        s = inner(pb.bufs["src1"], GUARD, T)[:, :5]
        if c["two"]:
            s = G.rnd(s + inner(pb.bufs["src2"], GUARD, T)[:, :5], "f32")
        alt = F.pad(s.t()[None], (pl, ro - T - pl), mode="reflect" if c["mode"] == 0 else "replicate")[0].t()
        got = put(pb, "dst", alt)
        assert all(r.ok for r in R.judge(pb, got)), c
    for c in R.codebook_cases():
        pb = R.codebook_prepare(c)
        es = inner(pb.bufs["es"], GUARD, c["K"]).to(torch.float32)
        us = pb.bufs["usage"][:c["K"]].to(torch.float32)
        alt = (es / us.clamp_min(R.CB_EPS)[:, None]).to(F64)            # IEEE fp32 division
        assert torch.equal(alt, inner(pb.outs["emb"].ref, GUARD, c["K"]))
        assert torch.equal(alt.t(), inner(pb.outs["embT"].ref, GUARD, c["D"]))
    for c in R.dft_cases():
        pb = R.dft_mag(c)
        sp = inner(pb.bufs["spec"], GUARD, c["F"])
        agrees(pb, "mag", torch.sqrt(torch.hypot(sp[:, :c["NB"]], sp[:, c["NB"]:]) ** 2 + R.F32_1E9))
    for c in R.col_stats_cases():
        pb = R.col_stats(c)
        T, C = c["T"], c["C"]
        x = inner(pb.bufs["x"], GUARD, T)[:, :C]
        e = torch.exp(inner(pb.bufs["lg"], GUARD, T)[:, :C]) if c["logits"] else torch.ones(T, C, dtype=F64)      # exp(80) fits float64
        mu = (e * x).sum(dim=0) / e.sum(dim=0)
        var = (e * x * x).sum(dim=0) / e.sum(dim=0) - mu * mu
        if "mean" in pb.outs:
            agrees(pb, "mean", mu)
        if "std" in pb.outs:
            agrees(pb, "std", torch.sqrt(var.clamp_min(float(torch.tensor(c["eps"], dtype=torch.float32)))))
    for c in R.se_cases():
        pb = R.se_scale(c)
        T, C = c["T"], c["C"]
        alt = torch.addcmul(inner(pb.bufs["r"], GUARD, T)[:, :C], inner(pb.bufs["x"], GUARD, T)[:, :C], pb.bufs["gate"][:C])
        agrees(pb, "y", alt)


def test_rvq_encode_one_level_is_cdist_argmin():
    for c in R.encode_cases():
        if c["nq"] != 1 or c["set"] == "tie":
            continue
        proj, emb = R.encode_operands(c)
        codes, _ = R.encode_walk(c, proj, emb)
        want = torch.argmin(torch.cdist(proj[:, :c["D"]], emb[0]), dim=1)
        assert torch.equal(codes[:, 0], want), c


def test_rvq_encode_conditions():
    """The float32 ascending-d model of the scan stays within the 2 % near-tie cap on the random set and has none on the separated set;
    the separated set's float64 margin is far above the bound; the tie set's winner is a true tie at the lower index."""
    for c in R.encode_cases():
        pb = R.rvq_encode(c)
        r = R.judge_encode(pb, R.encode_f32_model(c))
        assert r.ok, r.msg
        if c["set"] == "separated":
            assert r.near == 0
            # the float64 margin of every decision: the runner-up lies at least 100 bounds behind the winner
            proj, emb = R.encode_operands(c)
            assert R.encode_min_margin(c, proj, emb) >= 100.0, c
        if c["set"] == "tie":
            i0, i1 = R.tie_pair(c["K"], c["tie"])
            assert i0 < i1 < c["K"]
            codes = pb.enc["codes_out"][GUARD * c["nq"]:].view(-1, c["nq"])
            assert int(codes[0, 0]) == i0 and int(codes[0, c["n_sem"]]) == i0, c


MUTANT_CASES = [(name, m) for name, ms in R.MUTANTS.items() for m in ms]


@pytest.mark.parametrize("name,mutant", MUTANT_CASES)
def test_mutant_is_rejected(name, mutant):
    """on at least one case of the GPU test's list, per storage type the mutant exists in"""
    build, cases, dts = R.SUITE[name]
    for dt in dts:
        if mutant in R.ROUNDING_MUTANTS and dt == "f32":
            continue
        pool = R.Pool()
        rejected = False
        for c in cases(dt):
            pb = build(c, dt)
            res = R.judge(pb, R.as_got(build(c, dt, mutant=mutant)))
            pool.add(res)
            if not all(r.ok for r in res):
                rejected = True
                break
        assert rejected or pool.failures(), f"{name} {dt}: the mutant {mutant} passes every case"
