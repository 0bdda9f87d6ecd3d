"""CPU: the model of tests/_state_ref.py against itself, against a second formulation, and against its mutants -- on the case list the
GPU test runs (imported from it, not copied).

* The model passes its own judge on every case, and what it leaves outside the ranges it names is the sentinel it found there.
* A second formulation agrees: torch F.embedding / sum / cat for embed_sum, text_gather and prompt_rows -- the sums in float64, to which
  the float32 model is held by the checker of tests/_gemm_ref.py with TOL unchanged, everything that is a copy by bits --; the prompt
  builder's tensor-op stand-in of tests/test_prompt_builder_cpu.py (the oracle's prompt builder runs over it there) on the rows it
  defines; a direct Python loop of the reference decode loop's frame logic (generate.py) for the trajectories: with the text that was
  published in the end given up front, it produces the same codes, predictor inputs and talker inputs frame by frame.
* Every listed mutant of the model is rejected by at least one case.
"""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as G
import _rows_ref as RR
import _state_ref as R
from test_gpu_state_reference import CASES
from test_prompt_builder_cpu import _FakeEngine

F64 = torch.float64


def launches(case):
    return [s for s in case.steps if isinstance(s, R.Launch)]


def test_the_case_list_covers_what_the_issue_names():
    names = [c.name for c in CASES]
    for dt in R.DTS:
        for H in (1, 8, 257, 264, 1024, 2048, 2056):
            assert any(n.startswith(f"frame_begin {dt} H {H} ") for n in names)
        for H in (8, 264, 1024, 2048, 2056):
            assert any(n.startswith(f"embed_sum {dt} H {H} ") for n in names) and f"text_gather {dt} Ht {H}" in names
            assert f"prompt_rows {dt} H {H} n_text {R.N_TEXT} n_ref {R.N_REF}" in names
        for B in (1, 3, 128):
            assert any(n.startswith(f"frame_begin_batch {dt} H 264 G 16 B {B} ") for n in names)
            assert any(n.startswith(f"embed_sum_batch {dt} H 264 B {B} ") for n in names)
        for K in (1, 255, 256, 257, 1024, 2048):
            assert sum(n.startswith(f"rmsnorm {dt} K {K} ") for n in names) == 4
        for L in (1, 63, 64, 65, 130):
            for n_kv in (1, 2):
                assert f"kv_import {dt} L {L} n_kv {n_kv}" in names and f"kv_export {dt} L {L} n_kv {n_kv}" in names
            assert any(n.startswith(f"kv_adopt {dt} L {L} layers 2") for n in names)
        assert f"kv_adopt {dt} L 65 layers 64" in names
    kinds = {s.kind for c in CASES for s in launches(c)} | {"rmsnorm"}
    assert kinds == set(R.KINDS)
    # every outcome of frame_begin, in the single and in the batch form
    for kind in ("frame_begin", "frame_begin_batch"):
        seen = set()
        for c in CASES:
            if c.lanes is None and any(s.kind == kind for s in launches(c)):
                mem = c.mem.clone()
                for s in launches(c):
                    got = R.apply(mem, s)
                    seen |= set(got if isinstance(got, list) else [got])
        assert seen == {"finished", "ends", "enters a hold", "stays held", "leaves a hold", "runs"}, (kind, seen)


def test_the_model_passes_its_own_judge():
    for case in CASES:
        if case.pb is not None:
            res = RR.judge(case.pb, RR.as_got(case.pb))
            assert all(r.ok for r in res), [r.msg for r in res if not r.ok]
            continue
        a, b = R.run_model(case), R.run_model(case)
        assert len(a) == len(launches(case)) > 0
        for L, ma, mb in zip(launches(case), a, b):
            assert R.judge(ma, mb, f"{case.name}: {L.kind} {L.note}") == []
        # a float buffer the case fills with the sentinel alone holds, in the end, values or the sentinel: a NaN of another payload
        # would be arithmetic on an element that must not be read
        for name, buf in a[-1].bufs.items():
            if buf.is_floating_point() and name not in ("src", "cache", "dense", "dst"):
                nan = torch.isnan(buf.to(torch.float32))
                sent = R.bits(buf) == R.bits(R.sent(1, "bf16" if buf.dtype == torch.bfloat16 else "f32"))
                assert bool((nan == sent).all()), f"{case.name}: the model computed on the sentinel in {name}"


def rows2d(mem, ref, rows, ld):
    """[GUARD + rows + GUARD][ld] view of the table whose row 0 is at ref"""
    name, off = ref
    return mem.bufs[name][off - R.GUARD * ld:off + (rows + R.GUARD) * ld].view(rows + 2 * R.GUARD, ld)


def check_sum(x_model, rows, text, dt, what):
    """x_model (storage type) against rnd(rnd(sum64 rows) + text) under the checker of _gemm_ref (K = 17 terms)"""
    r64 = rows.to(F64)
    s64 = r64.sum(0)
    inner = G.rnd(s64, dt)
    t64 = text.to(F64) if text is not None else torch.zeros_like(s64)
    ref = G.rnd(inner + t64, dt) if text is not None else inner
    S = r64.abs().sum(0) + t64.abs()
    extra = G.ulp(inner, dt) if (dt != "f32" and text is not None) else None
    v = G.check(x_model.to(F64).view(1, 1, -1), ref.view(1, 1, -1), S.view(1, 1, -1), dt, 17, what=what,
                extra=None if extra is None else extra.view(1, 1, -1))
    assert v.ok, v.msg


def test_embed_sum_agrees_with_embedding_sum_cat_in_float64():
    n = 0
    for case in CASES:
        if case.lanes is not None or not case.name.startswith("embed_sum"):
            continue
        out = R.run_model(case)
        mem = case.mem
        for L, after in zip(launches(case), out):
            batch = L.kind == "embed_sum_batch"
            H = L.n[0]
            B = L.n[6] if batch else 1
            tabs = L.tab[2] if batch else L.tab[0]
            for l in range(B):
                st = mem.states[(L.tab[0][l] if batch else L.p[0])[0][1:]]
                x = R.sl(after, ((L.p[0][0], L.p[0][1] + l * H) if batch else L.p[5]), H)
                rn = R.sl(after, ((L.p[3][0], L.p[3][1] + l * R.HEAD_DIM) if batch else L.p[4]), R.HEAD_DIM)
                if st["done"] != 0 or st["pos"] >= st["max_seq"] - 1:
                    assert bool(torch.isnan(x).all()) and bool(torch.isnan(rn).all()), f"{case.name} lane {l}: x or rope_now written"
                    continue
                codes = L.tab[1][l] if batch else L.p[1]
                ids = R.sl(mem, codes, (st["frame"] + 1) * 16)[st["frame"] * 16:].long()
                rows = torch.stack([F.embedding(ids[j] + R.GUARD, rows2d(mem, tabs[j], R.V0 if j == 0 else R.V1, H)) for j in range(16)])
                tt, tl = st["trailing_text"], st["trailing_len"]
                text = R.sl(mem, (tt[0], tt[1] + st["gen_step"] * H), H) if st["gen_step"] < tl else R.sl(mem, st["tts_pad"], H)
                check_sum(x, rows, text, L.dt, f"{case.name} lane {l}")
                delta = L.n[2] if not batch else st["rope_delta"]
                rp = torch.tensor(st["pos"] + delta).clamp(0, L.n[1] - 1) + R.GUARD
                cs = torch.cat([F.embedding(rp, rows2d(mem, L.p[1 if batch else 2], L.n[1], 64)), F.embedding(rp, rows2d(mem, L.p[2 if batch else 3], L.n[1], 64))])
                assert torch.equal(R.bits(rn), R.bits(cs)), f"{case.name} lane {l}: rope_now"
                n += 1
    assert n > 200


def test_text_gather_and_prompt_rows_agree_with_tensor_ops():
    for case in CASES:
        if case.name.startswith("text_gather"):
            (L,) = launches(case)
            (after,) = R.run_model(case)
            cnt, Ht, vocab = L.n[:3]
            ids = R.sl(case.mem, L.p[0], cnt).clamp(0, vocab - 1)
            want = F.embedding(ids + R.GUARD, rows2d(case.mem, L.p[1], vocab, Ht))
            assert torch.equal(R.bits(R.sl(after, L.p[2], cnt * Ht)), R.bits(want.reshape(-1))), case.name
        if not case.name.startswith("prompt_rows"):
            continue
        (L,) = launches(case)
        (after,) = R.run_model(case)
        mem, dt = case.mem, L.dt
        n_text, n_rows, n_ref, V0, V1, H = L.n[:6]
        tabs2d = [rows2d(mem, L.tab[0][j], V0 if j == 0 else V1, H) for j in range(16)]
        prog = R.sl(mem, L.p[1], 3 * n_rows).view(n_rows, 3)
        text = rows2d(mem, L.p[0], R.N_TEXT, H)[R.GUARD:]
        spk = R.sl(mem, L.p[3], H)
        ref = R.sl(mem, L.p[2], R.N_REF * 16).view(R.N_REF, 16)
        # the stand-in of test_prompt_builder_cpu.py (the oracle's prompt builder runs over it there) on the rows it defines: ids and
        # arguments in range, a text row or none
        eng = _FakeEngine.__new__(_FakeEngine)
        eng.tabs = [t[R.GUARD:] for t in tabs2d]
        for r, (trow, kind, arg) in enumerate(prog.tolist()):
            got = R.sl(after, (L.p[4][0], L.p[4][1] + r * H), H)
            has_text = 0 <= trow < n_text
            c = None
            if kind == 1:
                c = F.embedding(torch.tensor(arg).clamp(0, V0 - 1) + R.GUARD, tabs2d[0])
            elif kind == 2:
                c = spk
            elif kind == 3 and n_ref > 0:
                ids = torch.stack([ref[min(max(arg, 0), n_ref - 1), j].clamp(0, (V0 if j == 0 else V1) - 1) for j in range(16)])
                c = torch.stack([F.embedding(ids[j] + R.GUARD, tabs2d[j]) for j in range(16)])
            what = f"{case.name} row {r} ({trow}, {kind}, {arg})"
            if c is not None and c.dim() == 2:
                check_sum(got, c, text[trow] if has_text else None, dt, what)
            elif c is not None and has_text:
                check_sum(got, c[None], text[trow], dt, what)
            else:
                want = text[trow] if has_text else (c if c is not None else torch.zeros(H, dtype=R.TDT[dt]))
                assert torch.equal(R.bits(got), R.bits(want)), what
            in_range = (kind in (0, 2) or (kind == 1 and 0 <= arg < V0) or (kind == 3 and 0 <= arg < n_ref and bool(((ref[arg] >= 0) & (ref[arg] < V1)).all())))
            if in_range and kind in (0, 1, 2) and trow < n_text and (kind or trow >= 0) and dt == "f32":
                one = eng.prompt_rows(text, torch.tensor([[trow, kind, arg]]), ref_codes=ref, spk_embed=spk)[0]
                assert torch.equal(R.bits(got), R.bits(one)), what + ": the stand-in of the prompt builder test"


def reference_loop(d, dt, mem, tabs, final_rows, pos0, max_seq):
    """generate.py's decode loop for one lane, the text known up front: per frame the 16 codes, the predictor input and the talker
    input (None for the frame that meets the position limit); the tokens, codes and hidden states are the script's."""
    sc = d["sc"]
    H = R.TRAJ_H
    emb = [rows2d(mem, tabs[j], R.TRAJ_V if j == 0 else R.V1, H)[R.GUARD:] for j in range(16)]
    trailing = d["text_vals"][:final_rows]
    token, past_hidden, gen_step = d["first"], d["ph_vals"][0], 0
    frames = []
    for step_idx in range(min(sc["max_new"], R.TRAJ_STEPS)):
        if token == R.TRAJ_EOS:
            break
        last_id_hidden = emb[0][token]
        pred_input = torch.cat((past_hidden, last_id_hidden))
        cb = d["pcodes"][step_idx]
        hiddens = [last_id_hidden.float()] + [emb[j + 1][cb[j]].float() for j in range(15)]
        acc = hiddens[0]
        for h in hiddens[1:]:
            acc = acc + h
        inputs = acc.to(R.TDT[dt]).float()
        inputs = inputs + (trailing[gen_step] if gen_step < len(trailing) else d["pad_val"]).float()
        if pos0 + step_idx >= max_seq - 1:
            frames.append(([token] + cb, pred_input, None))
            break
        frames.append(([token] + cb, pred_input, inputs.to(R.TDT[dt])))
        token = sc["tokens"][step_idx]
        past_hidden = d["ph_vals"][step_idx + 1]
        gen_step += 1
    return frames


@pytest.mark.parametrize("dt", R.DTS)
def test_trajectories_agree_with_the_reference_decode_loop(dt):
    H = R.TRAJ_H
    want_frames = {"A": 5, "B": 4, "C": 3, "D": 1}
    for case in CASES:
        if case.lanes is None or f" {dt} single" not in case.name:
            continue
        out = R.run_model(case)
        ls = launches(case)
        for l, d in enumerate(case.lanes):
            st0 = case.mem.states[d["name"]]
            final_rows = max([e[2] for e in d["sc"]["events"] if e[1] == "publish"] + [d["sc"]["begin_rows"]])
            tabs = next(s for s in ls if s.kind == "embed_sum").tab[0]
            ref = reference_loop(d, dt, case.mem, tabs, final_rows, st0["pos"], st0["max_seq"])
            got = []
            for L, after in zip(ls, out):
                if L.p and L.p[0] == (d["st"], 0) and L.kind == "frame_begin" and after.states[d["name"]]["done"] == 0:
                    got.append([R.sl(after, L.p[3], 2 * H).clone(), None])
                if L.p and L.p[0] == (d["st"], 0) and L.kind == "embed_sum" and after.states[d["name"]]["done"] == 0:
                    got[-1][1] = R.sl(after, L.p[5], H).clone()
            end = out[-1].states[d["name"]]
            assert end["frame"] == len(got) == want_frames[d["name"]] and end["done"] == 1, (case.name, d["name"], end["frame"], len(got))
            assert len(ref) >= len(got) and (d["name"] == "D" or len(ref) == len(got)), (case.name, d["name"], len(ref), len(got))
            codes = R.sl(out[-1], d["codes"], len(got) * 16).view(len(got), 16).tolist()
            for f_, ((pi, x), (rc, rpi, rx)) in enumerate(zip(got, ref)):
                what = f"{case.name} lane {d['name']} frame {f_}"
                assert codes[f_] == rc, what
                assert torch.equal(R.bits(pi), R.bits(rpi)), what + ": predictor input"
                assert (x is None) == (rx is None) and (x is None or torch.equal(R.bits(x), R.bits(rx))), what + ": talker input"
    # what the scripts are there for: two holds entered and left, EOS, max_new, the position limit, a cancel while held
    case = next(c for c in CASES if c.name == f"trajectory A+B {dt} single")
    hist = [m.states["A"]["done"] for L, m in zip(launches(case), R.run_model(case)) if L.kind == "frame_begin" and L.p[0][0] == "$A"]
    assert [b for a, b in zip([0] + hist, hist) if a != b] == [2, 0, 2, 0, 1], hist


# mutant -> the kinds it touches (the cases without any of them are not run against it)
FB, ES = ("frame_begin", "frame_begin_batch"), ("embed_sum", "embed_sum_batch")
MUTANT_KINDS = {"no_hold_copy": FB, "ph_hold_ignored": FB, "frame_gt_max_new": FB, "pos_ge_max_seq": ES, "text_row_by_frame": ES,
                "rope_clamp_low": ES, "rope_clamp_high": ES, "lane_rope_delta_ignored": ("embed_sum_batch",), "pred_in_stride_h": ("frame_begin_batch",),
                "codes_slot_plus_1": FB, "trow_le_n_text": ("prompt_rows",), "kind3_not_rounded": ("prompt_rows",), "no_n_ref_guard": ("prompt_rows",),
                "scatter_first_item": ("text_scatter",), "poll_held_as_finished": ("poll_gather",),
                "block_and_row_swapped": ("kv_import", "kv_export"), "source_by_destination_table": ("kv_adopt",)}
_GOOD = {}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    """at least one case tells the model from the mutant (a mutant that leaves the case's buffers is told apart, too)"""
    caught = []
    for i, case in enumerate(CASES):
        if case.pb is not None or not any(s.kind in MUTANT_KINDS[mutant] for s in launches(case)):
            continue
        if i not in _GOOD:
            _GOOD[i] = R.run_model(case)
        try:
            bad = R.run_model(case, mutant)
        except AssertionError:
            caught.append(case.name)
            continue
        if any(R.judge(a, b) for a, b in zip(_GOOD[i], bad)):
            caught.append(case.name)
    assert caught, f"no case tells the model from its mutant {mutant}"
    if mutant in ("no_hold_copy", "ph_hold_ignored"):           # the trajectories are what these two are for
        assert any(n.startswith("trajectory") for n in caught), caught
