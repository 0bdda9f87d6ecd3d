"""Conformance of the decode-loop state, prompt and KV glue kernels with the model of tests/_state_ref.py.

Each launch goes alone through tools/microbench/libstate_probe.so (built with the library's kernarg-preload option, so frame_begin_kernel
and embed_sum_kernel are the code objects the library ships).  A case is an initial memory image -- every buffer with guard rows in
front and behind, sentinel-filled outputs, sentinel rows wherever no id points, the lanes' buffers and states laid out in shuffled
order -- and a list of launches; after EVERY launch every buffer is compared by bits and the arena that holds the DecodeStates byte
for byte with the model's.  Nothing here has a tolerance: everything is bit-exact, except rmsnorm_kernel, which goes through the
rmsnorm reference and judge of tests/_rows_ref.py (bound + exact fraction, constants unchanged).

Never launched: a null ref_codes or a null spk.  The n_ref == 0 guard of prompt_rows_kernel is launched with ref_codes pointing inside a
guarded allocation whose guard holds out-of-range ids that clamp to sentinel rows, so a kernel without the guard gives NaN rows and no
fault; the null-spk guard is checked by reading only (csrc/prompt_kernels.cuh: `kind == 2 && spk`), and the probe refuses both null
combinations (test_probe_refuses_what_would_leave_the_buffers).

The trajectories run two lanes through frame_begin -> (codes 1..15 planted) -> embed_sum -> (a new past_hidden, as the stack leaves it,
held or not) -> sample_talker_kernel (greedy, V = 64, a planted maximum) with text_publish / decode_cancel in between, once with the
single-stream kernels and once with the batch kernels; after every step each lane's buffers and state are the same bits in both runs.

The last test prints the per-kernel record and asserts that every instantiation the probe builds was launched.
Observed on the MI355X (a record: nothing is tuned to it; "cases" counts the cases that launch the kernel, trajectories included):
  kernel                                      cases  launches
  frame_begin_kernel                             22       164
  frame_begin_batch_kernel                       12        48
  embed_sum_kernel                               16       120
  embed_sum_batch_kernel                         12        48
  rmsnorm_kernel                                 48        48   largest err / bound 0.026, exact fraction bf16 1.0000, f32 0.5702
  copy_kernel                                    12        12
  text_gather_kernel                             10        10
  prompt_rows_kernel                             16        16
  kv_paged_copy_kernel (to the cache)            20        20
  kv_paged_copy_kernel (from the cache)          20        20
  kv_adopt_kernel                                12        12
  sample_talker_kernel (greedy)                   8       160
  text_open_kernel                               14        18
  text_publish_kernel                             8        14
  poll_gather_kernel                              3         3
  text_scatter_kernel                            16        16
  text_publish_lanes_kernel                       8        14
  kv_table_write_kernel                           4         4
  decode_arm_kernel                               6         6
  decode_set_forced_kernel                        1         3
  decode_cancel_kernel                            7         7
  codes_to_i64_kernel                             6         6
  instantiations launched: 34 of 34 (twelve typed kinds in bf16 and fp32, ten kinds without a storage type).
  Every launch left every buffer and every state byte equal to the model's; the batch lanes equalled their single-stream runs.
One defect, found by reading and fixed with the cases that cover it: prompt_rows_kernel read ref_codes[-16 .. -1] for a row of kind 3
when n_ref == 0 (through the null pointer the host passes with n_ref = 0), and spk for a row of kind 2 with a null spk.  The cases
"prompt_rows * n_ref 0" launch the first combination on a guarded ref_codes and pass with the guard in the kernel.  A probe built once
from the kernel without the n_ref guard failed exactly these four cases (bf16 and fp32, H = 264 and 2056): the 16 rows of kind 3 came
out as NaN where the model has text only or zeros (4224 of 22176 and 32896 of 172704 elements), and nothing else differed.
"""
import ctypes as C
import os
import random
from collections import defaultdict

import pytest
import torch

import _rows_ref as RR
import _state_ref as R
from test_gpu_sampler_reference import DecodeState, TeacherForcing, layout_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "microbench", "libstate_probe.so")
REFUSED = 100000
vp = C.c_void_p


class LaneTab(C.Structure):
    _fields_ = [("st", vp * 128), ("codes", vp * 128), ("seen", vp * 128), ("past_hidden", vp * 128), ("ph_hold", vp * 128)]


class StateArgs(C.Structure):
    _fields_ = [("p", vp * 8), ("tab", (vp * 128) * 5), ("iv", C.c_int * 132), ("iv2", C.c_int * 128), ("n", C.c_long * 8), ("f", C.c_float * 2),
                ("host", vp)]


CASES = R.all_cases()              # (tests/test_state_reference_cpu.py imports this list)
GROUPS = defaultdict(list)
for _c in CASES:
    GROUPS[_c.name.split()[0]].append(_c)

STATS = defaultdict(lambda: {"cases": 0, "launches": 0, "ratio": 0.0})
REACHED = set()
POOL = RR.Pool()
SNAPSHOTS = {}                     # trajectory name -> per step, per lane, what the lane owns


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tools/microbench/libstate_probe.so missing: run __graft_entry__.build() (make tools)"
    lib = C.CDLL(PROBE)
    lib.state_probe_run.argtypes = [C.c_int, C.c_int, C.POINTER(StateArgs), vp]
    lib.state_probe_admits.argtypes = [C.c_int, C.c_int, C.POINTER(StateArgs)]
    lib.state_probe_layout.argtypes = [C.POINTER(C.c_long), C.c_int]
    lib.state_probe_insts.argtypes = [C.POINTER(C.c_int), C.c_int]
    assert lib.state_probe_version() == 1 and lib.state_probe_kinds() == len(R.KINDS) and lib.state_probe_refused_code() == REFUSED
    buf = (C.c_long * 128)()
    n = lib.state_probe_layout(buf, 128)
    want = layout_of(DecodeState) + layout_of(TeacherForcing) + layout_of(LaneTab) + layout_of(StateArgs)
    assert list(buf[:n - 4]) == want, "a ctypes mirror of DecodeState / TeacherForcing / LaneTab / StateArgs is out of date"
    assert list(buf[n - 4:n]) == [R.MAX_LANES, R.MAX_VOCAB, R.KEYS_PER_TILE, R.HEAD_DIM]
    assert [f[0] for f in DecodeState._fields_] == [f[0] for f in R.STATE_FIELDS], "the model's field list is not DecodeState's"
    return lib


# ---- one memory image on the device ------------------------------------------------------------------------------------------------
ST_SIZE, TF_SIZE = C.sizeof(DecodeState), C.sizeof(TeacherForcing)


class Device:
    """A Mem on the device: the buffers as they are, the states and the forcing objects in arenas whose slots are handed out in shuffled
    order with a sentinel slot between any two."""

    def __init__(self, mem: R.Mem, seed=0):
        self.bufs = {k: v.cuda() for k, v in mem.bufs.items()}
        rng = random.Random(seed)
        self.slot, self.tslot = {}, {}
        names = list(mem.states)
        order = list(range(len(names)))
        rng.shuffle(order)
        for nm, o in zip(names, order):
            self.slot[nm] = (2 * o + 1) * ST_SIZE
        for i, nm in enumerate(mem.tfs):
            self.tslot[nm] = (2 * i + 1) * TF_SIZE
        self.st_arena = torch.empty((2 * len(names) + 1) * ST_SIZE, dtype=torch.uint8, device="cuda")
        self.tf_arena = torch.empty((2 * len(mem.tfs) + 1) * TF_SIZE, dtype=torch.uint8, device="cuda")
        self.st_arena.copy_(self.arena_image(mem))
        self.tf_arena.copy_(self.tf_image(mem))

    def addr(self, ref):
        if ref is None:
            return None
        name, off = ref
        if name.startswith("$"):
            return self.st_arena.data_ptr() + self.slot[name[1:]]
        if name.startswith("&"):
            return self.tf_arena.data_ptr() + self.tslot[name[1:]]
        b = self.bufs[name]
        return b.data_ptr() + off * b.element_size()

    def c_state(self, st):
        s = DecodeState()
        for name, kind in R.STATE_FIELDS:
            setattr(s, name, self.addr(st[name]) if kind == "p" else st[name])
        return s

    def arena_image(self, mem):
        img = bytearray([R.SENT8]) * self.st_arena.numel()
        for nm, st in mem.states.items():
            img[self.slot[nm]:self.slot[nm] + ST_SIZE] = bytes(self.c_state(st))
        return torch.frombuffer(img, dtype=torch.uint8)

    def tf_image(self, mem):
        img = bytearray([R.SENT8]) * self.tf_arena.numel()
        for nm, tf in mem.tfs.items():
            img[self.tslot[nm]:self.tslot[nm] + TF_SIZE] = bytes(TeacherForcing(self.addr(tf["forced"]), self.addr(tf["decisions"])))
        return torch.frombuffer(img, dtype=torch.uint8)

    def args(self, L: R.Launch):
        a = StateArgs()
        for i, ref in enumerate(L.p):
            a.p[i] = self.addr(ref)
        for t, refs in L.tab.items():
            for i, ref in enumerate(refs):
                a.tab[t][i] = self.addr(ref)
        for i, v in enumerate(L.iv):
            a.iv[i] = v
        for i, v in enumerate(L.iv2):
            a.iv2[i] = v
        for i, v in enumerate(L.n):
            a.n[i] = v
        for i, v in enumerate(L.f):
            a.f[i] = v
        if L.host is not None:
            self.host = self.c_state(L.host)                  # (kept alive for the launch)
            a.host = C.addressof(self.host)
        return a

    def differences(self, want: R.Mem, what):
        bad = []
        got = R.Mem({k: v.cpu() for k, v in self.bufs.items()})
        for name, w in want.bufs.items():
            ne = R.bits(got.bufs[name]) != R.bits(w)
            if bool(ne.any()):
                i = int(torch.nonzero(ne)[0])
                bad.append(f"{what}: buffer {name}: {int(ne.sum())} of {w.numel()} elements differ, first at {i}: got {got.bufs[name][i].item()!r}, "
                           f"the model has {w[i].item()!r}")
        arena, img = self.st_arena.cpu(), self.arena_image(want)
        if not torch.equal(arena, img):
            raw = bytes(arena.numpy().tobytes())
            named = False
            for nm, st in want.states.items():
                g, w = DecodeState.from_buffer_copy(raw[self.slot[nm]:self.slot[nm] + ST_SIZE]), self.c_state(st)
                for f_, _k in R.STATE_FIELDS:
                    if getattr(g, f_) != getattr(w, f_):
                        bad.append(f"{what}: state {nm}.{f_} = {getattr(g, f_)!r}, the model has {getattr(w, f_)!r}")
                        named = True
            if not named:
                bad.append(f"{what}: a byte of the state arena outside the states' fields changed")
        if not torch.equal(self.tf_arena.cpu(), self.tf_image(want)):
            bad.append(f"{what}: a TeacherForcing object differs from the model's")
        return bad, got


def launch(probe, dev, L, what):
    a = dev.args(L)
    kind, te = R.KIND[L.kind], R.TE[L.dt]
    assert probe.state_probe_admits(kind, te, C.byref(a)) == 1, f"{what}: the probe refuses the launch"
    torch.cuda.synchronize()
    rc = probe.state_probe_run(kind, te, C.byref(a), None)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:           # a device fault: nothing more may run on this GPU in this session
        pytest.exit(f"{what}: {e}", returncode=3)
    if rc != 0:
        pytest.exit(f"{what}: the probe returned HIP error {rc}", returncode=3)
    REACHED.add(probe.state_probe_last_inst())
    STATS[R.KERNEL[L.kind]]["launches"] += 1


def run_case(probe, case, fails):
    """Every launch of the case; after each one the whole memory against the model."""
    dev = Device(case.mem, seed=len(case.name))
    model = case.mem.clone()
    kinds = set()
    for s in case.steps:
        if isinstance(s, R.Write):
            model.bufs[s.buf][s.off:s.off + s.data.numel()] = s.data
            dev.bufs[s.buf][s.off:s.off + s.data.numel()] = s.data.cuda()
            continue
        what = f"{case.name}: {s.kind} {s.note}"
        launch(probe, dev, s, what)
        R.apply(model, s)
        bad, got = dev.differences(model, what)
        fails += bad
        kinds.add(s.kind)
        if case.lanes and s.kind == "talker_step" and s.p[0][0] == case.lanes[-1]["st"]:
            snap = [R.lane_view(R.Mem(got.bufs, model.states), d) for d in case.lanes]
            snap.append({k: R.bits(got.bufs[k]).clone() for k in ("pred_in", "x", "rope_now")})
            SNAPSHOTS.setdefault(case.name, []).append(snap)
        if bad:
            break                       # (what follows would repeat the difference)
    for k in kinds:
        STATS[R.KERNEL[k]]["cases"] += 1


def to_device(b, fmt):
    if fmt == "bf16":
        return torch.where(b >= (1 << 15), b - (1 << 16), b).to(torch.int16).cuda()
    return torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32).cuda()


def run_rmsnorm(probe, case, fails):
    pb = case.pb
    init = {name: pb.initial_bits(name) for name in list(pb.bufs) + [n for n in pb.outs if n not in pb.bufs]}
    dev = {name: to_device(b, pb.dt) for name, b in init.items()}
    a = StateArgs()
    for i, (name, off) in enumerate(pb.p):
        a.p[i] = dev[name].data_ptr() + off * R.esz(pb.dt)
    a.n[0], a.f[0] = pb.K, pb.f[0]
    kind, te = R.KIND["rmsnorm"], R.TE[pb.dt]
    assert probe.state_probe_admits(kind, te, C.byref(a)) == 1, f"{case.name}: the probe refuses the launch"
    rc = probe.state_probe_run(kind, te, C.byref(a), None)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{case.name}: {e}", returncode=3)
    if rc != 0:
        pytest.exit(f"{case.name}: the probe returned HIP error {rc}", returncode=3)
    REACHED.add(probe.state_probe_last_inst())
    mask = 0xFFFF if pb.dt == "bf16" else 0xFFFFFFFF
    back = {name: dev[name].cpu().to(torch.int64) & mask for name in dev}
    for name in pb.bufs:
        if name not in pb.outs and not torch.equal(back[name], init[name]):
            fails.append(f"{case.name}: input {name} changed")
    results = RR.judge(pb, {name: back[name] for name in pb.outs})
    POOL.add(results)
    st = STATS[R.KERNEL["rmsnorm"]]
    st["cases"] += 1
    st["launches"] += 1
    for r in results:
        if not r.ok:
            fails.append(r.msg)
        st["ratio"] = max(st["ratio"], r.ratio)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_kernels(probe, group):
    fails = []
    for case in GROUPS[group]:
        if case.pb is not None:
            run_rmsnorm(probe, case, fails)
        else:
            run_case(probe, case, fails)
    if group == "rmsnorm":
        fails += POOL.failures()
    assert not fails, f"{len(fails)} differences:\n" + "\n".join(fails[:12])


def test_batch_lanes_equal_their_single_stream_runs(probe):
    """after every step each lane owns the same bits, and the shared pred_in / x / rope_now hold the same bits, whether the lanes ran
    one after the other through the single-stream kernels or in lock-step through the batch kernels"""
    if not SNAPSHOTS:                   # (this test alone: run the trajectories first)
        fails = []
        for case in GROUPS["trajectory"]:
            run_case(probe, case, fails)
        assert not fails, "\n".join(fails[:12])
    pairs = 0
    for name, snaps in SNAPSHOTS.items():
        if not name.endswith(" single"):
            continue
        other = SNAPSHOTS[name[:-len("single")] + "batch"]
        assert len(snaps) == len(other) == R.TRAJ_STEPS, name
        for step, (a, b) in enumerate(zip(snaps, other)):
            for la, lb in zip(a, b):
                for k in la:
                    same = la[k] == lb[k] if isinstance(la[k], dict) else torch.equal(la[k], lb[k])
                    assert same, f"{name} step {step}: {k} differs between the single-stream and the batch run"
        pairs += 1
    assert pairs == len(R.PAIRS) * len(R.DTS)


def first_launch(prefix, pick=lambda c: True):
    case = next(c for c in CASES if c.name.startswith(prefix) and pick(c))
    return case, next(s for s in case.steps if isinstance(s, R.Launch))


def test_probe_refuses_what_would_leave_the_buffers(probe):
    """each refusal: admits says 0, run returns the refused code, and no byte of the memory image has changed"""
    def refused(case, L, why, edit=None, st_edit=None, te=None):
        mem = case.mem.clone()
        if st_edit:
            for nm, kw in st_edit.items():
                mem.states[nm].update(kw)
        dev = Device(mem)
        a = dev.args(L)
        if edit:
            edit(a)
        kind = R.KIND[L.kind]
        t = R.TE[L.dt] if te is None else te
        assert probe.state_probe_admits(kind, t, C.byref(a)) == 0, why
        assert probe.state_probe_run(kind, t, C.byref(a), None) == REFUSED, why
        torch.cuda.synchronize()
        bad, _ = dev.differences(mem, why)
        assert not bad, bad

    def setn(i, v):
        return lambda a: a.n.__setitem__(i, v)

    def setp(i, v):
        return lambda a: a.p.__setitem__(i, v)

    case, L = first_launch("frame_begin f32 H 264")
    nm = L.p[0][0][1:]
    refused(case, L, "tok outside the seen / codec_emb rows", st_edit={nm: dict(token=R.V0, done=0, text_open=0)})
    refused(case, L, "negative tok", st_edit={nm: dict(token=-1, done=0, text_open=0)})
    refused(case, L, "frame >= frames allocated", st_edit={nm: dict(frame=L.n[3], max_new=L.n[3] + 2, done=0, text_open=0)})
    refused(case, L, "a storage type the probe does not have", te=1)
    case, L = first_launch("frame_begin_batch f32 H 264 G 16 B 3")
    refused(case, L, "a lane's tok outside the table", st_edit={"l0": dict(token=R.V0 + 3, done=0, text_open=0)})
    refused(case, L, "more than 128 lanes", setn(4, 129))
    for prefix, i in (("embed_sum f32 H 264", 0), ("embed_sum_batch f32 H 264 B 3", 0), ("text_gather f32 Ht 264", 1), ("prompt_rows f32 H 264 n_text 5 n_ref 4", 5)):
        case, L = first_launch(prefix)
        refused(case, L, f"{prefix}: H no multiple of 8", setn(i, 260))
    case, L = first_launch("embed_sum f32 H 264", )
    refused(case, L, "a code id outside its table", setn(4, 1))
    refused(case, L, "frame >= frames allocated", setn(5, 1))
    case, L = first_launch("embed_sum_batch f32 H 264 B 3")
    refused(case, L, "more than 128 lanes", setn(6, 129))
    case, L = first_launch("prompt_rows f32 H 264 n_text 5 n_ref 4")
    refused(case, L, "kind 3 with a null ref_codes", setp(2, None))
    refused(case, L, "kind 2 with a null spk", setp(3, None))
    case, L = first_launch("prompt_rows f32 H 264 n_text 5 n_ref 0")
    refused(case, L, "kind 3 with a null ref_codes (n_ref = 0)", setp(2, None))
    for prefix in ("kv_import f32 L 130 n_kv 2", "kv_export bf16 L 65 n_kv 1"):
        case, L = first_launch(prefix)
        refused(case, L, f"{prefix}: a block-table entry outside the pool", setn(3, 1))
        refused(case, L, f"{prefix}: a block stride that is no multiple of 16 bytes", setn(0, L.n[0] + 1))
        refused(case, L, f"{prefix}: a block stride below the block", setn(0, L.n[0] // 2))
        refused(case, L, f"{prefix}: more tiles than the table holds", setn(4, 0))
    case, L = first_launch("kv_adopt bf16 L 130")
    refused(case, L, "kv_adopt: a destination entry outside the pool", setn(3, 1))
    refused(case, L, "kv_adopt: a source entry outside the pool", setn(4, 1))
    refused(case, L, "kv_adopt: a block that is no multiple of 16 bytes", setn(2, L.n[2] + 4))
    refused(case, L, "kv_adopt: more than 128 tensors", setn(0, 129))
    case, L = first_launch("poll_gather B 3")
    refused(case, L, "more than 128 lanes", setn(0, 129))
    case, L = first_launch("text_publish_lanes B 5 items 2")
    refused(case, L, "more than 128 items", setn(0, 129))
    case, L = first_launch("text_scatter empty middle row_vec 33")
    refused(case, L, "more than 128 items", setn(0, 129))
    refused(case, L, "rows beyond the last item", setn(2, L.n[2] + 1))
    refused(case, L, "an item with more rows than its table holds", lambda a: a.iv2.__setitem__(0, 1))
    case, L = first_launch("kv_table_write first 3 count 5")
    refused(case, L, "entries beyond the table", setn(2, 7))
    refused(case, L, "more than 128 values", setn(1, 129))
    case, L = first_launch("decode_arm f32 H 264")
    refused(case, L, "a bitmap longer than the buffer", setn(0, R.MAX_VOCAB + 64))
    case, L = first_launch("trajectory A+B f32 single", )
    a = Device(case.mem).args(L)
    assert probe.state_probe_admits(len(R.KINDS), 0, C.byref(a)) == 0 and probe.state_probe_run(-1, 0, C.byref(a), None) == REFUSED


def test_zz_record(probe):
    """Prints the per-kernel record; every instantiation the probe builds was launched."""
    print()
    print(f"  {'kernel':<42}{'cases':>7}{'launches':>10}")
    for kind in R.KINDS:
        st = STATS[R.KERNEL[kind]]
        if st["cases"]:
            extra = ""
            if kind == "rmsnorm":
                extra = "   largest err / bound %.3f, exact fraction %s" % (st["ratio"], ", ".join(
                    "%s %.4f" % (dt, POOL.fraction("rmsnorm_kernel", dt)) for dt in R.DTS))
            print(f"  {R.KERNEL[kind]:<42}{st['cases']:>7}{st['launches']:>10}{extra}")
    buf = (C.c_int * 64)()
    want = set(buf[:probe.state_probe_insts(buf, 64)])
    if all(STATS[R.KERNEL[k]]["cases"] for k in R.KINDS):                 # (the whole module ran)
        assert REACHED == want, f"instantiations never launched: {sorted(want - REACHED)}"
        print(f"  instantiations launched: {len(REACHED)} of {len(want)}")
